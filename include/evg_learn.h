/* evg_learn.h -- the glue of a DQN learner's optimize_model on the device: the TD target, the Huber loss and its gradient with respect to Q for one
 * sampled batch (evg_td_head), and one Adam step over all parameter tensors of one network (evg_adam_step).  The entry points libevg_learn.so adds to
 * those of libevg.so and libevg_grad.so: with the forwards of evg.h / evg_qnet_bf16.h and the backward of evg_qnet_grad.h they are the whole of
 * agents/Smart_State/DQNAgent.py:336-385, agents/Minimized/DQNAgent.py and agents/Minimized_Rainbow/DQNAgent.py:279-327 (the double-DQN target). */
#ifndef EVG_LEARN_H
#define EVG_LEARN_H
#include "evg.h"
#include "evg_qnet_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two functions under ABI 7.  They are NOT part of libevg.so: `make learn` builds libevg_learn.so from the same sources with -DEVG_LEARN -DEVG_GRAD,
 * which exports evg.h's entry points, the two of evg_qnet_grad.h and these two, so that a learner needs one extra library.  A handle made by any of
 * the libraries is valid in the others; an error's text is read with the evg_last_error of the library whose call failed.
 *
 * ---- evg_td_head ------------------------------------------------------------------------------------------------------------------------------------
 * All pointers are device pointers, contiguous, 16-byte aligned.  S = EVG_TD_SWARMS = 12.
 *
 *   q_pred   [B][OUT]    f32   the policy forward on swarm_obs
 *   action   [B]         i64   the column of q_pred the transition took
 *   q_next   [B][S][OUT] f32   the target network on next_state_swarms
 *   q_select [B][S][OUT] f32   the policy network on next_state_swarms: EVG_TD_DOUBLE_MEAN only, NULL otherwise (ignored if given)
 *   reward   [B]         f32
 *   not_done [B]         u8    (torch.bool storage): 0 is "done", anything else "not done"
 *   weights  [B]         f32   importance weights of a prioritized batch, or NULL (w = 1)
 *
 * Per sample b, every operation one fp32 operation in exactly this order (the build contracts nothing; tests/learner_model.py follows it):
 *
 *   v[s]      EVG_TD_MAX_MEAN, EVG_TD_MAX_MAX:  max over a of q_next[b][s][a]
 *             EVG_TD_DOUBLE_MEAN:               q_next[b][s][a*], a* the FIRST index at which q_select[b][s][.] takes its maximum
 *   future    _MEAN modes:  ((...((v[0] + v[1]) + v[2]) + ...) + v[11]) / 12.0f     (s ascending, then one division)
 *             EVG_TD_MAX_MAX: max over s of v[s]
 *             0.0f where not_done[b] == 0, whatever q_next / q_select hold there (they are still read: they must be readable, they need not be finite)
 *   estimated fmaf(future, scale, reward[b])                                        (one rounding)
 *   td        q_pred[b][action[b]] - estimated
 *   term      |td| < 1 ?  (0.5f * td) * td  :  |td| - 0.5f                          (|td| == 1 takes the linear branch, as smooth_l1_loss with beta 1)
 *   wterm     w * term                                                              (no multiplication when weights is NULL)
 *   gq[b][a]  a == action[b] ?  (w * min(max(td, -1.0f), 1.0f)) / (float)B  :  0.0f  (every element of gq is written)
 *   priority  |td| + 1e-5f
 *   loss      (sum over b of wterm) / (float)B
 *
 * The sum over b is evaluated in fp32 in a fixed order: workgroup g of G = min(ceil(B / 16), EVG_TD_HEAD_MAX_BLOCKS) takes the sample groups
 * g, g + G, ... (16 samples each, one per 16 lanes); a 16-lane group adds its samples' wterm in ascending order, the workgroup adds its 16 groups'
 * sums in ascending order and leaves one partial in the workspace; a second launch adds the G partials (lane l the partials l, l + 64, ..., then the
 * 64 lanes in ascending order) and divides by B.  The order is a function of B alone: two calls on the same operands give a bit-equal loss.  No
 * floating-point atomics.
 *
 * action[b] outside 0..OUT-1 is device data no host check can see.  Such a row reads no q_pred element, writes zeros to its whole gq row, adds 0 to
 * the loss and gets the priority 1e-5f and the `estimated` of its operands.  Nothing is written outside the row.
 *
 * Outputs: gq [B][OUT] (exactly what evg_*_qnet_backward takes), loss [1], priorities [B] or NULL, estimated [B] or NULL.
 * workspace: EVG_TD_HEAD_WORKSPACE_BYTES, 16-byte aligned; its content is scratch.
 * Domain: finite operands (q_next / q_select of done rows excepted).  Two launches, no allocation, no synchronisation: capturable.
 *
 * Memory access: 16 lanes own one sample; lane s < 12 reads the OUT consecutive floats of swarm s, so each load instruction of a wavefront covers the
 * four samples' contiguous 4 * 12 * OUT floats at a stride of OUT floats and the OUT loads together use every byte of every line touched.
 *
 * Refusals (EVG_ERR_INVALID, nothing launched): NULL handle or descriptor, wrong struct_size; B outside 1..EVG_TD_HEAD_MAX_BATCH; OUT not 5 or 11;
 * an unknown mode; a scale that is not finite; q_pred, action, q_next, reward, not_done, gq, loss or the workspace NULL; q_select NULL in the double
 * mode; any given pointer not 16-byte aligned; a workspace smaller than EVG_TD_HEAD_WORKSPACE_BYTES. */
#define EVG_TD_SWARMS 12
#define EVG_TD_MAX_MEAN 0            /* Smart_State, Minimized: amax over actions, mean over swarms */
#define EVG_TD_MAX_MAX 1             /* Blind: amax over actions, amax over swarms */
#define EVG_TD_DOUBLE_MEAN 2         /* Minimized_Rainbow: the policy network selects, the target network evaluates, mean over swarms */
#define EVG_TD_HEAD_MAX_BATCH (1 << 20)
#define EVG_TD_HEAD_MAX_BLOCKS 1024
#define EVG_TD_HEAD_WORKSPACE_BYTES (4LL * EVG_TD_HEAD_MAX_BLOCKS)

typedef struct evg_td_head_args {
    uint32_t struct_size;              /* = sizeof(evg_td_head_args) */
    int32_t mode;                      /* EVG_TD_* */
    int32_t batch;                     /* B */
    int32_t out;                       /* OUT: 5 or 11 */
    float scale;                       /* gamma ** n_step */
    uint32_t reserved;                 /* 0 */
    const float* q_pred;
    const int64_t* action;
    const float* q_next;
    const float* q_select;
    const float* reward;
    const uint8_t* not_done;
    const float* weights;
    float* gq;
    float* loss;
    float* priorities;
    float* estimated;
    void* workspace;
    int64_t workspace_bytes;
} evg_td_head_args;

/* ---- evg_adam_step ----------------------------------------------------------------------------------------------------------------------------------
 * torch.optim.Adam with weight_decay 0, amsgrad False, maximize False, over the n tensors of one network, in place, in one launch.
 *
 * ctl is a 32-byte device block { int64 step; double beta1_pow; double beta2_pow; int64 reserved } holding the number of steps taken and
 * beta1 ** step, beta2 ** step as running products in double (a new optimizer: {0, 1.0, 1.0, 0}).  A call reads (step, p1, p2) -- or, with
 * fresh_state != 0, takes (0, 1.0, 1.0) and reads every m and v as 0.0f -- and computes, once, in double:
 *
 *   p1' = p1 * (double)beta1     p2' = p2 * (double)beta2
 *   step_size = (float)((double)lr / (1.0 - p1'))          bc2s = (float)sqrt(1.0 - p2')
 *
 * and then per element, every operation one fp32 operation in exactly this order (omb1 = 1.0f - beta1, omb2 = 1.0f - beta2):
 *
 *   g   = clamp > 0 ?  min(max(grad, -clamp), clamp)  :  grad
 *   m'  = m + (g - m) * omb1
 *   v'  = beta2 * v + (omb2 * g) * g
 *   den = sqrtf(v') / bc2s + eps                           (sqrtf and / correctly rounded)
 *   p'  = p - step_size * (m' / den)
 *
 * m', v', p' are stored; ctl becomes {step + 1, p1', p2'}.  With fresh_state the stored m, v and ctl hold this one step's values: what constructing
 * optim.Adam anew inside every optimize_model call does (Smart_State, Minimized).
 *
 * The launch is ONE workgroup of 1024 threads that loops over the elements (a network here has at most 9 099).  Every thread reads ctl before
 * the loop; thread 0 stores the advanced ctl after a workgroup barrier that all threads reach after their reads.  There is no other workgroup, so
 * nothing reads ctl after the store: no race, and ctl advances exactly once per call.
 *
 * Refusals (EVG_ERR_INVALID, nothing launched): NULL handle or descriptor, wrong struct_size; n outside 1..EVG_ADAM_MAX_TENSORS; a count outside
 * 1..EVG_ADAM_MAX_COUNT; a param, grad, m, v or ctl pointer NULL or not 16-byte aligned; lr not finite; beta1 or beta2 outside [0, 1); eps not > 0
 * or not finite; a clamp that is negative or not finite.
 * Domain: finite operands.  No allocation, no synchronisation: capturable. */
#define EVG_ADAM_MAX_TENSORS 6
#define EVG_ADAM_MAX_COUNT (1 << 24)
#define EVG_ADAM_CTL_BYTES 32

typedef struct evg_adam_tensor {
    float* param;
    const float* grad;
    float* m;
    float* v;
    int64_t count;
} evg_adam_tensor;

typedef struct evg_adam_args {
    uint32_t struct_size;              /* = sizeof(evg_adam_args) */
    int32_t n;                         /* tensors: 1..EVG_ADAM_MAX_TENSORS */
    float lr, beta1, beta2, eps;
    float clamp;                       /* > 0: clamp each gradient element as it is read; 0: none */
    int32_t fresh_state;
    void* ctl;
    evg_adam_tensor t[EVG_ADAM_MAX_TENSORS];
} evg_adam_args;

EVG_API int evg_td_head(evg_handle* h, const evg_td_head_args* a, void* stream);
EVG_API int evg_adam_step(evg_handle* h, const evg_adam_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
