/* evg_dqn_learn.h -- the rest of the agents/DQN family's optimize_model on the device: the family's TD target, loss and dLoss/dQ for one batch
 * (evg_dqn_td_head: gather of the seven unravelled actions, topk(7) of the target network's 132 values, Huber or squared loss over B x 7 pairs) and one
 * Adam step over a LARGE network launched over a grid (evg_adam_step_wide).  The entry points libevg_dqnlearn.so adds to those of libevg_dqngrad.so:
 * with evg_dqn_qnet (evg_dqn.h) and evg_dqn_qnet_backward (evg_dqn_grad.h) they are the whole of agents/DQN/DQNAgent.py:220-290 (optimize_model) and
 * :294-337 (prioritized_optimize_model). */
#ifndef EVG_DQN_LEARN_H
#define EVG_DQN_LEARN_H
#include "evg_dqn_grad.h"
#include "evg_learn.h"       /* evg_adam_args, evg_adam_tensor, EVG_ADAM_*: evg_adam_step_wide takes evg_adam_step's descriptor */

#ifdef __cplusplus
extern "C" {
#endif

/* Two functions under ABI 7.  They are NOT part of any other library: `make dqnlearn` builds libevg_dqnlearn.so from the same sources with -DEVG_DQN
 * -DEVG_DQN_GRAD -DEVG_DQN_LEARN, which exports evg.h's entry points, the three of evg_dqn.h, evg_dqn_qnet_backward and these two (NOT evg_td_head /
 * evg_adam_step, which evg_learn.h only declares here).  A handle made by any of the libraries is valid in the others; an error's text is read with
 * the evg_last_error of the library whose call failed.
 *
 * ---- evg_dqn_td_head --------------------------------------------------------------------------------------------------------------------------------
 * All pointers are device pointers, contiguous, 16-byte aligned.
 *
 *   q_pred   [B][132] f32   the policy network on the states
 *   action   [B][7]   i64   the seven unravelled actions of a row (unit * 11 + node), as remember_game_state stores them
 *   q_next   [B][132] f32   the target network on the next states
 *   reward   [B]      f32
 *   not_done [B]      u8    (torch.bool storage) or NULL: NULL means no row is done (optimize_model has no mask)
 *   weights  [B]      f32   importance weights of a prioritized batch, or NULL
 *
 * Per sample b, every operation one fp32 operation in exactly this order (the build contracts nothing; tests/dqn_learn_model.py restates it):
 *
 *   n[0..6]   the seven largest elements of q_next[b][0..131] WITH multiplicity, descending (topk's values; which index a tie came from is immaterial)
 *   est[j]    (n[j] * gamma) + reward[b]          two roundings, as the reference's two torch ops; the product is replaced by 0.0f where
 *                                                 not_done[b] == 0
 *   td[j]     q_pred[b][action[b][j]] - est[j]
 *   HUBER:    e[j] = |td| < 1 ? (0.5f * td) * td : |td| - 0.5f;  with weights e[j] = w * e[j];  g[j] = (w * min(max(td, -1), 1)) / (float)(7B)
 *   SQUARED:  e[j] = (td * td) * w  (no weights: no multiplication);                          g[j] = ((2.0f * td) * w) / (float)(7B)
 *   row       ((((((e[0] + e[1]) + e[2]) + e[3]) + e[4]) + e[5]) + e[6])
 *   priority  SQUARED: row / 7.0f + 1e-5f         HUBER: (|td[0]| + ... + |td[6]|, j ascending) / 7.0f + 1e-5f
 *   gq[b][a]  0.0f, plus g[j] for every j with action[b][j] == a, j ascending: all 132 elements are written; duplicates add, as gather's backward does
 *   loss      (sum over b of row) / (float)(7B)
 *
 * The sum over b is evaluated in fp32 in a fixed order, evg_td_head's: workgroup g of G = min(ceil(B / 16), EVG_DQN_TD_MAX_BLOCKS) takes the sample
 * groups g, g + G, ... (16 samples each, one per 16 lanes); a 16-lane group adds its samples' rows in ascending order, the workgroup adds its 16
 * groups' sums in ascending order and leaves one partial in the workspace; a second launch adds the G partials (lane l the partials l, l + 64, ...,
 * then the 64 lanes in ascending order) and divides by (float)(7B).  The order is a function of B alone: two calls on the same operands give bit-equal
 * outputs.  No floating-point atomics.
 *
 * action[b][j] outside 0..131 is device data no host check can see.  Such a pair reads no q_pred element, has td = 0: it adds 0 to row and to gq and
 * counts 0 in the priority; its `estimated` is that of its operands.  Nothing is written outside the row.
 *
 * Outputs: gq [B][132] (what evg_dqn_qnet_backward takes), loss [1], priorities [B] or NULL, estimated [B][7] or NULL.
 * workspace: EVG_DQN_TD_WORKSPACE_BYTES, 16-byte aligned; its content is scratch.
 * Domain: finite operands.  -0.0f in q_next is outside the pinned domain for the bits of `estimated` (a tie between the two zeros has no defined
 * winner).  Two launches, no allocation, no synchronisation: capturable.
 *
 * How.  The sixteen lanes of a sample hold its q_next row in nine registers each, lane l the elements l, l + 16, ..., l + 128 (padding: -inf), so each
 * of the nine load instructions of a wavefront covers 64 contiguous bytes of each of its four samples and together they use every byte of the rows'
 * 528.  Seven selection rounds: a lane-local maximum, a maximum over the sixteen lanes by cross-lane (DPP) operations, and the LOWEST lane that holds
 * the maximum retires its FIRST register equal to it -- one instance, not every element equal to it: with the family's final ReLU a row is mostly
 * exact zeros.  Lane j < 7 keeps round j's value and forms pair j; the same sixteen lanes build the gq row in nine registers each and store it whole.
 *
 * Refusals (EVG_ERR_INVALID, nothing launched): NULL handle or descriptor, wrong struct_size; B outside 1..EVG_DQN_TD_MAX_BATCH; an unknown mode; a
 * gamma that is not finite; q_pred, action, q_next, reward, gq, loss or the workspace NULL; any given pointer not 16-byte aligned; a workspace smaller
 * than EVG_DQN_TD_WORKSPACE_BYTES. */
#define EVG_DQN_TD_HUBER 0             /* optimize_model: F.smooth_l1_loss */
#define EVG_DQN_TD_SQUARED 1           /* prioritized_optimize_model: ((q - expected) ** 2 * weights).mean() */
#define EVG_DQN_TD_ACTIONS 7
#define EVG_DQN_TD_MAX_BATCH (1 << 20)
#define EVG_DQN_TD_MAX_BLOCKS 1024
#define EVG_DQN_TD_WORKSPACE_BYTES (4LL * EVG_DQN_TD_MAX_BLOCKS)

typedef struct evg_dqn_td_head_args {
    uint32_t struct_size;              /* = sizeof(evg_dqn_td_head_args) */
    int32_t mode;                      /* EVG_DQN_TD_* */
    int32_t batch;                     /* B */
    float gamma;
    const float* q_pred;
    const int64_t* action;
    const float* q_next;
    const float* reward;
    const uint8_t* not_done;
    const float* weights;
    float* gq;
    float* loss;
    float* priorities;
    float* estimated;
    void* workspace;
    int64_t workspace_bytes;
} evg_dqn_td_head_args;

/* ---- evg_adam_step_wide ------------------------------------------------------------------------------------------------------------------------------
 * evg_adam_step (evg_learn.h) for a network too large for one workgroup: the same descriptor, the same ctl block, fresh_state, clamp, the same
 * double-precision bias terms and the same fp32 operations per element in the same order -- per element bit-equal to evg_adam_step -- launched over a
 * grid.  (The 105-528-132 network has 125 796 parameters: 123 dependent trips per thread of evg_adam_step's one workgroup.)
 *
 * Each tensor is cut into units of four consecutive elements, the last one shorter where the count is no multiple of 4; the units of the n tensors
 * form one flat index space.  A thread takes a unit: a full one with 128-bit loads and stores (every tensor base is 16-byte aligned), a short one
 * element by element.  G = min(ceil(units / 256), EVG_ADAM_WIDE_MAX_BLOCKS) workgroups of 256 threads stride over the units.
 *
 * ctl.  The element launch only READS ctl (every thread, before its loop).  A second launch of ONE thread on the same stream reads ctl again, forms
 * the same products and stores {step + 1, p1', p2'}: it starts after every workgroup of the element launch has finished, so no workgroup can read a
 * ctl that this call has advanced, and ctl advances exactly once per call.  No floating-point atomics, no allocation, no synchronisation: capturable.
 *
 * Refusals: evg_adam_step's, word for word. */
#define EVG_ADAM_WIDE_MAX_BLOCKS 512

EVG_API int evg_dqn_td_head(evg_handle* h, const evg_dqn_td_head_args* a, void* stream);
EVG_API int evg_adam_step_wide(evg_handle* h, const evg_adam_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
