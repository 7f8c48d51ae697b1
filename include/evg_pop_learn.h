/* evg_pop_learn.h -- self-royale: the grouped forms of the learner step's kernels, so that ONE sampled batch trains every member of one team, each
 * transition routed to the member that played it (the reference's self-royale training scripts: every team member that played an episode learns from it).  The
 * entry points libevg_poplearn.so adds to those of libevg_learn.so; everglades_amd.PopulationLearner chains them with the grouped forwards of evg.h
 * (evg_smart_population_qnet / evg_population_qnet, EVG_QNET_EXPANDED). */
#ifndef EVG_POP_LEARN_H
#define EVG_POP_LEARN_H
#include "evg.h"
#include "evg_qnet_grad.h"
#include "evg_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Six functions under ABI 7.  They are NOT part of libevg.so, libevg_grad.so or libevg_learn.so: `make poplearn` builds libevg_poplearn.so from the
 * same sources with -DEVG_GRAD -DEVG_LEARN -DEVG_POP_LEARN, which exports everything libevg_learn.so does and these six.  A handle made by any of
 * the libraries is valid in the others; an error's text is read with the evg_last_error of the library whose call failed.
 *
 * ---- the lists ------------------------------------------------------------------------------------------------------------------------------------
 * Every grouped kernel reads who owns a row from the bucket pass that a grouped EXPANDED forward of the policy team on the batch's swarm_obs [B][59]
 * (one id per row, seat slot 0) has just left in its population descriptor (include/evg.h, "the layout follows the call"):
 *
 *   index [B]   the stable lists: member m's rows, ascending, at index[first[m] .. first[m] + count[m] - 1]; bin 16 holds the rows whose id is >= K
 *   first [17], count [17]
 *
 * R_m is member m's list and c_m = count[m].  Nothing is read back to the host: c_m, the shares of the grid and the divisors are device data.
 * A value outside its range (an index outside 0..B-1, a count or first outside the list) is clamped into it, as the grouped forwards do.
 *
 * ---- evg_td_head_grouped --------------------------------------------------------------------------------------------------------------------------
 * evg_td_head (evg_learn.h: the same operands, the same per-sample operations in the same order) applied once per member to the rows R_m as a batch of
 * c_m: position k of the list takes the place of sample k.  gq[b] is divided by c_m, loss[m] is the sum over R_m in evg_td_head's fixed order for a
 * batch of c_m (16-lane groups over list positions, G_m = min(ceil(c_m / 16), EVG_TD_HEAD_MAX_BLOCKS) workgroups) divided by c_m: bit for bit what
 * evg_td_head gives on the gathered rows.  The order is a function of the ids alone.  No floating-point atomics.
 *   loss [K]: loss[m] = 0.0f where c_m = 0.
 *   A row of bin 16 (no member): its gq row, its priority and its `estimated` are 0.0f; it is in no sum and no count.
 *   workspace: EVG_TD_HEAD_GROUPED_WORKSPACE_BYTES.   Launches: one of (min(ceil(B / 16), 1024), K + 1) workgroups, one of K.
 * Refusals: evg_td_head's for `td` (its `loss` is [K], its workspace the larger one), and NULL / misaligned lists, K outside 1..16, lists.batch != td.batch.
 *
 * ---- evg_smart_population_backward, evg_population_backward -----------------------------------------------------------------------------------------
 * evg_smart_qnet_backward / evg_minimized_qnet_backward (evg_qnet_grad.h: the same chain, tile maps and padded partials) once per member on the
 * rows R_m, with member m's parameters param[i][m] (i in the order w1, b1, w2, b2[, w3, b3]) into grad[i][m].  The grid is
 * (X, K) with X the plain launch's workgroups for B rows; member m uses live_m = min(ceil(c_m / 64), ceil(X c_m / B)) of its row of the grid -- the
 * share the grouped forward gives it -- and the other workgroups leave before staging anything.  Each live workgroup leaves one partial; the members'
 * partials are packed in member order, so there are at most X + K of them: EVG_POP_LEARN_MAX_PARTIALS.  A second launch sums, for each member, its
 * live_m partials in ascending order, clamps to [-clamp, clamp] if clamp > 0 and OVERWRITES the member's gradient tensors; c_m = 0 writes zeros.
 * The order of every sum is a function of (the ids, h1, h2, the device's CU count): two calls are bit-equal.  No floating-point atomics.
 *   workspace: 4 * EVG_POP_LEARN_MAX_PARTIALS * EVG_SMART_QNET_GRAD_PARTIAL (or EVG_MINI_QNET_GRAD_PARTIAL) bytes always suffice.
 * Refusals: B outside 1..EVG_TD_HEAD_MAX_BATCH, K outside 1..16, hidden sizes outside the family's range, any pointer of a member < K or of the lists
 * NULL or misaligned, a workspace smaller than the partials of this B need, a clamp that is negative or not finite.
 *
 * ---- evg_adam_step_grouped ------------------------------------------------------------------------------------------------------------------------
 * K workgroups of 1024 threads; workgroup m is evg_adam_step's single workgroup over member m's n tensors with member m's own 32-byte control block
 * ctl + 32 m.  One workgroup per block, so evg_adam_step's no-race argument holds per member.  A workgroup whose c_m is 0 returns before it reads or
 * writes anything: parameters, m, v and the control block of a member without rows stay bit-identical.
 * Refusals: evg_adam_step's, per member; K outside 1..16; count NULL.
 *
 * ---- evg_pop_learn_expand_ids ---------------------------------------------------------------------------------------------------------------------
 * out[b * repeat + s] = member[b]: a transition's id for each of its 12 next-state rows (what the grouped target forward takes), without a torch op.
 *
 * ---- evg_pop_learn_take_rows ----------------------------------------------------------------------------------------------------------------------
 * The grouped forwards are fp32.  Targets at bf16 (evg_qnet_bf16.h) are one plain bf16 forward per member over the whole batch into `src`, each
 * followed by this: dst[r][:] = src[r][:] where ids[r] == member, 0.0f where ids[r] >= num_members (a row of nobody), and untouched elsewhere.  After
 * the K pairs dst holds, bit for bit, every row through its own member's network.  One launch of ceil(rows * width / 256) workgroups of 256.
 * Refusals: NULL or misaligned pointers, K outside 1..16, member outside 0..K-1, rows outside 1..64 * EVG_TD_HEAD_MAX_BATCH, width outside 1..16. */
#define EVG_POP_LEARN_MAX_PARTIALS (EVG_QNET_GRAD_MAX_BLOCKS + EVG_POP_MAX_MEMBERS)
#define EVG_TD_HEAD_GROUPED_WORKSPACE_BYTES (4LL * EVG_TD_HEAD_MAX_BLOCKS * EVG_POP_MAX_MEMBERS)
#define EVG_POP_LEARN_MAX_TENSORS 6

typedef struct evg_pop_lists {
    const int32_t* index;              /* [batch] */
    const int32_t* first;              /* [17] */
    const int32_t* count;              /* [17] */
    int32_t num_members;               /* K: 1..16 */
    int32_t batch;                     /* B */
} evg_pop_lists;

typedef struct evg_td_head_grouped_args {
    uint32_t struct_size;              /* = sizeof(evg_td_head_grouped_args) */
    uint32_t reserved;                 /* 0 */
    evg_td_head_args td;               /* loss: [K]; workspace: EVG_TD_HEAD_GROUPED_WORKSPACE_BYTES */
    evg_pop_lists lists;
} evg_td_head_grouped_args;

typedef struct evg_pop_backward_args {
    uint32_t struct_size;              /* = sizeof(evg_pop_backward_args) */
    int32_t h1;
    int32_t h2;                        /* Smart_State only */
    int32_t final_relu;
    float clamp;
    uint32_t reserved;                 /* 0 */
    evg_pop_lists lists;
    const float* x;                    /* [B][59] */
    const float* gq;                   /* [B][OUT] */
    const float* param[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    float* grad[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    void* workspace;
    int64_t workspace_bytes;
} evg_pop_backward_args;

typedef struct evg_adam_grouped_args {
    uint32_t struct_size;              /* = sizeof(evg_adam_grouped_args) */
    int32_t n;                         /* tensors per member: 1..EVG_POP_LEARN_MAX_TENSORS */
    float lr, beta1, beta2, eps;
    float clamp;
    int32_t fresh_state;
    int32_t num_members;               /* K */
    uint32_t reserved;                 /* 0 */
    const int32_t* count;              /* [>= K]: c_m */
    void* ctl;                         /* K blocks of EVG_ADAM_CTL_BYTES */
    int64_t elements[EVG_POP_LEARN_MAX_TENSORS];   /* elements of tensor i: the members share their shapes */
    float* param[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    const float* grad[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    float* m[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
    float* v[EVG_POP_LEARN_MAX_TENSORS][EVG_POP_MAX_MEMBERS];
} evg_adam_grouped_args;

EVG_API int evg_pop_learn_expand_ids(evg_handle* h, const uint8_t* member, int32_t batch, int32_t repeat, uint8_t* out, void* stream);
EVG_API int evg_pop_learn_take_rows(evg_handle* h, const float* src, const uint8_t* ids, int32_t member, int32_t num_members, int64_t rows, int32_t width,
                                    float* dst, void* stream);
EVG_API int evg_td_head_grouped(evg_handle* h, const evg_td_head_grouped_args* a, void* stream);
EVG_API int evg_smart_population_backward(evg_handle* h, const evg_pop_backward_args* a, void* stream);
EVG_API int evg_population_backward(evg_handle* h, const evg_pop_backward_args* a, void* stream);
EVG_API int evg_adam_step_grouped(evg_handle* h, const evg_adam_grouped_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
