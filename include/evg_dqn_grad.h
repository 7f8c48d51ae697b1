/* evg_dqn_grad.h -- the backward pass of the agents/DQN family's Q network, QNetwork(105 -> h1 -> 132) of evg_dqn.h: the parameter gradients that
 * optimize_model's policy forward needs, as one differentiable operation.  The entry point libevg_dqngrad.so adds to those of libevg_dqn.so.  No loss,
 * no targets, no optimizer: the caller supplies the upstream gradient gq = dLoss/dQ and gets dLoss/d(parameters) back. */
#ifndef EVG_DQN_GRAD_H
#define EVG_DQN_GRAD_H
#include "evg_dqn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One function under ABI 7.  It is NOT part of libevg.so or libevg_dqn.so, whose entry points are exactly those of evg.h and evg_dqn.h: `make dqngrad`
 * builds libevg_dqngrad.so from the same sources with -DEVG_DQN -DEVG_DQN_GRAD, which exports evg.h's entry points, the three of evg_dqn.h and this
 * one.  A handle made by any of the libraries is valid in the others (same sources, one HIP runtime); an error's text is read with the evg_last_error
 * of the library whose call failed.
 *
 * Contract.  For `rows` rows x [rows][105], let a1 be the hidden activations of evg_dqn.h's fmaf chain, bit for bit -- recomputed here by the same
 * matrix-core chain as evg_dqn_qnet's -- and q that chain's output, which the caller passes in (evg_dqn_qnet's output for x and net; only its sign is
 * read, and only with final_relu).  Given gq [rows][132]:
 *
 *     d2  = gq * (final_relu ? (q > 0) : 1)                  torch's ReLU backward: the derivative at 0 is 0
 *     gb2 = sum_r d2[r]          gW2 = sum_r d2[r] (x) a1[r]
 *     d1  = (W2^T d2) * (a1 > 0)
 *     gb1 = sum_r d1[r]          gW1 = sum_r d1[r] (x) x[r]
 *
 *   1. The masks and the activations that enter the outer products are those of the exact fp32 chain: a pre-activation near zero cannot fall on the
 *      other side of its mask.
 *   2. The sums W2^T d2 and sum_r are evaluated in fp32 (one rounding per product-and-add), in an order that is not part of the contract ...
 *   3. ... but is a function of (rows, h1, the device's CU count) alone: two calls on the same operands return bit-equal gradients.  No
 *      floating-point atomics.
 *   4. There is no gradient with respect to x.
 *   5. The output tensors are overwritten, not accumulated into; exactly the nn.Linear shapes are written (w1 [h1][105], b1 [h1], w2 [132][h1],
 *      b2 [132]).
 *   6. A padded hidden unit (>= h1), input column (>= 105) or output (>= 132) contributes exactly nothing: by selection, as in the forward.
 *   7. `clamp` > 0 clamps every gradient element to [-clamp, clamp] after the sum (param.grad.data.clamp_(-1, 1)); 0 means none.
 *   8. Domain: finite x, parameters, q and gq.  Non-finite values are outside the pinned domain: what they produce is not specified.
 *
 * How.  This network's parameter set is 503 KB at h1 = 528: a workgroup cannot hold one, so the weight gradients are computed tile-parallel, not
 * row-parallel as evg_qnet_grad.h's are.  Two launches, or three:
 *   - the delta kernel, row-parallel with evg_dqn_qnet's structure (chunks of EVG_DQN_CHUNK hidden units, the same staging): per chunk it recomputes
 *     layer 1, forms d1's tile from the row group's d2 fragments against the staged W2 columns, and stores a1 and the masked d1 to the workspace as
 *     [rows][HP] floats each, HP = h1 rounded up to 16.  16 rows per workgroup pass up to EVG_DQN_GRAD_TINY_ROWS rows (the wavefronts share the row
 *     group and split the chunk's column tiles), 64 beyond; min(passes, EVG_DQN_GRAD_MAX_BLOCKS) workgroups stride over the passes;
 *   - the weight-gradient kernel: a wavefront owns hidden tile t (16 units) -- gW2's nine 16 x 16 tiles [:, t] and gW1's seven [t, :], 64 accumulator
 *     registers -- and runs down the rows in ascending k-steps of 4 rows; a workgroup's four wavefronts share the staged d2 and x blocks.  The bias
 *     gradients are the sums of the same operand fragments.  Rows are cut into S = EVG_DQN_GRAD_SLICES(rows) or fewer slices of equal length, one
 *     workgroup column each;
 *   - with more than one slice, a reduction that adds the slices' partial sums in ascending slice order and clamps.  (One slice: the weight-gradient
 *     kernel clamps and stores the gradients itself.)
 * No allocation, no synchronisation, capturable.
 *
 * Refusals (EVG_ERR_INVALID, nothing launched): those of evg_dqn_qnet for the handle and the descriptor; rows outside 1..EVG_DQN_GRAD_MAX_ROWS; x, gq,
 * a gradient pointer or the workspace NULL or not 16-byte aligned; q NULL with final_relu, or not 16-byte aligned; a NULL gradient descriptor or a
 * wrong struct_size; a workspace smaller than EVG_DQN_GRAD_WORKSPACE_BYTES(rows, h1); a clamp that is negative or not finite. */
#define EVG_DQN_GRAD_MAX_ROWS (1 << 16)
#define EVG_DQN_GRAD_TINY_ROWS 4096         /* up to here the delta kernel's workgroup pass is one 16-row group, beyond it 64 rows */
#define EVG_DQN_GRAD_MAX_BLOCKS 256         /* the delta kernel's grid cap: one sweep of the capped grid is 256 * 64 rows          */
#define EVG_DQN_GRAD_SLICE_ROWS 128         /* the weight-gradient kernel: no slice of the rows is shorter than this ...           */
#define EVG_DQN_GRAD_MAX_SLICES 56          /* ... and no more slices than this: 9 x 56 workgroups (h1 = 528) are resident at once */
#define EVG_DQN_GRAD_HP(h1) (((int64_t)(h1) + 15) / 16 * 16)
#define EVG_DQN_GRAD_SLICES(rows) \
    ((int64_t)(rows) <= EVG_DQN_GRAD_SLICE_ROWS ? 1 : ((int64_t)(rows) + EVG_DQN_GRAD_SLICE_ROWS - 1) / EVG_DQN_GRAD_SLICE_ROWS < EVG_DQN_GRAD_MAX_SLICES \
        ? ((int64_t)(rows) + EVG_DQN_GRAD_SLICE_ROWS - 1) / EVG_DQN_GRAD_SLICE_ROWS : EVG_DQN_GRAD_MAX_SLICES)
/* floats of one slice's partial sums: gW2 [144][HP], gW1 [HP][112], gb2 [144], gb1 [HP] */
#define EVG_DQN_GRAD_PARTIAL(h1) (257 * EVG_DQN_GRAD_HP(h1) + 144)
/* what one call needs: a1 and d1, and one partial per slice where there is more than one; a function of rows and h1 only */
#define EVG_DQN_GRAD_WORKSPACE_BYTES(rows, h1) \
    (8 * (int64_t)(rows) * EVG_DQN_GRAD_HP(h1) + (EVG_DQN_GRAD_SLICES(rows) > 1 ? 4 * EVG_DQN_GRAD_SLICES(rows) * EVG_DQN_GRAD_PARTIAL(h1) : 0))

typedef struct evg_dqn_grads {         /* where the gradients go: the nn.Linear shapes of evg_dqn_net */
    uint32_t struct_size;              /* = sizeof(evg_dqn_grads) */
    uint32_t reserved;                 /* 0 */
    float* w1;
    float* b1;
    float* w2;
    float* b2;
} evg_dqn_grads;

EVG_API int evg_dqn_qnet_backward(evg_handle* h, const evg_dqn_net* net, int64_t rows, const float* x, const float* q, const float* gq,
                                  const evg_dqn_grads* grads, void* workspace, int64_t workspace_bytes, float clamp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
