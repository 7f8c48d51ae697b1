/* evg_qnet_grad.h -- the backward pass of the two Q networks' expanded fp32 forward: the parameter gradients that optimize_model's policy forward
 * needs, as one differentiable operation.  The entry points libevg_grad.so adds to those of libevg.so.  No loss, no targets, no optimizer: the caller
 * supplies the upstream gradient gq = dLoss/dQ and gets dLoss/d(parameters) back. */
#ifndef EVG_QNET_GRAD_H
#define EVG_QNET_GRAD_H
#include "evg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two functions under ABI 7.  They are NOT part of libevg.so, whose entry points are exactly those of evg.h: `make grad` builds libevg_grad.so from the
 * same sources with -DEVG_GRAD, which exports evg.h's entry points plus these two.  A handle made by either library is valid in the other (same
 * sources, one HIP runtime); an error's text is read with the evg_last_error of the library whose call failed.
 *
 * Contract.  For one network (num_sets 1) and `rows` expanded rows x [rows][59], let a1, a2 (Smart_State only) and q be the activations and the output
 * of evg.h's fmaf chain, bit for bit: the values evg_smart_qnet / evg_minimized_qnet compute in the EVG_QNET_EXPANDED layout, recomputed here by the
 * same matrix-core chain.  Given gq [rows][OUT] (OUT = 5, or 11 for the Minimized network):
 *
 *     d3  = gq * (final_relu ? (q > 0) : 1)                  torch's ReLU backward: the derivative at 0 is 0
 *     gb3 = sum_r d3[r]          gW3 = sum_r d3[r] (x) a2[r]
 *     d2  = (W3^T d3) * (a2 > 0)
 *     gb2 = sum_r d2[r]          gW2 = sum_r d2[r] (x) a1[r]
 *     d1  = (W2^T d2) * (a1 > 0)
 *     gb1 = sum_r d1[r]          gW1 = sum_r d1[r] (x) x[r]
 *
 * (the Minimized network, 59 -> h1 -> 11, has one hidden layer fewer: d2 = gq * mask, gb2, gW2 = sum d2 (x) a1, d1 = (W2^T d2) * (a1 > 0), gb1, gW1).
 *
 *   1. The masks and the activations that enter the outer products are those of the exact fp32 chain: a pre-activation near zero cannot fall on the
 *      other side of its mask.
 *   2. The sums W^T d and sum_r are evaluated in fp32 (one rounding per product-and-add), in an order that is not part of the contract ...
 *   3. ... but is a function of (rows, h1, h2, the device's CU count) alone: two calls on the same operands return bit-equal gradients.  No
 *      floating-point atomics.
 *   4. There is no gradient with respect to x.
 *   5. The output tensors are overwritten, not accumulated into; exactly the nn.Linear shapes are written (w1 [h1][59], b1 [h1], w2 [h2][h1], ...).
 *   6. A padded hidden unit (index >= h1, >= h2) contributes exactly nothing.
 *   7. `clamp` > 0 clamps every gradient element to [-clamp, clamp] after the sum (param.grad.data.clamp_(-1, 1)); 0 means none.
 *   8. Domain: finite x, parameters and gq.  Non-finite values are outside the pinned domain: what they produce is not specified.
 *
 * Two launches (the backward kernel, whose every workgroup leaves one partial sum in `workspace`, and a reduction over the workgroups in ascending
 * order); no allocation, no synchronisation, capturable.  The grid is min(ceil(rows / 64), 2 * CUs, EVG_QNET_GRAD_MAX_BLOCKS) workgroups; the workspace
 * must hold one partial for each: EVG_*_QNET_GRAD_WORKSPACE_BYTES is enough for any rows on any device.  A workgroup's four wavefronts take 16 rows each
 * at a time: one sweep of the capped grid is EVG_QNET_GRAD_MAX_BLOCKS * 64 rows.
 *
 * Refusals (EVG_ERR_INVALID, nothing launched): those of the fp32 entry points for the handle, the descriptor and rows; num_sets != 1; x, gq, a
 * gradient pointer or the workspace NULL or not 16-byte aligned; a workspace smaller than the grid of this call needs; a clamp that is negative or
 * not finite. */
#define EVG_QNET_GRAD_MAX_BLOCKS 512
#define EVG_SMART_QNET_GRAD_PARTIAL 9360       /* floats per workgroup: gW1 [64][64], gW2 [64][64], gW3 [16][64], gb1 [64], gb2 [64], gb3 [16] */
#define EVG_MINI_QNET_GRAD_PARTIAL 10384       /* gW1 [128][64], gW2 [16][128], gb1 [128], gb2 [16] */
#define EVG_SMART_QNET_GRAD_WORKSPACE_BYTES (4LL * EVG_QNET_GRAD_MAX_BLOCKS * EVG_SMART_QNET_GRAD_PARTIAL)
#define EVG_MINI_QNET_GRAD_WORKSPACE_BYTES (4LL * EVG_QNET_GRAD_MAX_BLOCKS * EVG_MINI_QNET_GRAD_PARTIAL)

typedef struct evg_qnet_grads {        /* where the gradients go: the shapes of the descriptor's tensors */
    uint32_t struct_size;              /* = sizeof(evg_qnet_grads) */
    uint32_t reserved;                 /* 0 */
    float* w1;
    float* b1;
    float* w2;
    float* b2;
    float* w3;
    float* b3;
} evg_qnet_grads;

typedef struct evg_mini_qnet_grads {
    uint32_t struct_size;              /* = sizeof(evg_mini_qnet_grads) */
    uint32_t reserved;                 /* 0 */
    float* w1;
    float* b1;
    float* w2;
    float* b2;
} evg_mini_qnet_grads;

EVG_API int evg_smart_qnet_backward(evg_handle* h, const evg_qnet* net, int64_t rows, const float* x, const float* gq, const evg_qnet_grads* grads,
                                    void* workspace, int64_t workspace_bytes, float clamp, void* stream);
EVG_API int evg_minimized_qnet_backward(evg_handle* h, const evg_mini_qnet* net, int64_t rows, const float* x, const float* gq,
                                        const evg_mini_qnet_grads* grads, void* workspace, int64_t workspace_bytes, float clamp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
