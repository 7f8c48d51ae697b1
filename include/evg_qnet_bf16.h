/* evg_qnet_bf16.h -- the two Q networks' reduced-precision forward on the bf16 matrix cores, for acting and for the target network: the entry points
 * libevg_bf16.so adds to those of libevg.so.  The bit-exact fp32 evaluators of evg.h (evg_smart_qnet, evg_minimized_qnet) are as they were and stay
 * the default; this is a second numeric mode beside them. */
#ifndef EVG_QNET_BF16_H
#define EVG_QNET_BF16_H
#include "evg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two functions under ABI 7.  They are NOT part of libevg.so, whose entry points are exactly those of evg.h: `make bf16` builds libevg_bf16.so from the
 * same sources with -DEVG_BF16, which exports evg.h's entry points plus these two.  A handle made by either library is valid in the other (same
 * sources, one HIP runtime); an error's text is read with the evg_last_error of the library whose call failed.
 *
 * Arguments, layouts (EVG_QNET_COMPACT, EVG_QNET_COMPACT_SEATS: seat p through weight set p, EVG_QNET_EXPANDED), descriptors and refusals
 * (EVG_ERR_INVALID, nothing launched) are those of evg_smart_qnet and evg_minimized_qnet.  The weights are fp32 and are read in place on every call
 * (converted while they are staged); one launch, no allocation, no synchronisation, capturable.  Every layer runs on v_mfma_f32_16x16x32_bf16.
 *
 * Numeric contract (tests/qnet_bf16_model.py restates it):
 *    1. Every input is rounded x~ = bf16_rne(x): the 59 features, in the compact layouts the 34 shared and the 13 swarm features.
 *    2. Every weight is rounded W~ = bf16_rne(W).  Biases stay fp32.
 *    3. The one-hot term of the compact layouts is W~1[j][47 + s] (here: a product with an input of 1.0 inside the matrix core).
 *    4. A pre-activation is b[j] + sum over k of W~[j][k] * in[k]; the products are exact.
 *    5. Accumulation is in fp32; its order and the matrix core's internal rounding are not part of the contract.
 *    6. A hidden activation is bf16_rne(relu(pre)), the ReLU being pre < 0 ? 0 : pre: a NaN stays a NaN.
 *    7. The output layer is the fp32 pre-activation, through the same ReLU when final_relu is set; it is not rounded.
 *    8. Padded hidden units (index >= h1 or >= h2) enter the next layer as exact zeros whatever their accumulators hold: a non-finite input times a
 *       zero pad does not leak a NaN.
 *    9. The sign of a zero is not part of the contract.
 *   10. Inputs or weights that are bf16 subnormals (after rounding) are outside the pinned domain.
 * The compact and the expanded form of the same features agree within the accumulation order of item 5, not bit for bit. */
EVG_API int evg_smart_qnet_bf16(evg_handle* h, const evg_qnet* net, int layout, int64_t rows, const float* in0, const float* in1, float* q_out,
                                void* stream);
EVG_API int evg_minimized_qnet_bf16(evg_handle* h, const evg_mini_qnet* net, int layout, int64_t rows, const float* in0, const float* in1, float* q_out,
                                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
