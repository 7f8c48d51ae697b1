/* evg_pop_bf16.h -- self-royale on the bf16 matrix cores: the grouped forward of the two populations (evg.h: evg_population, evg_smart_population) in the
 * numeric mode of evg_qnet_bf16.h, for the acting turn and for the target networks of a team.  The entry points libevg_popbf16.so adds to those of
 * libevg_bf16.so.  The bit-exact fp32 grouped forwards of evg.h (evg_population_qnet, evg_smart_population_qnet) are as they were and stay the default. */
#ifndef EVG_POP_BF16_H
#define EVG_POP_BF16_H
#include "evg.h"
#include "evg_qnet_bf16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two functions under ABI 7.  They are NOT part of libevg.so or libevg_bf16.so: `make popbf16` builds libevg_popbf16.so from the same sources with
 * -DEVG_BF16 -DEVG_POP_BF16, which exports evg.h's entry points, the two of evg_qnet_bf16.h and these two.  A handle made by any of the libraries is
 * valid in the others; an error's text is read with the evg_last_error of the library whose call failed.
 *
 * Arguments, descriptors, layouts and the meaning of `member` and `seat` are those of evg_population_qnet and evg_smart_population_qnet, and so is
 * everything the call publishes in the descriptor: the stable lists in `index`, `first` / `count` of the 17 bins per seat slot (the layout follows the
 * call), zeros in q_out and the sticky EVG_POP_S_BAD_MEMBER for every row whose id is not below its team's size.  The bucket pass is the same three
 * launches; the fourth is the grouped forward on v_mfma_f32_16x16x32_bf16.  Four launches, no allocation, no synchronisation, capturable.  The weights
 * are fp32 and are read in place on every call.  The refusals (EVG_ERR_INVALID, nothing launched) are those of the fp32 entry points, with their text.
 *
 * Numeric contract.  Every Q row equals, BIT FOR BIT, what evg_minimized_qnet_bf16 / evg_smart_qnet_bf16 writes for that row in the same layout with
 * the weights of team[seat][member[row]].  This is items 1-10 of evg_qnet_bf16.h applied per row: the rows of a group of 16 are the columns of every
 * matrix-core product, a column of a result depends on that column of the B operand alone, and the instruction sequence is the plain kernels' own body
 * -- which 15 other rows share a row's group does not enter its arithmetic.  tests/population_bf16_cases.py composes the routing of the populations with
 * tests/qnet_bf16_model.py accordingly. */
EVG_API int evg_population_qnet_bf16(evg_handle* h, const evg_population* pop, int layout, int64_t rows, int seat, const uint8_t* member,
                                     const float* in0, const float* in1, float* q_out, void* stream);
EVG_API int evg_smart_population_qnet_bf16(evg_handle* h, const evg_smart_population* pop, int layout, int64_t rows, int seat, const uint8_t* member,
                                           const float* in0, const float* in1, float* q_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
