/* evg_replay_priority.h -- prioritized sampling over the Smart_State replay memory of evg.h (evg_replay_*): the entry points libevg_priority.so adds to
 * those of libevg.so.  The plane layout and the stamp are listed with the memory's buffers in evg.h. */
#ifndef EVG_REPLAY_PRIORITY_H
#define EVG_REPLAY_PRIORITY_H
#include "evg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one more status bit of the memory's ctl[1]: a priority update got a priority that is NaN, infinite or <= 0 (skipped) */
enum { EVG_REPLAY_S_BAD_PRIORITY = 4 };
#define EVG_REPLAY_PSCAN_WORDS(slots, N, S) (((int64_t)(slots) * (N) * (S) + 3) / 4 + 2 * (((int64_t)(slots) * (N) * (S) + 1023) / 1024))

/* ---- Prioritized sampling over the replay memory (agents/DQN/PrioritizedMemory.py: sample / update_priorities) -------------------------------------
 * Three functions and one descriptor under ABI 7.  They are NOT part of libevg.so, whose entry points are exactly those of evg.h: `make priority` builds
 * libevg_priority.so from the same sources with -DEVG_PRIORITY, which exports evg.h's entry points plus these three (as libevg_diag.so adds its
 * configure call).  A handle made by either library is valid in the other (same sources, one HIP runtime); an error's text is read with the
 * evg_last_error of the library whose call failed.  evg_replay_sample and every other entry point are as they were.  The library stores the
 * priorities the consumer hands back and draws by them; the TD error, autograd and the optimizer stay the consumer's.  Three differences from the
 * reference class, next to the two of the memory itself:
 *   1. A transition that was never updated weighs wmax AS OF THE DRAW, wmax being the largest weight stored since the last clear (monotone).  The
 *      reference fixes priorities.max() -- over the current values -- at push time.
 *   2. When one update names a transition several times, the LARGEST priority is kept (the reference's Python loop keeps the last).  Draws are with
 *      replacement, so duplicates are normal; they carry one TD error whenever the consumer computed them from one network.
 *   3. Probabilities are q / Q with integer weights: with frexp(wmax) = (m, e), q = max(1, (uint64) ldexp((double) w, 32 - e)), w the stored weight or
 *      wmax.  Weights are thus quantised to 2^-32 of the maximum and floored at one unit (nothing is undrawable); q < 2^32, the heaviest transition has
 *      q >= 2^31, and Q fits 64 bits for every size the memory admits.  The draws are exact integer arithmetic: a host model reproduces them bit for bit.
 */
typedef struct evg_replay_priority {
    float alpha;                   /* in [0, 1]: w = priority ** alpha                                                      */
    float* plane;                  /* float [slots][N][S][8], 16-byte aligned                                               */
    unsigned long long* pscan;     /* uint64 [EVG_REPLAY_PSCAN_WORDS(slots, N, S)], 8-byte aligned                          */
    unsigned long long* pctl;      /* uint64 [4], 8-byte aligned                                                            */
} evg_replay_priority;

/* Zeroes the plane and sets wmax = 1.0f.  Call it with evg_replay_clear (which resets the status bits).  Enqueued on `stream`. */
EVG_API int evg_replay_priority_clear(evg_handle* h, const evg_replay* m, const evg_replay_priority* p, void* stream);
/* update_priorities: handles int32 [batch][4] (16-byte aligned) as a sample returned them, priorities float [batch].  Stores
 * w = (float) pow((double) priority, (double) alpha) -- alpha == 1 gives the priority itself, alpha == 0 gives 1.0f, a positive result below FLT_MIN
 * becomes FLT_MIN -- at the transition's entry of the plane and raises wmax to it.  A priority that is NaN, infinite or <= 0 is skipped and sets
 * EVG_REPLAY_S_BAD_PRIORITY in ctl[1]; a handle that names no transition is skipped and sets EVG_REPLAY_S_BAD_HANDLE.  Two launches (reset, then an
 * atomic maximum), so that the result does not depend on thread order: of several priorities for one transition the largest is kept. */
EVG_API int evg_replay_update_priorities(evg_handle* h, const evg_replay* m, const evg_replay_priority* p, int batch, const int32_t* handles,
                                         const float* priorities, void* stream);
/* evg_replay_sample drawing by weight (five launches: scan, top, draw, weights, gather): draw i takes u = (word 0 << 32) | word 1 of
 * Philox((i, call index, 7), seed), t = the high 64 bits of u * Q, and names the transition that holds position t of the integer weights laid out in
 * record order.  The call index is the memory's own (ctl[0] / ctl[3]): uniform and prioritized samples share one counter.
 *   weights_out  float [batch] (16-byte aligned): (T q_i / Q) ** -beta in float64, T the transition count (ctl[2]), divided by the batch's largest and
 *                rounded once; beta == 0 gives exactly 1.0f
 * An empty memory gives handles of -1, zero outputs and weights, and EVG_REPLAY_S_EMPTY, as in evg_replay_sample. */
EVG_API int evg_replay_sample_prioritized(evg_handle* h, const evg_replay* m, int batch, uint64_t seed, float* swarm_obs, int64_t* action,
                                          float* next_state, float* reward, uint8_t* not_done, int32_t* handles, const evg_replay_priority* p, float beta,
                                          float* weights_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
