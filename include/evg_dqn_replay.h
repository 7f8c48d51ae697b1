/* evg_dqn_replay.h -- the agents/DQN family's replay memory of RAW OBSERVATIONS on the device: what DQNAgent.remember_game_state,
 * SimpleMemory.ReplayMemory and the batch assembly of optimize_model do (agents/DQN/DQNAgent.py:199-337, SimpleMemory.py), per env, with no torch op
 * and no host synchronisation between the step and the batch.  The entry points libevg_dqnreplay.so adds to those of libevg_dqnlearn.so. */
#ifndef EVG_DQN_REPLAY_H
#define EVG_DQN_REPLAY_H
#include "evg_dqn_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Eight functions under ABI 7.  They are NOT part of any other library: `make dqnreplay` builds libevg_dqnreplay.so from the same sources with
 * -DEVG_DQN -DEVG_DQN_GRAD -DEVG_DQN_LEARN -DEVG_DQN_REPLAY, so that a learner step from the memory needs this one library.  A handle made by any of
 * the libraries is valid in the others; an error's text is read with the evg_last_error of the library whose call failed.
 *
 * ---- the ring ------------------------------------------------------------------------------------------------------------------------------------------
 * Storage is caller-owned device memory described by an evg_dqn_replay descriptor, allocated once (everglades_amd.DqnReplay does it).  It is a ring of
 * `slots` = H + 1 TURNS.  Slot t % slots holds, for every env,
 *
 *   obs       the seat's observation of turn t in the HANDLE'S OWN obs_dtype (float32, float64 or int16: 420, 840 or 210 bytes a row), [N][105] at
 *             obs + slot * EVG_DQN_REPLAY_OBS_STRIDE(N, element size) BYTES.  The stride pads a slot to 16 bytes so that every slot base is what
 *             evg_observe / evg_step_vs_policy take as their output and evg_dqn_qnet as its input: the step of turn t - 1 WRITES the slot, the network
 *             of turn t READS it, and the memory stores it once -- `state` of record t and `next_state` of record t - 1.  Nothing copies an observation.
 *   actions   int32 [N][7][2] {unit, node} at actions + slot * EVG_DQN_REPLAY_ACT_STRIDE(N) ints: what evg_dqn_get_action wrote and the step played
 *   reward    double [slots][N]        the turn's shaped reward
 *   meta      int32 [slots][N][4]      {turn number in the episode, episode index on the handle, flags EVG_REPLAY_F_NOT_DONE, 0}
 *   valid     uint8 [slots][N]         1: the record is a transition
 *   env_state int32 [N][4]             per env: turn, episode, records of the episode, frozen (set by evg_dqn_replay_clear, advanced by record)
 *   scan      int32 [EVG_DQN_REPLAY_SCAN_INTS(slots, N)]   work space of sample / size
 *   ctl       uint64 [4]               {sample calls so far, status bits, records counted by the last scan, call index in use}
 *
 * A record is exactly ONE transition carrying seven actions; there is no n-step sum.  After record t the records t - H + 1 .. t are live: their own
 * slot and the next one still hold their two observations.
 *
 * Validity.  A record is a transition only if all seven rows have unit in 0..11 and node in 0..10 (the reference's gather(1, action) raises on
 * anything else); otherwise it is never drawn or gathered and EVG_DQN_REPLAY_S_BAD_ACTION is set, so that a caller's wild order rows cannot become an
 * out-of-range index of evg_dqn_td_head.
 *
 * Documented differences from the reference.  (1) The capacity is counted in turns of all envs.  (2) Draws are WITH replacement.  (3) With auto_reset
 * the slot behind a finishing step holds the next episode's first observation; the terminal observation is never written.  The record carries
 * not_done = 0 and the batch's next_state row is zeros for it.  Without auto_reset the slot does hold the terminal observation, and
 * EVG_DQN_REPLAY_TERMINAL_NEXT returns it unmasked (not_done is still reported); the flag is refused on an auto_reset handle. */
#define EVG_DQN_REPLAY_OBS_STRIDE(N, elem) (((int64_t)(N) * 105 * (elem) + 15) / 16 * 16)           /* bytes */
#define EVG_DQN_REPLAY_ACT_STRIDE(N) (((int64_t)(N) * 14 + 3) / 4 * 4)                              /* ints  */
#define EVG_DQN_REPLAY_SCAN_INTS(slots, N) (((int64_t)(slots) * (N) + 3) / 4 + ((int64_t)(slots) * (N) + 1023) / 1024)
#define EVG_DQN_REPLAY_MAX_BATCH (1 << 20)
/* grid caps: past them a workgroup strides over further tiles (gather: tiles of EVG_DQN_REPLAY_TILE transitions; draw: 256 draws) */
#define EVG_DQN_REPLAY_TILE 16
#define EVG_DQN_REPLAY_GATHER_MAX_BLOCKS 2048
#define EVG_DQN_REPLAY_DRAW_MAX_BLOCKS 256
/* status bits of ctl[1] (sticky until evg_dqn_replay_clear); the first two are EVG_REPLAY_S_EMPTY and EVG_REPLAY_S_BAD_HANDLE of evg.h, 4 is the
 * prioritized memory's bad priority */
#define EVG_DQN_REPLAY_S_BAD_ACTION 8
#define EVG_DQN_REPLAY_TERMINAL_NEXT 1     /* `flags` of sample / gather */

typedef struct evg_dqn_replay {
    uint32_t struct_size;          /* = sizeof(evg_dqn_replay)                                                               */
    int32_t slots;                 /* H + 1 >= 2                                                                             */
    int32_t seat;                  /* the learner's seat, 0 or 1 (the reward's player)                                       */
    int32_t shaping;               /* EVG_SHAPE_* of evg.h                                                                   */
    int32_t shaping_from, shaping_to;   /* EVG_SHAPE_TRANSITION: the two base functions                                      */
    int32_t transition_episodes;   /* EVG_SHAPE_TRANSITION: K >= 1                                                           */
    int32_t reserved;              /* 0                                                                                      */
    int64_t episode_base;          /* i_episode = episode_base + 1 + the env's episode index on the handle                   */
    void* obs;
    int32_t* actions;
    double* reward;
    int32_t* meta;
    uint8_t* valid;
    int32_t* env_state;
    int32_t* scan;
    unsigned long long* ctl;
} evg_dqn_replay;

/* Empties the memory (valid, meta, reward, ctl) and takes every env's counters from the handle's state as the stream reaches the call. */
EVG_API int evg_dqn_replay_clear(evg_handle* h, const evg_dqn_replay* m, void* stream);
/* One launch after step `turn` (0, 1, 2, ... since the last clear; the caller's counter, so that an unrolled loop can be captured).  Per env: the
 * turn's shaped reward in float64 (reward_in [N][2] f32, 8-byte aligned, and done_in [N] u8 of the step, or custom_in float [N] with
 * EVG_SHAPE_CUSTOM; the env's own turn and episode counters exactly as evg_replay_record uses them), the flag not_done, the valid byte; slot turn + 1's
 * record is emptied and the env's counters advance.  A frozen env (finished without auto_reset) records nothing. */
EVG_API int evg_dqn_replay_record(evg_handle* h, const evg_dqn_replay* m, int64_t turn, const float* reward_in, const uint8_t* done_in,
                                  const float* custom_in, void* stream);
/* The number of valid records, counted on the device into ctl[2]; no host read-back. */
EVG_API int evg_dqn_replay_size(evg_handle* h, const evg_dqn_replay* m, void* stream);
/* evg_dqn_td_head's batch (four launches: scan, top, draw, gather) for `batch` records drawn uniformly WITH replacement over the valid records: draw i
 * is word 0 of Philox((i, call index lo, hi, 5), seed), t = (word * total) >> 32, and names the t-th valid record in (slot, env) order -- the rule of
 * evg_replay_sample.  Outputs, row i (all 16-byte aligned):
 *   state       float [batch][105]   the record's observation: int16 converts exactly, float64 rounds to nearest even
 *   action      int64 [batch][7]     unit * 11 + node
 *   next_state  float [batch][105]   the next slot's observation; zeros where not_done = 0 (unless EVG_DQN_REPLAY_TERMINAL_NEXT)
 *   reward      float [batch]        the float64 shaped reward rounded once
 *   not_done    uint8 [batch]
 *   handles     int32 [batch][4]     {slot, env, 0, 0} (all -1 when the memory is empty)
 * An empty memory writes zeros and sets EVG_REPLAY_S_EMPTY in ctl[1].  The call index is ctl[0], advanced on the device. */
EVG_API int evg_dqn_replay_sample(evg_handle* h, const evg_dqn_replay* m, int batch, uint64_t seed, int flags, float* state, int64_t* action,
                                  float* next_state, float* reward, uint8_t* not_done, int32_t* handles, void* stream);
/* The same outputs for caller-chosen handles (one launch).  A handle that names no valid record gets zeros and sets EVG_REPLAY_S_BAD_HANDLE.
 *
 * The gather.  A source row starts at env * 105 * element size: 2-byte aligned for int16, 4-byte for float32.  It is read element by element, lane
 * by lane (a wavefront's load covers 64 consecutive elements), into an LDS tile of EVG_DQN_REPLAY_TILE transitions as float32; the tile -- 1 680
 * floats, a multiple of four -- leaves with 16-byte stores over the flat batch * 105 index space, a unit straddling two transitions like any other,
 * the last one element by element where batch * 105 is no multiple of 4.  Nothing is read past a slot's N-th row and nothing written past the batch.
 *
 * Refusals of these five (EVG_ERR_INVALID, nothing launched): NULL handle or descriptor, wrong struct_size, slots < 2, seat outside 0..1, an unknown
 * shaping, a NULL or misaligned (16 bytes) descriptor buffer; record: turn < 0, done_in or the reward operand NULL, reward_in not 8-byte aligned;
 * sample / gather: batch outside 1..EVG_DQN_REPLAY_MAX_BATCH, an unknown flag, a NULL or misaligned output or handle pointer, slots x N too large,
 * EVG_DQN_REPLAY_TERMINAL_NEXT on an auto_reset handle. */
EVG_API int evg_dqn_replay_gather(evg_handle* h, const evg_dqn_replay* m, int batch, const int32_t* handles, int flags, float* state, int64_t* action,
                                  float* next_state, float* reward, uint8_t* not_done, void* stream);

/* ---- sampling by priority (agents/DQN/PrioritizedMemory.py: sample / update_priorities over the same ring) -------------------------------------------
 * Three more caller-owned buffers next to the memory's:
 *
 *   weight  float  [slots][N]   priority ** alpha of the record, 0 = never updated
 *   stamp   int32  [slots][N]   the record the weight belongs to: its turn and episode in include/evg_replay_priority.h's encoding
 *                               (0x80000000 | (episode & 0x7FFFFF) << 8 | turn & 0xFF).  A stamp that is not the record's means "never updated", so
 *                               evg_dqn_replay_record knows nothing of these buffers and recording costs nothing more.
 *   pscan   uint64 [EVG_DQN_REPLAY_PSCAN_WORDS(slots, N)]   work space of the prioritized sample, 8-byte aligned
 *   pctl    uint64 [4]          {wmax as float bits, Q, the batch's least q, 0}
 *
 * The three documented rules of evg_replay_priority.h, unchanged: (1) a never-updated record weighs wmax -- the largest weight stored since the last
 * clear, 1 after it -- AS OF THE DRAW; (2) when one update names a record more than once the LARGEST priority is kept (two launches: reset, then a
 * maximum over the weights' bits -- no result depends on thread order, and an update with duplicate handles is idempotent); (3) draws use integer
 * weights q = max(1, floor(w * 2^(32 - e))) with frexp(wmax) = (m, e), probabilities q / Q, so that a host model reproduces every draw bit for bit and
 * nothing is undrawable.  Draw i takes u = (word 0 << 32) | word 1 of Philox((i, call index lo, hi, 7), seed) and the record that holds position
 * (u * Q) >> 64 in (slot, env) order.  weights_out[i] = (T q / Q) ** -beta in float64 over the batch's largest, rounded once; beta == 0 gives exactly
 * 1.0f.  A priority that is NaN, infinite or <= 0 is skipped and sets EVG_DQN_REPLAY_S_BAD_PRIORITY; a handle that names no valid record is skipped
 * and sets EVG_REPLAY_S_BAD_HANDLE.  The call index is the memory's ctl[0], shared with evg_dqn_replay_sample.
 *
 * Refusals, next to those above: a NULL priority descriptor, wrong struct_size, alpha outside [0, 1], a NULL buffer, weight or stamp not 16-byte or
 * pscan or pctl not 8-byte aligned; update: batch outside 1..EVG_DQN_REPLAY_MAX_BATCH, handles (16-byte aligned) or priorities NULL; sample: beta not
 * finite or < 0, weights_out NULL or not 16-byte aligned. */
#define EVG_DQN_REPLAY_PSCAN_WORDS(slots, N) (((int64_t)(slots) * (N) + 3) / 4 + 2 * (((int64_t)(slots) * (N) + 1023) / 1024))
#define EVG_DQN_REPLAY_S_BAD_PRIORITY 4

typedef struct evg_dqn_replay_priority {
    uint32_t struct_size;          /* = sizeof(evg_dqn_replay_priority) */
    float alpha;                   /* prob_alpha, in [0, 1]            */
    float* weight;
    int32_t* stamp;
    unsigned long long* pscan;
    unsigned long long* pctl;
} evg_dqn_replay_priority;

/* weights and stamps to "never updated", wmax = 1; call it behind evg_dqn_replay_clear */
EVG_API int evg_dqn_replay_priority_clear(evg_handle* h, const evg_dqn_replay* m, const evg_dqn_replay_priority* p, void* stream);
EVG_API int evg_dqn_replay_update_priorities(evg_handle* h, const evg_dqn_replay* m, const evg_dqn_replay_priority* p, int batch, const int32_t* handles,
                                             const float* priorities, void* stream);
/* evg_dqn_replay_sample's outputs for records drawn by weight, with replacement (five launches: scan, top, draw, weights, gather), and weights_out
 * float [batch] */
EVG_API int evg_dqn_replay_sample_prioritized(evg_handle* h, const evg_dqn_replay* m, const evg_dqn_replay_priority* p, int batch, uint64_t seed,
                                              int flags, float beta, float* state, int64_t* action, float* next_state, float* reward,
                                              uint8_t* not_done, int32_t* handles, float* weights_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
