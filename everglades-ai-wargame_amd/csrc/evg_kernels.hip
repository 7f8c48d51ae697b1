// evg_kernels.hip -- hand-written HIP kernels for gfx950 (MI355X / CDNA4).
//
// One fused kernel per env-step replaces EvergladesEnv.step -> EvergladesGame.game_turn ->
// board_state/player_state of the reference (everglades_env.py:32-73, server.py:211-501).
//
// Mapping: lane = (env slot, player); one wavefront = 32 envs per workgroup.
// The game rules are short, branchy integer programs with almost no parallelism inside one env
// (7 orders per player, ~1 contested node per turn), so envs are spread over LANES: one instruction
// serves 32 envs, where a wave-per-env mapping would leave most lanes idle.  Two lanes per env halve
// every per-player loop and give 2 waves per SIMD at 65 536 envs (latency hiding); the pair exchanges
// values with one DPP move.  Everything a lane indexes dynamically (its 12 group words, the node
// words, per-node accumulators) lives in LDS as [index][lane] columns: lane-private and
// bank-conflict-free by construction (bank = lane mod 32).  Combat is rebalanced over the whole wave:
// a prefix scan over lanes builds one work item per fighting group, damage accumulates in a shared
// LDS pool with integer LDS atomics (order-free, deterministic).  The SoA state arrays are
// env-fastest (coalesced); the wave's observation block (32 x 840 B, contiguous in the output) is
// assembled in LDS in output order and streamed out with 16-byte-per-lane coalesced stores.
// Uniform map/unit tables sit in SGPRs as nibble-packed words, per-lane-indexed ones in LDS.
// No MFMA: there is no dense contraction anywhere on this path.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "evg_device.h"
#include "evg_rng.h"
#include "evg_mt.h"

namespace evg {

// Diagnostics are compiled only into the separate libraries libevg_diag.so (-DEVG_DIAG: phase ablation, the 16-envs-per-wave
// variant, a switch that forces the IEEE-division branch) and libevg_stamps.so (-DEVG_DIAG -DEVG_STAMPS: lane 0 of every
// wave stores s_memtime at phase boundaries into a debug buffer of its own).  The product library libevg.so contains
// none of it: no ablation branch, no stamp, no environment variable.
#ifdef EVG_DIAG
#define ABLATED(bit) ((io.ablate & (bit)) != 0u)
#else
#define ABLATED(bit) false
#endif
#ifdef EVG_STAMPS
#define STAMP(i)                                                                        \
    do {                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                              \
        const unsigned long long t_ = clock64();                                        \
        __builtin_amdgcn_sched_barrier(0);                                              \
        if (lane == 0 && io.stamps) io.stamps[(size_t)blockIdx.x * 16 + (i)] = t_;      \
    } while (0)
// whole-launch stamps of the wave: s_memrealtime (constant 100 MHz) at its start and end plus where it ran (HW_ID, XCC_ID)
#define STAMP_WAVE_BEGIN() const unsigned long long wave_t0_ = __builtin_amdgcn_s_memrealtime()
#define STAMP_WAVE_END()                                                                                                   \
    do {                                                                                                                   \
        const unsigned long long t1_ = __builtin_amdgcn_s_memrealtime();                                                   \
        if (threadIdx.x == 0 && A->io_.stamps) {                                                                            \
            A->io_.stamps[(size_t)blockIdx.x * 16 + 14] = (wave_t0_ & 0xFFFFFFFFull) | ((unsigned long long)__builtin_amdgcn_s_getreg(63492) << 32); \
            A->io_.stamps[(size_t)blockIdx.x * 16 + 15] = (t1_ & 0xFFFFFFFFull) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);      \
        }                                                                                                                  \
    } while (0)
#else
#define STAMP(i)
#define STAMP_WAVE_BEGIN()
#define STAMP_WAVE_END()
#endif

// Phase markers (stamps build only).
#define PHASE(i) STAMP(i)

#include "step_common.inc"      // LDS layout of a wavefront's envs, phase fence, sorting network, small device helpers
#include "step_rules.inc"       // the rules of a turn, written once for both lane mappings (pure register functions)
#include "step_agents.inc"      // the scripted opponents (one device function over a view)
#include "league_choice.inc"    // the opponent league's member draw and object swap (the step kernel's league forms and league_kernels.inc)
#include "smart_decode.inc"     // the Smart_State agent's decode of its Q values (the standalone kernel and the step kernel's Q form)
#include "minimized_decode.inc" // the Minimized agents' decode of their 11-way Q values (the standalone kernel and the step kernel's 11-way Q forms)
#include "step_kernel.inc"      // evg_step_kernel: skeleton + the phases of a turn (step_orders / step_combat / step_move_capture / step_outputs .inc)

#include "evg_step4.inc"        // the four-lanes-per-env mapping: what persistent launches of SMALL batches run (launch_step)

#undef S
#undef io

#include "side_kernels.inc"     // pack, chunk-queue check, reset, seeding, action generators, fog planes, Smart_State features
#include "replay_kernels.inc"   // the Smart_State learner's n-step replay memory: record, count, draw, gather
#ifdef EVG_PRIORITY              // `make priority` (libevg_priority.so): the product's kernels plus ...
#include "replay_priority_kernels.inc"   // prioritized sampling over that memory: the weight plane's update pair, the q scan, draw and importance weights
#endif
#include "qnet_kernels.inc"     // the Smart_State Q network's forward pass (inference) on v_mfma_f32_16x16x4_f32
#include "league_kernels.inc"   // the opponent league: clear, assign after an explicit reset, importance weights
#include "minimized_qnet.inc"   // the Minimized agents' Q network's forward pass (59 -> h1 <= 128 -> 11) on v_mfma_f32_16x16x4_f32
#include "population_kernels.inc"   // self-royale: per-env members drawn from a population, the bucket pass and the grouped Minimized forward
#ifdef EVG_BF16                  // `make bf16` (libevg_bf16.so): the product's kernels plus ...
#include "qnet_bf16_kernels.inc"    // the two Q networks' reduced-precision forward on v_mfma_f32_16x16x32_bf16 (acting, target network)
#endif
#ifdef EVG_POP_BF16              // `make popbf16` (libevg_popbf16.so, with EVG_BF16): ... plus ...
#include "population_bf16_kernels.inc"   // self-royale: the grouped forward of both populations on the bf16 matrix cores
#endif
#ifdef EVG_GRAD                  // `make grad` (libevg_grad.so): the product's kernels plus ...
#include "qnet_grad_kernels.inc"    // the backward pass of the two Q networks' expanded fp32 forward (optimize_model's policy forward)
#endif
#ifdef EVG_LEARN                 // `make learn` (libevg_learn.so, with EVG_GRAD): ... plus ...
#include "learn_kernels.inc"        // the learner step's glue: the TD head (target, Huber loss, dLoss/dQ) and Adam over a network's tensors
#endif
#ifdef EVG_POP_LEARN             // `make poplearn` (libevg_poplearn.so, with EVG_GRAD and EVG_LEARN): ... plus ...
#include "pop_learn_kernels.inc"    // self-royale: the grouped TD head, backward and Adam that train every member of a team from one batch
#endif
#ifdef EVG_DQN                   // `make dqn` (libevg_dqn.so): the product's kernels plus ...
#include "dqn_decode.inc"           // the agents/DQN family's decode of its 132-way head (filter_actions) and its exploring draws
#include "dqn_kernels.inc"          // ... and its 105 -> h1 <= 528 -> 132 network, the hidden layer streamed in chunks, on v_mfma_f32_16x16x4_f32
#endif
#ifdef EVG_DQN_GRAD              // `make dqngrad` (libevg_dqngrad.so, with EVG_DQN): ... plus ...
#include "dqn_grad_kernels.inc"     // that network's backward pass: the row-parallel delta kernel and the tile-parallel weight-gradient GEMMs
#endif
#ifdef EVG_DQN_LEARN             // `make dqnlearn` (libevg_dqnlearn.so, with EVG_DQN and EVG_DQN_GRAD): ... plus ...
#include "dqn_learn_kernels.inc"    // the rest of that family's optimize_model: the top-7 TD head and Adam over a large network launched over a grid
#endif
#ifdef EVG_DQN_REPLAY            // `make dqnreplay` (libevg_dqnreplay.so, with EVG_DQN, EVG_DQN_GRAD and EVG_DQN_LEARN): ... plus ...
#include "dqn_replay_kernels.inc"   // that family's replay memory of raw observations: record, count, draw and the gather of optimize_model's batch
#endif

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// obs_dtype (EVG_OBS_*) -> the observation's element type: f is called with a value of that type as a tag (a generic lambda takes it as `auto ot` and
// names the type decltype(ot)) and its result is returned; -1 for a dtype that does not exist.  The one switch over the observation types in this file.
template <typename F>
static int with_obs_type(int obs_dtype, F&& f) {
    switch (obs_dtype) {
        case EVG_OBS_F32: return f(float{});
        case EVG_OBS_F64: return f(double{});
        case EVG_OBS_I16: return f(int16_t{});
        default: return -1;
    }
}

// The forms of evg_step_kernel that are launched, by name: what each one sets of the kernel's template parameters (step_kernel.inc; its static_asserts
// guard the combinations).
struct SingleTurn {                                  // one turn per launch, 32 envs per wavefront, orders read or drawn for both seats
    static constexpr int lanes = WG;                 // LPW: lanes of a wavefront that hold envs, two per env
    static constexpr bool multi = false;             // MULTI: the persistent form, io.turns consecutive turns per launch
    static constexpr bool stock_mt = false;          // MT: the stock-entropy mode's sequential MT19937 draws
    static constexpr bool chunked = false;           // CHUNKED: workgroups take (set, chunk of turns) units from their XCD's queue
    static constexpr bool seat = false;              // SEAT: the caller plays one seat, a scripted policy the other; obs is [N][105]
    static constexpr int waves_per_block = 1;        // WPB: independent wavefronts per workgroup
    static constexpr bool qdec = false;              // QDEC: orders decoded in the launch from the Q values io.q
    static constexpr bool league = false;            // LEAGUE: the scripted policy of the other seat is a per-env member of an opponent league (io.lg_*)
    static constexpr int head = HEAD_SMART;          // HEAD: the agent family whose network output a Q form decodes (HEAD_MINIMIZED: evg_step_minimized_kernel)
};
struct Persistent : SingleTurn { static constexpr bool multi = true; };
struct Chunked : Persistent { static constexpr bool chunked = true; };
struct StockEntropy : SingleTurn { static constexpr bool stock_mt = true; };
struct Seat : SingleTurn { static constexpr bool seat = true; };
struct SeatQ : Seat { static constexpr bool qdec = true; };
struct TwoSeatQ : SingleTurn { static constexpr bool qdec = true; };
struct SeatLeague : Seat { static constexpr bool league = true; };
struct SeatQLeague : SeatQ { static constexpr bool league = true; };
struct SeatQMin : SeatQ { static constexpr int head = HEAD_MINIMIZED; };
struct SeatQMinLeague : SeatQMin { static constexpr bool league = true; };
struct TwoSeatQMin : TwoSeatQ { static constexpr int head = HEAD_MINIMIZED; };
struct TwoSeatQMinLeague : TwoSeatQMin { static constexpr bool league = true; };
#ifdef EVG_DIAG
// diagnostic library, lanes = 32: 16 envs per wavefront + 32 helper lanes, in both launch forms
template <typename Form> struct HelperLanes : Form { static constexpr int lanes = WG / 2; };
struct Wg256 : SingleTurn { static constexpr int waves_per_block = 4; };
#endif
// (OT, form) -> the kernel, e.g. SeatQ with float32 observations: evg_step_kernel<float, 64, false, false, false, true, 1, true, false>
// (the 11-way head: evg_step_minimized_kernel<OT, LEAGUE>, two seats evg_step_minimized2_kernel<OT, LEAGUE>: kernels of their own names -- step_kernel.inc)
template <typename OT, typename Form>
constexpr auto step_kernel_of_head() {
    if constexpr (Form::head == HEAD_MINIMIZED && !Form::seat) return evg_step_minimized2_kernel<OT, Form::league>;
    else if constexpr (Form::head == HEAD_MINIMIZED) return evg_step_minimized_kernel<OT, Form::league>;
    else return evg_step_kernel<OT, Form::lanes, Form::multi, Form::stock_mt, Form::chunked, Form::seat, Form::waves_per_block, Form::qdec, Form::league>;
}
template <typename OT, typename Form>
constexpr auto step_kernel_of = step_kernel_of_head<OT, Form>();

// One launch of a step-kernel form over envs [io.env_lo, io.env_hi): a wavefront per set of envs -- the chunked form: as many workgroups as the device holds
// (io.grid_slots), each taking units from its XCD's queue
template <typename Form>
static int launch_form(const DevState& S, const StepIO& io, int obs_dtype, hipStream_t s) {
    constexpr int epw = Form::lanes / 2;
    const int waves = Form::chunked ? io.grid_slots : (io.env_hi - io.env_lo + epw - 1) / epw;
    const dim3 grid((unsigned)((waves + Form::waves_per_block - 1) / Form::waves_per_block)), block(WG * Form::waves_per_block);
    return with_obs_type(obs_dtype, [&](auto ot) {
        const StepArgs args{S, io};
        hipLaunchKernelGGL((step_kernel_of<decltype(ot), Form>), grid, block, 0, s, args);
        return (int)hipGetLastError();
    });
}

#ifdef EVG_DIAG
// round-5 experiment (diagnostic library, lanes = 256): the single-turn form with FOUR independent wavefronts per 256-thread workgroup
static int launch_step_wg256(const DevState& S, const StepIO& io, int obs_dtype, hipStream_t s) { return launch_form<Wg256>(S, io, obs_dtype, s); }
#endif

// the chunked form of the persistent two-lane kernel: as many workgroups as the device holds, each taking units from its XCD's queue
// (this and the one above are functions of their own, defined ahead of everything else that names a kernel, so that the compiler emits the kernels in the
// order it always did: the device assembly of two builds can then be compared as whole files)
static int launch_step_chunked(const DevState& S, const StepIO& io, int obs_dtype, hipStream_t s) { return launch_form<Chunked>(S, io, obs_dtype, s); }

// Persistent launches of small and medium batches: the four-lanes-per-env mapping of evg_step4.inc -- 16 envs per wavefront,
// twice the wavefronts, 2 213 instead of 3 164 vector instructions per wave-turn.  While a SIMD holds few wavefronts, what counts is
// how long ONE wavefront needs for a turn, not the total instruction count.  Persistent form, us per turn on a whole MI355X,
// two-lane / four-lane (A/B of two builds on one box): 8 192 envs 11.0 / 8.3, 16 384 envs 11.8 / 8.3, 24 576 envs 12.1 / 9.6,
// 32 768 envs 12.1 / 10.4 (2 048 four-lane wavefronts = two per SIMD, the 160-VGPR build at 2 waves per SIMD); 40 960 envs
// 14.0 / 12.9, 49 152 envs 14.5 / 13.7 (up to 3 072 wavefronts = three per SIMD: the same kernel built for three, still
// unspilled).  Beyond that the four-lane grid is no longer resident at once (4 waves per SIMD need <= 128 VGPRs: 28 spilled) and
// the two-lane kernel wins.  Same state in HBM, same results (the persistent form of every small-batch test runs this kernel and
// is compared with the two-lane single-turn form and with the oracle).  The two thresholds are what the DEVICE holds
// (DeviceCaps::slots4_w2 / slots4_w3 wavefronts of 16 envs), not literals.
template <bool MULTI, int WPE>
static int launch_step4(const DevState& S, const StepIO& io, int obs_dtype, hipStream_t s) {
    const dim3 grid((io.env_hi - io.env_lo + 15) / 16), block(WG);
    return with_obs_type(obs_dtype, [&](auto ot) {
        const StepArgs args{S, io};
        hipLaunchKernelGGL((evg_step4_kernel<decltype(ot), MULTI, WPE>), grid, block, 0, s, args);
        return (int)hipGetLastError();
    });
}

// What the device holds at once: compute units from hipDeviceProp_t, resident workgroups per CU from the occupancy of the kernels
// themselves.  On a whole MI355X: 256 CUs, 8 two-lane workgroups per CU (LDS: 8 x 20 208 B of 160 KiB; 2 waves per SIMD) = 2 048
// wavefronts = 65 536 envs; four-lane kernel 2 / 3 waves per SIMD = 2 048 / 3 072 wavefronts = 32 768 / 49 152 envs.
template <typename OT>
static int query_caps_t(DeviceCaps* c) {
    int b2m = 0, b2s = 0, b4w2 = 0, b4w3 = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b2m, (const void*)step_kernel_of<OT, Persistent>, WG, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b2s, (const void*)step_kernel_of<OT, SingleTurn>, WG, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b4w2, (const void*)evg_step4_kernel<OT, true, 2>, WG, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b4w3, (const void*)evg_step4_kernel<OT, true, 3>, WG, 0);
    if (e != hipSuccess) return (int)e;
    const int b2 = b2m < b2s ? b2m : b2s;
    if (b2 < 1 || b4w2 < 1 || b4w3 < 1) return (int)hipErrorLaunchOutOfResources;
    c->slots2 = c->cus * b2;
    // the four-lane builds aim at 2 / 3 waves per SIMD (amdgpu_waves_per_eu); the hardware may hold more of them, the plan does not use that
    c->slots4_w2 = c->cus * (b4w2 < 8 ? b4w2 : 8);
    c->slots4_w3 = c->cus * (b4w3 < 12 ? b4w3 : 12);
    return 0;
}

int query_device_caps(int device_id, int obs_dtype, DeviceCaps* caps) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return (int)e;
    caps->cus = prop.multiProcessorCount;
    caps->simds = 4 * caps->cus;
    // MI355X: 256 MiB of Infinity Cache behind 256 CUs; a partition gets its share (evg_config::cache_mib overrides)
    caps->cache_bytes = (256ll << 20) * caps->cus / 256;
    return with_obs_type(obs_dtype, [&](auto ot) { return query_caps_t<decltype(ot)>(caps); });
}

// Which kernel plays which envs.  Single-turn launches (evg_step) and the stock-entropy mode: one launch of the two-lane kernel.
// Persistent form: a batch up to what the device holds at once runs the four-lane kernel while its grid is resident at two or
// three waves per SIMD and the two-lane kernel above that (the thresholds are DeviceCaps, not literals).  A LARGER batch used to be
// one launch of ceil(N / 32) workgroups, each playing all its turns: whole rounds of resident workgroups one after the other -- which
// is good, every round's working set (171 MB at 65 536 envs) stays inside the 256 MB Infinity Cache -- but the REMAINDER behind the
// last whole round ran alone at low occupancy for a whole launch (98 304 envs: 30.9 us per turn where 1.5 x 17.0 = 25.5 would be
// proportional; 65 536 + 4 480 envs cost 28.0 instead of 18.0).  Now:
//   * the whole rounds but the last: one plain launch, as before;
//   * the last whole round TOGETHER WITH the remainder, while the two fit the Infinity Cache (kChunkFootprintMax): one CHUNKED launch -- as many
//     workgroups as the device holds, each taking units (set of 32 envs) x (chunk of kChunkTurns turns) from its XCD's queue and handing
//     the set on through HBM (see the kernel's prologue): all slots stay busy until the queues run dry (98 304 envs: 26 us per turn,
//     70 016: 18.0);
//   * a larger remainder: its own plain launch behind the whole rounds (four-lane kernel up to 49 152 envs).  Chunking it too would
//     cycle the launch through nearly two rounds' worth of envs, more than the Infinity Cache holds, and every turn then runs ~30 %
//     slower (measured: 131 104 envs chunked 46 us per turn, plain 44; 262 144 chunked 90, plain 67).
#ifndef EVG_CHUNK_TURNS
// turns per chunk of a chunked launch (a build-time knob so that it can be re-measured with two builds: tools/scaling_lib.py)
#define EVG_CHUNK_TURNS 25
#endif
[[maybe_unused]] constexpr int kChunkTurns = EVG_CHUNK_TURNS;
// A chunked launch cycles through ALL its envs every few chunks, so its working set -- state, and what THIS rollout writes: observations,
// orders, results; 2.74 KB per env with float32 observations -- must fit the device's share of the Infinity Cache (DeviceCaps::cache_bytes:
// 256 MiB on a whole MI355X, + 2 %): measured, us per turn, chunked / the alternative: 98 304 envs (270 MB) 25.8 / 27.5; 104 448 envs
// (287 MB) 32.5 / ~29.5.
long long rollout_bytes_per_env(const StepIO& io, int obs_dtype) {
    long long b = kStateBytesPerEnv + 13 /* fin_ret, fin_len, fin_win */ + 19 /* reward, done, winner, scores, status */ + 8 /* hand-over checksums */;
    if (io.obs) b += OBS2 * (obs_dtype == EVG_OBS_F64 ? 8 : (obs_dtype == EVG_OBS_I16 ? 2 : 4));
    if (io.actions_out) b += 2 * NA * 2 * 4;
    if (io.gen_actions == 2) b += 24;                    // the scripted agents' objects
    return b;
}
LaunchPlan plan_step(const DevState& S, const StepIO& io, int obs_dtype, const DeviceCaps& caps) {
    LaunchPlan p;
    p.n = 1;
    p.piece[0] = LaunchPiece{0, 0, S.N, 0};
    p.piece[1] = LaunchPiece{0, 0, 0, 0};
    const bool multi = io.turns > 1;
    if (S.mt_key || !multi) return p;
    [[maybe_unused]] const long long cap2 = 32ll * caps.slots2, cap4_2 = 16ll * caps.slots4_w2, cap4_3 = 16ll * caps.slots4_w3;
    [[maybe_unused]] const long long N = S.N;
#ifdef EVG_DIAG
    // experiment: the chunked form over the WHOLE batch, whatever its size (a working set beyond the Infinity Cache)
    if (io.lanes_per_wave == 2) {
        if (N > cap2 && io.turns > kChunkTurns) p.piece[0].chunk_turns = kChunkTurns;
        return p;
    }
    if (io.lanes_per_wave != 0) return p;          // a forced kernel variant plays the whole batch in one plain launch
#endif
#ifdef EVG_STAMPS
    return p;                                       // the stamp buffer is indexed by workgroup: one plain launch
#else
    if (N <= cap4_2) { p.piece[0].four_lane_wpe = 2; return p; }
    if (N <= cap4_3) { p.piece[0].four_lane_wpe = 3; return p; }
    if (N <= cap2) return p;
    const long long full = N / cap2, rem = N - full * cap2;
    if (rem == 0) return p;                         // whole rounds only: one plain launch
    if ((cap2 + rem) * rollout_bytes_per_env(io, obs_dtype) <= caps.cache_bytes + caps.cache_bytes / 50 && io.turns > kChunkTurns) {
        p.n = 0;
        if (full >= 2) p.piece[p.n++] = LaunchPiece{0, 0, (int32_t)((full - 1) * cap2), 0};
        p.piece[p.n++] = LaunchPiece{0, (int32_t)((full - 1) * cap2), (int32_t)N, kChunkTurns};
        return p;
    }
    p.n = 2;
    p.piece[0] = LaunchPiece{0, 0, (int32_t)(full * cap2), 0};
    p.piece[1] = LaunchPiece{rem <= cap4_2 ? 2 : (rem <= cap4_3 ? 3 : 0), (int32_t)(full * cap2), (int32_t)N, 0};
    return p;
#endif
}

// The caller's StepIO with the launcher-owned fields set for one plain launch over the whole handle ...
static StepIO whole_handle_io(const DevState& S, const StepIO& io_in) {
    StepIO io = io_in;
    io.env_lo = 0; io.env_hi = S.N; io.flags = 0; io.nsets = 0; io.chunk_turns = 0; io.progress_base = 0; io.grid_slots = 0;
    return io;
}
// ... and that of a single-turn launch: a grid that is resident at once staggers its wavefronts
static StepIO single_turn_io(const DevState& S, const StepIO& io_in, const DeviceCaps& caps) {
    StepIO io = whole_handle_io(S, io_in);
    io.turns = 1;
    if ((S.N + WG / 2 - 1) / (WG / 2) <= caps.slots2) io.flags |= STEP_F_STAGGER;
    return io;
}

int launch_step(const DevState& S, const StepIO& io_in, int obs_dtype, const DeviceCaps& caps, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool multi = io_in.turns > 1;
    StepIO io = multi ? whole_handle_io(S, io_in) : single_turn_io(S, io_in, caps);
    if (S.mt_key) {                       // stock-entropy mode: single-turn launches of the sequential-draw instantiation
        if (multi) return -1;
        return launch_form<StockEntropy>(S, io, obs_dtype, s);
    }
#ifdef EVG_DIAG
    // the two-lane kernel at any size
    if (io.lanes_per_wave == 64) return multi ? launch_form<Persistent>(S, io, obs_dtype, s) : launch_form<SingleTurn>(S, io, obs_dtype, s);
    if (io.lanes_per_wave == 256) return multi ? launch_form<Persistent>(S, io, obs_dtype, s) : launch_step_wg256(S, io, obs_dtype, s);
    if (io.lanes_per_wave == 4) return multi ? launch_step4<true, 4>(S, io, obs_dtype, s) : launch_step4<false, 4>(S, io, obs_dtype, s);
    if (io.lanes_per_wave == 32)
        return multi ? launch_form<HelperLanes<Persistent>>(S, io, obs_dtype, s) : launch_form<HelperLanes<SingleTurn>>(S, io, obs_dtype, s);
#endif
    if (!multi) return launch_form<SingleTurn>(S, io, obs_dtype, s);
    const LaunchPlan plan = plan_step(S, io, obs_dtype, caps);
    for (int i = 0; i < plan.n; ++i) {
        const LaunchPiece& pc = plan.piece[i];
        io.env_lo = pc.env_lo; io.env_hi = pc.env_hi;
        io.flags = (pc.four_lane_wpe && (pc.env_hi - pc.env_lo + 15) / 16 > caps.simds) ? STEP_F_SHARED_SIMD : 0;
        io.nsets = 0; io.chunk_turns = 0;
        if (pc.chunk_turns > 0) {
            io.nsets = (pc.env_hi - pc.env_lo + WG / 2 - 1) / (WG / 2);
            io.chunk_turns = pc.chunk_turns;
            io.progress_base = 0;
            io.grid_slots = io.nsets < caps.slots2 ? io.nsets : caps.slots2;
            // every XCD's queue starts at unit 0 and every set's progress flag at "no chunk finished": ONE memset on the stream (the two arrays are one
            // allocation, queue first).  Nothing of a chunked launch lives on the host, so a captured launch can be replayed (hipGraph).
            const hipError_t me = hipMemsetAsync(S.queue, 0, (1024 + ((size_t)S.N + 31) / 32 + 1) * sizeof(uint32_t), s);
            if (me != hipSuccess) return (int)me;
        }
        int rc;
        if (pc.four_lane_wpe == 2) rc = launch_step4<true, 2>(S, io, obs_dtype, s);
        else if (pc.four_lane_wpe == 3) rc = launch_step4<true, 3>(S, io, obs_dtype, s);
        else if (io.nsets > 0) rc = launch_step_chunked(S, io, obs_dtype, s);
        else rc = launch_form<Persistent>(S, io, obs_dtype, s);
        if (rc) return rc;
        if (io.nsets > 0) {
            // ... and behind it, on the same stream: every XCD's queue handed out all its units (sets x chunks), or the handle is flagged
            ChunkUnits want;
            const uint32_t nchunks = (uint32_t)((io.turns + io.chunk_turns - 1) / io.chunk_turns);
            for (int x = 0; x < 16; ++x) want.per_xcd[x] = x < S.nxcd ? (uint32_t)((io.nsets - x + S.nxcd - 1) / S.nxcd) * nchunks : 0u;
            hipLaunchKernelGGL(evg_chunk_verify_kernel, dim3(1), dim3(WG), 0, s, S, want);
            rc = (int)hipGetLastError();
            if (rc) return rc;
        }
    }
    return 0;
}

// evg_step_smart_q (self-play): one launch of the two-seat Q form of the single-turn two-lane kernel -- both seats' rows decoded from io.q in the launch
int launch_step_smart_q(const DevState& S, const StepIO& io, int obs_dtype, const DeviceCaps& caps, void* stream) {
    if (S.mt_key || !io.q) return -1;
    return launch_form<TwoSeatQ>(S, single_turn_io(S, io, caps), obs_dtype, reinterpret_cast<hipStream_t>(stream));
}

// evg_step_vs_policy(_smart / _smart_q) / evg_observe_seat: one launch of the one-seat instantiation of the single-turn two-lane kernel (io.q: its Q form,
// evg_step_vs_policy_smart_q: an instantiation of its own)
int launch_step_seat(const DevState& S, const StepIO& io_in, int obs_dtype, const DeviceCaps& caps, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (S.mt_key) return -1;
    const StepIO io = single_turn_io(S, io_in, caps);
    return io.q ? launch_form<SeatQ>(S, io, obs_dtype, s) : launch_form<Seat>(S, io, obs_dtype, s);
}

// evg_step_vs_league(_q): the league forms of the one-seat kernel (io.q: with the Q decode)
int launch_step_league(const DevState& S, const StepIO& io_in, int obs_dtype, const DeviceCaps& caps, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (S.mt_key || !io_in.lg_assign) return -1;
    const StepIO io = single_turn_io(S, io_in, caps);
    return io.q ? launch_form<SeatQLeague>(S, io, obs_dtype, s) : launch_form<SeatLeague>(S, io, obs_dtype, s);
}

// which XCC ids does this device have?  (evg_create: 1 024 one-wave workgroups report where they ran)
__global__ void __launch_bounds__(WG) evg_xcd_probe_kernel(uint32_t* out) {
    if (threadIdx.x == 0) out[blockIdx.x] = __builtin_amdgcn_s_getreg(63508) & 15u;      // HW_REG_XCC_ID
}
int launch_xcd_probe(uint32_t* out, void* stream) {
    hipLaunchKernelGGL(evg_xcd_probe_kernel, dim3(1024), dim3(WG), 0, reinterpret_cast<hipStream_t>(stream), out);
    return (int)hipGetLastError();
}

int launch_reset(const DevState& S, const uint8_t* mask, void* obs, int obs_dtype, void* stream) {
    const dim3 grid((S.N + WG - 1) / WG), block(WG);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return with_obs_type(obs_dtype, [&](auto ot) {
        hipLaunchKernelGGL(evg_reset_kernel<decltype(ot)>, grid, block, 0, s, S, mask, obs);
        return (int)hipGetLastError();
    });
}

int launch_scripted_actions(const DevState& S, int policy, int player, const void* obs, int32_t* actions, int obs_dtype, void* stream) {
    const dim3 grid((S.N + 255) / 256), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return with_obs_type(obs_dtype, [&](auto ot) {
        using OT = decltype(ot);
        hipLaunchKernelGGL(evg_scripted_actions_kernel<OT>, grid, block, 0, s, S, policy, player, (const OT*)obs, actions);
        return (int)hipGetLastError();
    });
}

int launch_mt_seed(const DevState& S, const uint32_t* seeds_dev, void* stream) {
    hipLaunchKernelGGL(evg_mt_seed_kernel, dim3((S.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), S, seeds_dev);
    return (int)hipGetLastError();
}

int launch_scripted_reset(const DevState& S, void* stream) {
    hipLaunchKernelGGL(evg_scripted_reset_kernel, dim3((2 * S.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), S);
    return (int)hipGetLastError();
}

// out_swarm non-NULL: compact form, out = shared [N][34]
int launch_smart_state(const DevState& S, int player, const void* obs, int seat_only, float* out, float* out_swarm, int obs_dtype, void* stream) {
    const int blocks = (S.N + 3) / 4;                       // one wavefront per env and pass; 8 blocks per CU resident, further envs in passes
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    const dim3 block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return with_obs_type(obs_dtype, [&](auto ot) {
        using OT = decltype(ot);
        if (out_swarm) hipLaunchKernelGGL((evg_smart_state_kernel<OT, true>), grid, block, 0, s, S.N, player, seat_only, (const OT*)obs, out, out_swarm);
        else hipLaunchKernelGGL((evg_smart_state_kernel<OT, false>), grid, block, 0, s, S.N, player, seat_only, (const OT*)obs, out, out_swarm);
        return (int)hipGetLastError();
    });
}

// network output -> orders: one DPP row (16 lanes) per env
int launch_smart_actions(const DevState& S, int player, const void* obs, int seat_only, const float* q, int32_t* actions, int32_t* directions, int obs_dtype,
                         void* stream, const SmartExplore* ex) {
    // (the exploring form draws per env in the first wavefront of 1 024-thread workgroups = 64 envs: side_kernels.inc)
    const unsigned threads = ex ? 1024u : 256u;
    const dim3 grid((unsigned)(((size_t)S.N * 16 + threads - 1) / threads)), block(threads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int2* a = reinterpret_cast<int2*>(actions);
    int2* d = reinterpret_cast<int2*>(directions);
    ExploreArgs X{};
    if (ex) X = ExploreArgs{S.seed_lo, S.seed_hi, S.env_id_base, S.episode, ex->seat, ex->eps, ex->eps_env, ex->explored};
    return with_obs_type(obs_dtype, [&](auto ot) {
        using OT = decltype(ot);
        if (ex) hipLaunchKernelGGL((evg_smart_actions_kernel<OT, true>), grid, block, 0, s, S.N, player, seat_only, (const OT*)obs, q, a, d, X);
        else hipLaunchKernelGGL((evg_smart_actions_kernel<OT, false>), grid, block, 0, s, S.N, player, seat_only, (const OT*)obs, q, a, d, X);
        return (int)hipGetLastError();
    });
}

// evg_step_vs_policy_minimized_q / evg_step_vs_league_minimized_q: the one-seat Q form with the 11-way head (io.lg_assign: its league form)
int launch_step_minimized(const DevState& S, const StepIO& io_in, int obs_dtype, const DeviceCaps& caps, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (S.mt_key || !io_in.q) return -1;
    const StepIO io = single_turn_io(S, io_in, caps);
    return io.lg_assign ? launch_form<SeatQMinLeague>(S, io, obs_dtype, s) : launch_form<SeatQMin>(S, io, obs_dtype, s);
}

// evg_step_minimized_q / evg_step_league_minimized_q: the two-seat Q form with the 11-way head (io.lg_assign: its league form)
int launch_step_minimized2(const DevState& S, const StepIO& io_in, int obs_dtype, const DeviceCaps& caps, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (S.mt_key || !io_in.q) return -1;
    const StepIO io = single_turn_io(S, io_in, caps);
    return io.lg_assign ? launch_form<TwoSeatQMinLeague>(S, io, obs_dtype, s) : launch_form<TwoSeatQMin>(S, io, obs_dtype, s);
}

// the Minimized agents' network output -> orders: one DPP row (16 lanes) per env; ex NULL: get_best_actions only
int launch_minimized_actions(const DevState& S, const float* q, int32_t* actions, void* stream, const SmartExplore* ex, uint8_t* explored) {
    const unsigned threads = ex ? 1024u : 256u;
    const dim3 grid((unsigned)(((size_t)S.N * 16 + threads - 1) / threads)), block(threads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int2* a = reinterpret_cast<int2*>(actions);
    ExploreArgs X{};
    X.explored = explored;
    if (ex) {
        X = ExploreArgs{S.seed_lo, S.seed_hi, S.env_id_base, S.episode, ex->seat, ex->eps, ex->eps_env, explored};
        hipLaunchKernelGGL(evg_minimized_actions_kernel<true>, grid, block, 0, s, S.N, S.env, q, a, X);
    } else {
        hipLaunchKernelGGL(evg_minimized_actions_kernel<false>, grid, block, 0, s, S.N, S.env, q, a, X);
    }
    return (int)hipGetLastError();
}

int launch_fog(const DevState& S, uint8_t* fog, uint8_t* know, int8_t* sight, void* stream) {
    hipLaunchKernelGGL(evg_fog_kernel, dim3((2 * S.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), S, fog, know, sight);
    return (int)hipGetLastError();
}

int launch_pack_results(const DevState& S, float* out, long long* counts, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (counts) {
        const hipError_t me = hipMemsetAsync(counts, 0, 4 * sizeof(long long), s);
        if (me != hipSuccess) return (int)me;
    }
    hipLaunchKernelGGL(evg_pack_results_kernel, dim3((S.N + 255) / 256), dim3(256), 0, s, S, reinterpret_cast<float4*>(out), counts);
    return (int)hipGetLastError();
}

static LeagueArgs league_args(const evg_league& lg) {
    return LeagueArgs{lg.weights, lg.assign, lg.objects, lg.counts, lg.ctl, lg.num_members, lg.seat, lg.resample ? 1 : 0};
}
int launch_league_clear(const DevState& S, const evg_league& lg, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t me = hipMemsetAsync(lg.counts, 0, (size_t)lg.num_members * 4 * sizeof(unsigned long long), s);
    if (me == hipSuccess) me = hipMemsetAsync(lg.ctl, 0, 2 * sizeof(unsigned long long), s);
    if (me != hipSuccess) return (int)me;
    hipLaunchKernelGGL(evg_league_clear_kernel, dim3((S.N + 255) / 256), dim3(256), 0, s, S, league_args(lg));
    return (int)hipGetLastError();
}
int launch_league_assign(const DevState& S, const evg_league& lg, const uint8_t* mask, void* stream) {
    hipLaunchKernelGGL(evg_league_assign_kernel, dim3((S.N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), S, league_args(lg), mask);
    return (int)hipGetLastError();
}
int launch_league_importance(const evg_league& lg, double* weights_out, void* stream) {
    hipLaunchKernelGGL(evg_league_importance_kernel, dim3(1), dim3(WG), 0, reinterpret_cast<hipStream_t>(stream), league_args(lg), weights_out);
    return (int)hipGetLastError();
}

int launch_random_actions(const DevState& S, int32_t* actions, int seat, void* stream) {
    // (a latency chain of two Philox blocks per thread; 128-thread blocks for the half-sized one-seat form are no faster: 5.4 against 5.2 us)
    const dim3 grid(((seat < 0 ? 2 : 1) * S.N + 255) / 256), block(256);
    hipLaunchKernelGGL(evg_random_actions_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), S, actions, seat);
    return (int)hipGetLastError();
}

}  // namespace evg
