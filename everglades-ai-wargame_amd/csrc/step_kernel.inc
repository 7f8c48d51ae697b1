// step_kernel.inc -- evg_step_kernel: ONE fused kernel per env-step (everglades_env.py:32-73 -> server.py:211-501), in all its launch forms
// (single-turn, persistent, chunked persistent, stock-entropy, one-seat).  This file holds the skeleton -- which envs and which turns a
// workgroup plays, the prologue loads, the turn loop, the chunk hand-over -- and includes the phases of a turn, in the order the
// reference's game_turn runs them, as textual fragments of the kernel body:
//     step_orders.inc        where the 7 order rows of a lane's player come from, and their application   (server.py:218-271)
//     step_combat.inc        combat at contested nodes: stages 0 / 1 / A / B                               (server.py:503-654)
//     step_move_capture.inc  movement, per-node aggregates, capture, scores, status, rewards, episode bookkeeping, auto-reset
//                                                                                                         (server.py:656-767, 281-348; everglades_env.py:37-73)
//     step_outputs.inc       observation image, state store, observation write-out, health of restarted envs (server.py:382-501)
// A fragment is not a function: it reads and writes the locals of the kernel body (each fragment's header lists them), because the phases
// share three dozen registers (group words, stamps, turn / status / episode, the order rows) that a call boundary would have to pass.
// Included by evg_kernels.hip inside namespace evg.
// ---------------------------------------------------------------------------------------------
// fused env-step: lane = (env slot, player); LPW / 2 envs per wavefront (LPW = 64 is the default variant)
// ---------------------------------------------------------------------------------------------
// The kernel reads its arguments through the kernarg segment pointer instead of by-value parameters: in the multi-turn
// instantiation that pointer is made opaque once per turn, so argument fields and table entries are (re)loaded next to
// their uses by cheap scalar loads instead of staying live across the whole loop (which cost 60+ VGPRs in SGPR spills).
struct StepArgs { DevState s_; StepIO io_; };
typedef const StepArgs __attribute__((address_space(4))) * step_args_ptr;
#define S (A->s_)
#define io (A->io_)

// SEAT (evg_step_vs_policy, evg_observe_seat): the turn of the reference's training / evaluation loops -- a caller on seat io.seat, an on-device bot on
// the other (evaluate.py:143-152) -- as an instantiation of the single-turn form: the caller's lane takes its 7 rows from the caller's tensor, the other
// lane evaluates its bot from the on-chip state (the gen_actions == 2 machinery), and only the caller's lane builds an observation row: the wave's image
// is [32][105] and the write-out half as long.
// WPB (diagnostic library only; round-5 experiment, profiles/r05_*_single_turn_wg256.txt): wavefronts per WORKGROUP of a single-turn launch.  1 is the
// product's form (one wavefront per workgroup); 4 packs four INDEPENDENT wavefronts -- each with its own StepLds slice and its own 32 envs, still no
// s_barrier anywhere -- into a 256-thread workgroup, so that a 65 536-env launch is 512 workgroup dispatches instead of 2 048.
// QDEC (evg_step_vs_policy_smart_q): the Q form of SEAT -- the caller hands its network output instead of its orders, and the launch decodes the 7 rows
// (DQNAgent.get_action: the epsilon coin, get_random_actions / get_best_actions; smart_decode.inc) in its prologue, over the whole wavefront: the order rows
// never go through HBM and the learner's turn is one launch from the network's output to its next input.
// QDEC without SEAT (evg_step_smart_q): the Q form of the plain single-turn kernel -- self-play, a DQNAgent on each seat: both seats' rows are decoded in the
// prologue, one seat per pass through the same LDS (the two seats' Q values, 15 360 B per wave, do not fit the union at once), and both players' features are
// written after the observation write-out.
// LEAGUE (evg_step_vs_league / evg_step_vs_league_q): SEAT or SEAT + QDEC with the bot as a PER-ENV quantity -- the opponent league of include/evg.h
// (evg_league).  The league lane's policy id is a per-lane value: assign[e], loaded in the prologue's round trip next to the agent words, picks it from the
// member ids in the kernel arguments, and agent_rows -- a chain over a runtime `policy` -- runs with it (lanes of a wave that play different bots take their
// branches one after the other).  The step that ends an episode tallies it per member; with auto_reset the reset branch also draws the member of the next
// episode (league_choice) and, when it changes, swaps the agent object with the member's slot of the league store.
// HEAD (Q forms only; evg_step_vs_policy_minimized_q / evg_step_vs_league_minimized_q): which agent family's network output io.q is -- HEAD_SMART: 5
// directions per swarm, the rules above; HEAD_MINIMIZED: 11 nodes per swarm (agents/Minimized, minimized_decode.inc), read by the decode straight from the
// caller's tensor (a swarm's 11 values are 44 contiguous bytes; 32 envs x 132 floats would not fit the union), no directions.  The head is a parameter of
// the kernel BODY (step_kernel_body.inc, included as text by both kernels below): evg_step_kernel keeps its nine parameters (and with them the name and
// the instruction stream of every instantiation there was before the second head) and compiles the body with HEAD_SMART, evg_step_minimized_kernel --
// the one-seat Q form, with or without the league -- compiles it with HEAD_MINIMIZED.
constexpr int HEAD_SMART = 0, HEAD_MINIMIZED = 1;
template <typename OT, int LPW, bool MULTI, bool MT = false, bool CHUNKED = false, bool SEAT = false, int WPB = 1, bool QDEC = false, bool LEAGUE = false>
__global__ void __launch_bounds__(WG * WPB) __attribute__((amdgpu_waves_per_eu(2, 2))) evg_step_kernel(StepArgs) {
    constexpr int HEAD = HEAD_SMART;
#include "step_kernel_body.inc"
}

// the one-seat Q form with the Minimized agents' 11-way head (SeatQMin; LEAGUE: SeatQMinLeague): the body's other parameters as constants
template <typename OT, bool LEAGUE>
__global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2))) evg_step_minimized_kernel(StepArgs) {
    constexpr int LPW = WG, WPB = 1, HEAD = HEAD_MINIMIZED;
    constexpr bool MULTI = false, MT = false, CHUNKED = false, SEAT = true, QDEC = true;
#include "step_kernel_body.inc"
}

// the TWO-seat Q form with the 11-way head (evg_step_minimized_q, TwoSeatQMin: Minimized self-play, a DQNAgent on each seat): the !SEAT skeleton of the Q
// prologue -- seat 0, then seat 1 through the same LDS rows, each lane drawing both Philox blocks of its own seat's agent call -- with the decode reading
// seat p's [12][11] block of io.q [N][2][12][11]; both players' observations and features as evg_step_smart_q.
// LEAGUE (evg_step_league_minimized_q, TwoSeatQMinLeague): the seat 1 - io.seat is the league's, and ONE member -- io.lg_qmember, -1: none -- is the
// caller's second network instead of a bot: where assign[e] is that member the league seat's rows are the decode of q[e][1 - seat], elsewhere the member's
// bot plays (agent_rows) and the second decode pass skips the env.  Assignment, tally, redraw and object swap are the one-seat league forms'.
// A kernel of its own name: every instantiation of the two kernels above keeps its mangled name and its instruction stream.
template <typename OT, bool LEAGUE>
__global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(2, 2))) evg_step_minimized2_kernel(StepArgs) {
    constexpr int LPW = WG, WPB = 1, HEAD = HEAD_MINIMIZED;
    constexpr bool MULTI = false, MT = false, CHUNKED = false, SEAT = false, QDEC = true;
#include "step_kernel_body.inc"
}
