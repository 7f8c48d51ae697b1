// evg_step4.inc -- the fused env-step with FOUR lanes per env (included by evg_kernels.hip, inside namespace evg, while the
// macros S / io are defined).  The product library launches it for PERSISTENT rollouts of SMALL batches and for the REMAINDER of a
// large batch behind its whole rounds (plan_step: as long as the four-lane grid is resident at two or three unspilled waves per SIMD
// -- DeviceCaps::slots4_w2 / slots4_w3 wavefronts, i.e. 32 768 / 49 152 envs on a whole MI355X), where what counts is how long ONE
// wavefront needs for a turn; the diagnostic library can select it at any size and in the single-turn form as well
// (evg_diag_configure lanes = 4).  Bit-for-bit the same results as the two-lane kernel.
//
// The rules of the turn are not written here: both mappings call the same functions of step_rules.inc.  This file holds the four-lane SCHEDULE of
// those rules -- which lane owns which groups, nodes and rows, the DPP exchanges, the LDS layout, the load and store schedules.  The tests that
// compare it with the two-lane kernel:
//   * tests/test_gpu_parity.py::test_four_lanes_per_env_variant_matches_oracle            every phase, both launch forms, against the oracle
//   * ::test_small_batch_persistent_rollout_equals_the_two_lane_kernel                     what the product launches below 49 152 envs, against the two-lane kernel
//   * ::test_damage_pool_overflow_takes_two_passes_four_lane_kernel                        the combat pool's two-pass branch of this mapping
//   * ::test_custom_tables_vs_oracle, ::test_non_default_map_and_unit_files_through_abi    runtime tables (their persistent legs run 224 / 200 envs: this kernel)
//   * ::test_persistent_multi_turn_rollout_equals_stepwise, ::test_config5_scripted_rollout_vs_oracle (small N), the scripted-bot tests at small N
//   * tests/test_abi_and_host.py::test_both_lane_mappings_cite_the_same_reference_lines    (CPU) the PHASE(k) markers come in the same order in both mappings,
//     every phase cites the same anchor ranges of server.py / everglades_env.py, both call every rule of step_rules.inc in the same phase, and no rule
//     formula is written outside step_rules.inc
//
// Mapping: lane = 4 * env_slot + 2 * player + half; one wavefront = 16 envs per workgroup; grid = N / 16.  Each (env, player)
// side is shared by two lanes: half h owns the side's groups 6h .. 6h+5 (their words, arrival stamps, movement, aggregates,
// observation rows) and half of everything else that is per side (one of the two Philox blocks of the random orders, 4 or 3 of
// the 7 order rows, 6 of the 12 sort keys, 3 of the 11 nodes of capture, ~52 of the 105 observation values).  All exchanges
// stay inside a quad: DPP quad_perm [1,0,3,2] reaches the other half, [2,3,0,1] the opponent.  A wavefront issues 2 213 VALU
// instructions per turn instead of 3 164 and there are twice as many wavefronts, but status, rewards, exchanges and the per-turn
// overhead are paid per lane: MORE instructions in total.  Persistent form, us per turn, product's choice / two-lane kernel forced / four-lane kernel
// forced (WPE 4 build), round-4 build on one box (tools/two_vs_four_lanes.py, profiles/r04_a_two_vs_four_lanes_persistent.txt): 4 096 envs 7.7 / 10.8 / 7.9,
// 8 192 envs 8.2 / 10.9 / 8.4, 16 384 envs 8.3 / 11.7 / 8.9, 24 576 envs 9.6 / 11.9 / 11.1, 32 768 envs 10.4 / 12.0 / 11.4 (product: WPE 2 build, two
// waves per SIMD), 40 960 envs 12.6 / 13.8 / 14.2, 49 152 envs 13.3 / 14.2 / 14.9 (product: WPE 3 build, three waves per SIMD, still unspilled);
// with the whole 65 536-env batch at 4 waves per SIMD (<= 128 VGPRs, 28 spilled) the SIMDs are issue-bound and the two-lane kernel wins: 15.4 against
// 18.6 us per turn.  Same HBM state; no stock-entropy (MT19937) mode; no one-seat (evg_step_vs_policy) form: single-turn launches always run the
// two-lane kernel (tools/single_turn_lanes.py: no better with four lanes).

struct __align__(16) Step4Lds {
    static constexpr int COLS = 32;          // env sides per wavefront
    static constexpr int DP_CAP = 640;       // words of the damage pool (two passes of 8 envs each when a wave needs more)
    uint32_t G[12][COLS];                    // group words [gid][col], col = 2 * env_slot + player
    uint16_t NW[12][COLS / 2];               // node words by node ID, one column per env
    union {
        struct {
            uint32_t SNAP[12][COLS];         // bit31 fights | list-order prefix of alive units << 16 | node << 12 | alive mask
            uint32_t FS[12][COLS];           // the side at node n: alive fighting units << 16 | word offset of its damage bytes in DP
            uint32_t TURN[COLS], EPI[COLS];
            uint16_t W[COLS * 12];           // work list: col | gid << 5
            uint32_t DP[DP_CAP];
        } c;
        uint32_t A[12][COLS];                // per (side, node): capture points | units listed << 16
        int16_t  O[COLS * OBS];              // observations in output order [env][player][105]
    } u;
    LdsTables tab;
};
static_assert(sizeof(Step4Lds) <= 10240, "16 workgroups per CU (4 waves per SIMD) need <= 10 240 B of LDS each");

// value held by the other half of the same side (lane ^ 1) / by the same half of the opposing side (lane ^ 2)
__device__ __forceinline__ int xH(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ int xP(int v) { return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true); }   // quad_perm [2,3,0,1]

// 6-input sorting network (12 compare-exchanges, depth 5; checked with the 0-1 principle in tools/gen_sort12.py)
#define EVG_SORT6_CES(CE) CE(0, 5) CE(1, 3) CE(2, 4) CE(1, 2) CE(3, 4) CE(0, 3) CE(2, 5) CE(0, 1) CE(2, 3) CE(4, 5) CE(1, 2) CE(3, 4)

// WPE: waves per SIMD the register allocation aims at.  4 = the whole 65 536-env batch resident (<= 128 VGPRs, 28 spilled; the
// diagnostic experiment); 2 and 3 = 158 VGPRs, nothing spilled: the forms the product launches for up to 32 768 / 49 152 envs.
template <typename OT, bool MULTI, int WPE = 4>
__global__ void __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) evg_step4_kernel(StepArgs) {
    step_args_ptr A = (step_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int EPW = 16;                             // envs per wavefront
    constexpr int DP_CAP = Step4Lds::DP_CAP;
    __shared__ Step4Lds L;
    const int lane = threadIdx.x;
    const int E = lane >> 2, P = (lane >> 1) & 1, H = lane & 1;
    const int e0 = io.env_lo + blockIdx.x * EPW;      // this launch plays envs [env_lo, env_hi) of the handle (launch_step)
    const int nvalid = min(EPW, io.env_hi - e0);
    const bool valid = E < nvalid;
    const int e = valid ? e0 + E : e0;
    const size_t N = (size_t)S.N;
    const DevTables* T = S.T;

    STAMP(0);
    STAMP_WAVE_BEGIN();
    // ---- prologue loads: the constant tables (one blob, already in its LDS layout) and this lane's share of the state
    constexpr int TV = (int)(sizeof(LdsTables) / 16);
    static_assert(TV > WG && TV <= 2 * WG, "table blob is copied in two rounds");
    const uint4* timg = reinterpret_cast<const uint4*>(&T->lds);
    const uint4 tv0 = timg[lane], tv1 = timg[lane + WG < TV ? lane + WG : 0];
    const uint32_t envw = S.env[e];
    uint32_t episode = S.episode[e];
    float ep_ret = S.ep_ret[(size_t)P * N + e];         // this side's running episode return (half 0 keeps it)
    uint32_t g_in[6], sw[3], n_in[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) g_in[k] = S.grp[(size_t)(P * 12 + H * 6 + k) * N + e];
#pragma unroll
    for (int j = 0; j < 3; ++j) sw[j] = S.stamp[(size_t)(P * 3 + j) * N + e];
    const int q = lane & 3;                             // the quad's four lanes share the env's 6 node words: lane q loads words q and q + 4
    n_in[0] = S.node[(size_t)q * N + e];
    n_in[1] = S.node[(size_t)(q < 2 ? q + 4 : q) * N + e];
    uint32_t ag_cycle = 0, ag_swarm = 0, ag_dfs = 0;    // fused scripted agents: both halves keep a copy of their seat's agent object
    const size_t ai = (size_t)P * N + e;
    if (io.gen_actions == 2) { ag_cycle = S.agent_cycle[ai]; ag_swarm = S.agent_swarm[ai]; ag_dfs = S.agent_dfs[ai]; }
    // caller-supplied orders (evg_step): half 0 takes rows 0..3 of its side, half 1 rows 4..6
    int2 act_in[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) act_in[i] = make_int2(0, 0);
    if (!MULTI && !io.gen_actions && io.actions) {
        const int2* ap = reinterpret_cast<const int2*>(io.actions) + ((size_t)e * 2 + P) * NA + H * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < 3 || !H) act_in[i] = ap[i];
    }
    int turn = (int)(envw & 0xFFu);
    int status = (int)((envw >> 8) & 3u);
    // this half's six arrival stamps as two private words (bytes k = 0..3 | 4, 5) out of the side's three
    uint32_t s_lo = H ? ((sw[1] >> 16) | (sw[2] << 16)) : sw[0];
    uint32_t s_hi = H ? (sw[2] >> 16) : (sw[1] & 0xFFFFu);
    {
        uint4* lt = reinterpret_cast<uint4*>(&L.tab);
        lt[lane] = tv0;
        if (lane + WG < TV) lt[lane + WG] = tv1;
    }
    const int col0 = lane >> 1;
#pragma unroll
    for (int k = 0; k < 6; ++k) L.G[H * 6 + k][col0] = g_in[k];
    {
        const int n0 = 2 * q + 1;                       // word q: nodes 2q+1, 2q+2; word q+4 (q < 2): nodes 2q+9, 2q+10
        L.NW[n0][E] = (uint16_t)(n_in[0] & 0xFFFFu);
        L.NW[n0 + 1][E] = (uint16_t)(n_in[0] >> 16);
        if (q < 2) {
            L.NW[n0 + 8][E] = (uint16_t)(n_in[1] & 0xFFFFu);
            if (n0 + 9 <= NN) L.NW[n0 + 9][E] = (uint16_t)(n_in[1] >> 16);
        }
    }
    WAVE_SYNC();
    const bool observe_only = io.observe_only != 0;

    const int nturns = MULTI ? io.turns : 1;
    for (int iter = 0; iter < nturns; ++iter) {
    int lane_ = threadIdx.x;
    if (MULTI) { asm volatile("" : "+s"(A)); asm volatile("" : "+v"(lane_)); T = S.T; }
    const int lane = lane_;
    if (MULTI && WPE <= 3 && (io.flags & STEP_F_SHARED_SIMD)) {
        // more wavefronts than SIMDs (launch_step sets the flag from the device's SIMD count; the largest batches this kernel is launched for): the same
        // tie-free issue priorities as in
        // the two-lane kernel -- hardware slot 1 at priority 1, the even slots at 2 in three turns of five and at 0 otherwise
        // (persistent form, us per turn: 11.1 -> 10.4 at 32 768 envs, 10.4 -> 9.6 at 24 576).  With TWO waves per SIMD that is
        // tie-free; with THREE (WPE = 3 build, 32 769 .. 49 152 envs) slots 0 and 2 follow the same 2 / 0 schedule, so between those
        // two the arbiter's age order still decides -- only slot 1 is separated from both (measured as it is: 14.0 -> 12.9 us at 40 960)
        if (__builtin_amdgcn_s_getreg(6148) & 1u) __builtin_amdgcn_s_setprio(1);
        else if ((0x15u >> (iter % 5)) & 1u) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
    }
    if (MULTI) { PHASE(0); }
    const int E = lane >> 2, P = (lane >> 1) & 1, H = lane & 1, q = lane & 3;
    const int col = lane >> 1;                          // LDS column of this lane's side
    const bool valid = E < nvalid;
    const int e = valid ? e0 + E : e0;
    const size_t N = (size_t)S.N;
    const uint64_t p1nib = L.tab.nib[0];
    // this half's groups are 6H .. 6H+5: their nibbles sit 24 bits up in the per-side tables
    const uint32_t spd_h = (uint32_t)(L.tab.nib[1 + P] >> (24 * H)), ctl_h = (uint32_t)(L.tab.nib[3 + P] >> (24 * H));
    const uint32_t cst_h = (uint32_t)(L.tab.nib[5 + P] >> (24 * H)), typ_h = (uint32_t)(L.tab.nib[7 + P] >> (24 * H));
    const uint32_t misc = (uint32_t)L.tab.nib[9];
    const int max_turns = (int)(misc & 0xFFu);

    // ---------------- this side's 7 order rows as two nibble words (row i = nibble i): groups in gp7, nodes in np7.  For orders
    // that are not drawn here the lane's own rows (H * 4 + s) are kept in full in act_mine.
    uint32_t gp7 = 0, np7 = 0;
    int2 act_mine[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) act_mine[i] = act_in[i];
    if (io.gen_actions == 1) {
        // random_actions stand-in (gen_random_rows above, oracle/rng_spec.py): half 0 draws the 7 distinct groups from block 0,
        // half 1 the 7 distinct nodes from block 1 -- the same partial Fisher-Yates on a nibble-packed permutation with different
        // constants -- and the halves swap their results
        const uint4 x = rng_block(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, RNG_ACTION, (uint32_t)H, turn, 0, P, 0);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
        uint64_t perm = H ? 0xBA987654321ull : 0xBA9876543210ull;
        const uint32_t span = H ? 11u : 12u;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int j = i + (int)(__umul24(rng_half(w, i), span - (uint32_t)i) >> 16);
            const uint64_t d = ((perm >> (4 * i)) ^ (perm >> (4 * j))) & 15ull;
            perm ^= (d << (4 * i)) ^ (d << (4 * j));
        }
        const uint32_t mine = (uint32_t)perm & 0x0FFFFFFFu, other = (uint32_t)xH((int)mine);
        gp7 = H ? other : mine;
        np7 = H ? mine : other;
    } else if (io.gen_actions == 2) {
        // on-device scripted agents: both halves evaluate their seat's bot (identical results, identical agent objects)
        int2 rows[NA];
        const ChipView<Step4Lds> view{&L, col, E, P, turn, p1nib};
        const AgentTabs atabs{L.tab.nib[11], L.tab.nib[12], L.tab.nib[13], T};
        agent_rows(P ? io.policy1 : io.policy0, view, atabs, S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, P, true, status == 0,
                   &ag_cycle, &ag_swarm, &ag_dfs, rows);
        if (valid && !H && (!MULTI || iter == nturns - 1)) {
            const size_t ai_ = (size_t)P * N + e;
            S.agent_cycle[ai_] = ag_cycle; S.agent_swarm[ai_] = ag_swarm; S.agent_dfs[ai_] = ag_dfs;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int2 lo = rows[i], hi = i < 3 ? rows[4 + i] : make_int2(0, 0);
            act_mine[i] = H ? hi : lo;
        }
    }
    if (io.gen_actions && valid && io.actions_out) {
        int2* ao = reinterpret_cast<int2*>(io.actions_out) + ((size_t)e * 2 + P) * NA + H * 4;
        if (io.gen_actions == 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < 3 || !H) ao[i] = make_int2((int)((gp7 >> (4 * (H * 4 + i))) & 15u), (int)((np7 >> (4 * (H * 4 + i))) & 15u));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < 3 || !H) ao[i] = act_mine[i];
        }
    }
    PHASE(1);

    const bool frozen = status != 0;                    // finished, not auto-reset: repeat terminal outputs
    const bool play = valid && !frozen && !observe_only;

    if (play) {
        turn += 1;                                                               // server.py:214
        // ---------------- orders (server.py:218-271): each half evaluates its own rows (0..3 | 4..6) from the pre-order words
        const uint64_t node_map = player_node_map(P, p1nib);
        if (!ABLATED(1u) && io.gen_actions == 1) {
            // drawn above: 7 DISTINCT groups in 0..11, nodes in 1..11 -> no domain checks, no "already commanded" test
            uint32_t gv[4], wv[4], nv[4], dv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint32_t sh = 4u * (uint32_t)(H * 4 + s);
                gv[s] = (gp7 >> sh) & 15u;
                nv[s] = map_node(node_map, (np7 >> sh) & 15u);
                wv[s] = L.G[gv[s]][col];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) dv[s] = order_dist(L.tab.adj[wv[s] & G_LOC_M], nv[s]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if ((s < 3 || !H) && order_accepted(wv[s], dv[s])) L.G[gv[s]][col] = ordered_word(wv[s], nv[s], dv[s]);
        } else if (!ABLATED(1u)) {
            // general rows (evg_step's tensor, scripted bots): the "already commanded" chain (:241, :252) runs over half 0's rows first, its result
            // crosses to half 1, whose rows follow
            int gidv[4], nidv[4], rawv[4];
            uint32_t wv[4], dv[4];
            bool condv[4], accv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                gidv[s] = act_mine[s].x; nidv[s] = act_mine[s].y;
                condv[s] = order_ids(gidv[s], nidv[s], rawv[s], node_map, P) && (s < 3 || !H);
                wv[s] = L.G[gidv[s]][col];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                dv[s] = order_dist(L.tab.adj[wv[s] & G_LOC_M], (uint32_t)nidv[s]);
                condv[s] = condv[s] && order_accepted(wv[s], dv[s]);
            }
            uint32_t used = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {                         // half 0's chain
                accv[s] = condv[s] && !((used >> rawv[s]) & 1u);
                used |= (accv[s] && !H ? 1u : 0u) << rawv[s];
            }
            const uint32_t used0 = (uint32_t)xH((int)used);       // for half 1: what half 0 accepted
            if (H) {
                used = used0;
#pragma unroll
                for (int s = 0; s < 4; ++s) {                     // half 1's chain
                    accv[s] = condv[s] && !((used >> rawv[s]) & 1u);
                    used |= (accv[s] ? 1u : 0u) << rawv[s];
                }
            }
            // aliased ids (a negative index naming the same group): the later row wins like in the reference, so half 0's rows
            // are written by earlier instructions than half 1's
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (H == hh && accv[s]) L.G[gidv[s]][col] = ordered_word(wv[s], (uint32_t)nidv[s], dv[s]);
        }
    }
    WAVE_SYNC();
    PHASE(2);

    // ---------------- combat (server.py:503-654), stage 0: pre-combat snapshot of this half's six groups
    uint32_t g[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = L.G[H * 6 + k][col];
    uint32_t occ = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t w = g[k];
        const bool elig = (w & G_MASK_M) != 0 && ((w & G_MODE_M) >> G_MODE_S) != MODE_MOVING;
        occ |= (elig ? 1u : 0u) << (w & G_LOC_M);
    }
    occ |= (uint32_t)xH((int)occ);
    const uint32_t contested = (play && !ABLATED(2u)) ? (occ & (uint32_t)xP((int)occ)) : 0u;
    if (__any(contested != 0)) {
        // list order = (arrival stamp, gid) order (SURVEY App. C): each half sorts its six keys, one half-cleaner step across the
        // pair leaves the six smallest in half 0 and the six largest in half 1, and each half sorts again
        uint32_t key[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t w = g[k];
            const uint32_t mask = (w & G_MASK_M) >> G_MASK_S;
            const uint32_t elig = (mask != 0 && ((w & G_MODE_M) >> G_MODE_S) != MODE_MOVING) ? 1u : 0u;
            const uint32_t stamp = k < 4 ? (s_lo >> (8 * k)) & 0xFFu : (s_hi >> (8 * (k - 4))) & 0xFFu;
            key[k] = (stamp << 21) | ((uint32_t)(H * 6 + k) << 17) | ((w & G_LOC_M) << 13) | (mask << 1) | elig;
        }
#define EVG_CE(a, b) { const uint32_t lo_ = min(key[a], key[b]); key[b] = max(key[a], key[b]); key[a] = lo_; }
        EVG_SORT6_CES(EVG_CE)
        {
            uint32_t o[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] = (uint32_t)xH((int)key[5 - i]);
#pragma unroll
            for (int i = 0; i < 6; ++i) key[i] = H ? max(key[i], o[i]) : min(key[i], o[i]);
        }
        EVG_SORT6_CES(EVG_CE)
#undef EVG_CE
        // list positions 6H .. 6H+5: running per-node sums of alive fighting units (bytes of a0..a2) inside the half ...
        uint32_t a0 = 0, a1 = 0, a2 = 0, fmask = 0, snap[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint32_t kk = key[i];
            const uint32_t gid = (kk >> 17) & 15u, loc = (kk >> 13) & 15u, mask = (kk >> 1) & 0xFFFu;
            const bool fights = (kk & 1u) && ((contested >> loc) & 1u);
            const uint32_t idx = loc >> 2, sh = (loc & 3u) * 8;
            const uint32_t cur = idx == 0 ? a0 : (idx == 1 ? a1 : a2);
            const uint32_t base = (cur >> sh) & 0xFFu;
            const uint32_t add = fights ? (uint32_t)__popc(mask) << sh : 0u;
            a0 += idx == 0 ? add : 0u;
            a1 += idx == 1 ? add : 0u;
            a2 += idx == 2 ? add : 0u;
            fmask |= (fights ? 1u : 0u) << gid;
            snap[i] = fights ? (0x80000000u | (base << 16) | (loc << 12) | mask) : 0u;
        }
        // ... plus, for half 1, what half 0 lists before it at the same node
        const uint32_t b0 = (uint32_t)xH((int)a0), b1 = (uint32_t)xH((int)a1), b2 = (uint32_t)xH((int)a2);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint32_t gid = (key[i] >> 17) & 15u, loc = (key[i] >> 13) & 15u;
            const uint32_t idx = loc >> 2, sh = (loc & 3u) * 8;
            const uint32_t before = ((idx == 0 ? b0 : (idx == 1 ? b1 : b2)) >> sh) & 0xFFu;
            L.u.c.SNAP[gid][col] = snap[i] + ((H && snap[i]) ? before << 16 : 0u);
        }
        a0 += b0; a1 += b1; a2 += b2;                   // the side's totals per node, known to both halves
        if (!H) { L.u.c.TURN[col] = (uint32_t)turn; L.u.c.EPI[col] = episode; }
        int ndw = 0;                                    // damage bytes of this side, a word-rounded run per node: counted by half 0
        if (!H) {
            uint32_t c = contested;
            while (c) {
                const uint32_t n = (uint32_t)__ffs(c) - 1u;
                c &= c - 1;
                const uint32_t aw = (n >> 2) == 0 ? a0 : ((n >> 2) == 1 ? a1 : a2);
                ndw += (int)((((aw >> ((n & 3u) * 8)) & 0xFFu) + 3u) >> 2);
            }
        }
        PHASE(3);

        // Stage 1: wave-wide work list (one item per fighting group, the 12-unit group's items last) and damage-pool layout
        const int nf_a = __popc(fmask & 0x7FFu), nf_b = (int)((fmask >> 11) & 1u);
        const int packed = nf_a | (nf_b << 10) | (ndw << 17);
        int incl = packed;
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, false);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, false);
        const int excl = incl - packed;
        const int tot = __builtin_amdgcn_readlane(incl, WG - 1), mid = __builtin_amdgcn_readlane(excl, WG / 2);
        const int excl_a = excl & 0x3FF, excl_b = (excl >> 10) & 0x7F, excl_d = excl >> 17;
        const int tot_a = tot & 0x3FF, tot_b = (tot >> 10) & 0x7F, tot_d = tot >> 17, mid_a = mid & 0x3FF, mid_b = (mid >> 10) & 0x7F, mid_d = mid >> 17;
        const int npass = tot_d <= DP_CAP ? 1 : 2;      // the pool holds every fight of the wave in the common case; else envs 0..7, then 8..15
        const uint32_t dmg_nib = (misc >> 8) & 0xFFFFu;
        const bool fast_div = ((misc >> 24) & 1u) != 0;
        for (int ps = 0; ps < npass; ++ps) {
            const bool inpass = npass == 1 || (lane / (WG / 2)) == ps;
            const bool second = npass == 2 && ps == 1, first = npass == 2 && ps == 0;
            const int ref_a = second ? mid_a : 0, ref_b = second ? mid_b : 0, ref_d = second ? mid_d : 0;
            const int end_a = first ? mid_a : tot_a, end_b = first ? mid_b : tot_b, end_d = first ? mid_d : tot_d;
            const int na = end_a - ref_a, nitems = na + (end_b - ref_b), ndwords = end_d - ref_d;
            if (inpass) {
                int wi = excl_a - ref_a;
                uint32_t f = fmask & 0x7FFu;
                while (f) {
                    const uint32_t gid = (uint32_t)__ffs(f) - 1u;
                    f &= f - 1;
                    L.u.c.W[wi++] = (uint16_t)((uint32_t)col | (gid << 5));
                }
                if (nf_b) L.u.c.W[na + excl_b - ref_b] = (uint16_t)((uint32_t)col | (11u << 5));
                if (!H) {
                    int doff = excl_d - ref_d;
                    uint32_t c = contested;
                    while (c) {
                        const uint32_t n = (uint32_t)__ffs(c) - 1u;
                        c &= c - 1;
                        const uint32_t aw = (n >> 2) == 0 ? a0 : ((n >> 2) == 1 ? a1 : a2);
                        const uint32_t tn = (aw >> ((n & 3u) * 8)) & 0xFFu;
                        L.u.c.FS[n][col] = (tn << 16) | (uint32_t)doff;
                        doff += (int)((tn + 3u) >> 2);
                    }
                }
            }
            for (int i = lane; i < ndwords; i += WG) L.u.c.DP[i] = 0;
            WAVE_SYNC();
            PHASE(4);

            // Phase A (:549-566): one lane per fighting group; each of its alive units draws one target among the opposing side's
            // alive fighting units at the node; damage accumulates in the pool (LDS atomics: integer, order-free, deterministic)
            const uint32_t seed_lo = S.seed_lo, seed_hi = S.seed_hi, id_base = S.env_id_base + (uint32_t)e0;
            for (int it = lane; it < nitems; it += WG) {
                const uint32_t item = L.u.c.W[it];
                const int SL = (int)(item & 31u), gid = (int)(item >> 5), side = SL & 1;
                const uint32_t sp = L.u.c.SNAP[gid][SL];
                const int node = (int)((sp >> 12) & 15u), cnt = __popc(sp & 0xFFFu);
                const uint32_t fso = L.u.c.FS[node][SL ^ 1];
                const uint32_t tot_o = fso >> 16, doff_o = fso & 0xFFFFu;
                const uint64_t tn_s = L.tab.nib[7 + side];
                const uint32_t type = (uint32_t)((tn_s >> (4 * gid)) & 15u);
                const uint32_t dmg = (dmg_nib >> (4 * type)) & 15u;
                const int turn_e = (int)L.u.c.TURN[SL];
                const uint32_t epi_e = L.u.c.EPI[SL], env_id_e = id_base + (uint32_t)(SL >> 1);
                for (int b = 0; b * 8 < cnt; ++b) {               // one block = eight 16-bit draws: a second one only for the 12-unit group
                    const uint4 x = rng_block(seed_lo, seed_hi, env_id_e, epi_e, RNG_COMBAT, (uint32_t)b, turn_e, node, side, gid);
                    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (b * 8 + i < cnt) {
                            const uint32_t uid = __umul24(rng_half(xs, i), tot_o) >> 16;                // :562 (tot_o <= 100)
                            atomicAdd(&L.u.c.DP[doff_o + (uid >> 2)], dmg << (8 * (uid & 3u)));         // :563-566
                        }
                    }
                }
            }
            WAVE_SYNC();
            PHASE(5);

            // Phase B (:573-644): one lane per fighting group; see the two-lane kernel for the byte gymnastics
            for (int it = lane; it < nitems; it += WG) {
                const uint32_t item = L.u.c.W[it];
                const int SL = (int)(item & 31u), gid = (int)(item >> 5), side = SL & 1;
                const uint32_t sp = L.u.c.SNAP[gid][SL];
                const int node = (int)((sp >> 12) & 15u);
                const uint32_t mask = sp & 0xFFFu;
                const uint32_t doff = L.u.c.FS[node][SL] & 0xFFFFu;
                const uint32_t base = (sp >> 16) & 0xFFu;
                const uint32_t run0 = doff * 4u + base, w0i = run0 >> 2, sh0 = run0 & 3u;
                uint32_t dw[4];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) dw[qd] = L.u.c.DP[min(w0i + (uint32_t)qd, (uint32_t)(DP_CAP - 1))];
                const uint32_t cnt = (uint32_t)__popc(mask);                                          // 1..12
                uint32_t d0 = __builtin_amdgcn_alignbyte(dw[1], dw[0], sh0), d1 = __builtin_amdgcn_alignbyte(dw[2], dw[1], sh0);
                uint32_t d2 = __builtin_amdgcn_alignbyte(dw[3], dw[2], sh0);
                {
                    const uint64_t keep = cnt >= 8u ? ~0ull : ((1ull << (8u * cnt)) - 1ull);
                    d0 &= (uint32_t)keep; d1 &= (uint32_t)(keep >> 32);
                    d2 = cnt > 8u ? (cnt >= 12u ? d2 : (d2 & ((1u << (8u * (cnt - 8u))) - 1u))) : 0u;
                }
                if ((d0 | d1 | d2) != 0u) {
                    double* row = S.health + (size_t)(e0 + (SL >> 1)) * (2 * NU) + side * NU + gid * 8;
                    double h[12];
                    {
                        const double2* r2 = reinterpret_cast<const double2*>(row);
#pragma unroll
                        for (int sl = 0; sl < 4; ++sl) { const double2 v = r2[sl]; h[2 * sl] = v.x; h[2 * sl + 1] = v.y; }
                        if (gid == 11) {
#pragma unroll
                            for (int sl = 4; sl < 6; ++sl) { const double2 v = r2[sl]; h[2 * sl] = v.x; h[2 * sl + 1] = v.y; }
                        } else {
                            h[8] = h[9] = h[10] = h[11] = 0.0;
                        }
                    }
                    const uint32_t type = (uint32_t)((L.tab.nib[7 + side] >> (4 * gid)) & 15u);
                    const int di = damage_index(type, L.NW[node][SL >> 1], side, node);      // node defence of the controlling side, :592-597
                    const double denom = L.tab.den[di], rcp = L.tab.rcp[di];
                    uint32_t deadmask = 0;
                    auto apply_hits = [&](auto fast) { deadmask = hit_slots<decltype(fast)::value>(h, 0, gid == 11, mask, d0, d1, d2, denom, rcp); };
                    if (fast_div) apply_hits(std::true_type{}); else apply_hits(std::false_type{});       // quotient :601, subtraction :609; one body per form
                    const uint32_t newmask = mask & ~deadmask;
                    double2* w2 = reinterpret_cast<double2*>(row);
#pragma unroll
                    for (int sl = 0; sl < 4; ++sl) w2[sl] = make_double2(h[2 * sl], h[2 * sl + 1]);
                    double sum = np_sum8(h);
                    if (gid == 11) {
#pragma unroll
                        for (int sl = 4; sl < 6; ++sl) w2[sl] = make_double2(h[2 * sl], h[2 * sl + 1]);
                        sum = health_sum_tail(sum, h);
                    }
                    const uint32_t w = L.G[gid][SL];
                    L.G[gid][SL] = hit_word(w, newmask, sum);
                }
            }
            WAVE_SYNC();
        }
    }
    PHASE(6);

    // ---------------- movement of this half's groups (server.py:656-706), branch-free
    uint32_t gw[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) gw[k] = L.G[H * 6 + k][col];
    if (play && !ABLATED(4u)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            bool arrive;
            gw[k] = move_group(gw[k], (spd_h >> (4 * k)) & 15u, arrive);
            if (k < 4) { const uint32_t sh = 8 * k; s_lo = arrive ? ((s_lo & ~(0xFFu << sh)) | ((uint32_t)turn << sh)) : s_lo; }
            else { const uint32_t sh = 8 * (k - 4); s_hi = arrive ? ((s_hi & ~(0xFFu << sh)) | ((uint32_t)turn << sh)) : s_hi; }
        }
    }
    PHASE(7);

    // ---------------- per-node aggregates of this side (post-movement): capture points | units listed << 16
#pragma unroll
    for (int k = 0; k < 6; ++k) L.u.A[H * 6 + k][col] = 0;
    WAVE_SYNC();        // both halves' zeros before either half's adds (different rows of the same column)
    int my_unit_score = 0, my_alive = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t w = gw[k];
        const int cnt = __popc(w & G_MASK_M);
        atomicAdd(&L.u.A[w & G_LOC_M][col], node_contribution(w, cnt, (ctl_h >> (4 * k)) & 15u));   // ds_add_u32 (0 for a destroyed group)
        my_unit_score += unit_score(cnt, (cst_h >> (4 * k)) & 15u);
        my_alive += cnt;
    }
    my_unit_score += xH(my_unit_score);
    my_alive += xH(my_alive);
    WAVE_SYNC();

    // ---------------- capture (server.py:708-767) and node scores (:297-310): the quad splits the nodes, three each
    int part0 = 0, part1 = 0, base_cap = 0;
    {
        uint32_t a0v[3], a1v[3], nwv[3];
        int cpv[3], tsv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int n = (3 * q + 1 + j) % 12;       // j = 2 of lane 3 is the unused slot 0
            a0v[j] = L.u.A[n][col & ~1];
            a1v[j] = L.u.A[n][col | 1];
            nwv[j] = L.NW[n][E];
            cpv[j] = L.tab.cp[n];
            tsv[j] = L.tab.ts[n];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int n = 3 * q + 1 + j;
            const NodeTurn r = capture_node(nwv[j], (int)(a0v[j] & 0xFFFFu), (int)(a1v[j] & 0xFFFFu), cpv[j], tsv[j], n <= NN, play);
            L.NW[n % 12][E] = (uint16_t)r.nw;             // (unchanged when nothing is captured; slot 0 -- n = 12 -- does not exist and is never read)
            base_cap |= r.base_cap ? 1 : 0;
            part0 += r.part0;
            part1 += r.part1;
        }
    }
    // combine the quad: scores (server.py:291-317) and status (:321-328) are then known to all four lanes
    const int opp_unit_score = xP(my_unit_score), opp_alive = xP(my_alive);
    part0 += xH(part0); part0 += xP(part0);
    part1 += xH(part1); part1 += xP(part1);
    base_cap |= xH(base_cap); base_cap |= xP(base_cap);
    int score[2];
    score[0] = part0 + (P ? opp_unit_score : my_unit_score);
    score[1] = part1 + (P ? my_unit_score : opp_unit_score);
    status = play ? status_after_turn(status, turn, max_turns, my_alive + opp_alive, base_cap != 0) : status;      // :321-328
    PHASE(8);

    // ---------------- reward / done / winner (everglades_env.py:37-61, evaluate.py:155-160)
    const bool done = status != 0;
    const TurnOutcome out = turn_outcome(done, score[0], score[1]);
    const float rew0 = out.rew0, rew1 = out.rew1;
    const int winner = out.winner;
    {
        float* const p_reward = io.reward;
        uint8_t* const p_done = io.done;
        int8_t* const p_winner = io.winner;
        int32_t* const p_scores = io.scores;
        uint8_t* const p_status = io.status;
        if (valid && !observe_only && q == 0) {
            reinterpret_cast<float2*>(p_reward)[e] = make_float2(rew0, rew1);
            p_done[e] = done ? 1 : 0;
            if (p_winner) p_winner[e] = (int8_t)winner;
            if (p_scores) reinterpret_cast<int2*>(p_scores)[e] = make_int2(score[0], score[1]);
            if (p_status) p_status[e] = (uint8_t)status;
        }
    }

    // ---------------- episode bookkeeping + auto-reset (half 0 of each side keeps the side's return)
    bool do_reset = false;
    float* const p_fin_ret = S.fin_ret;
    int32_t* const p_fin_len = S.fin_len;
    int8_t* const p_fin_win = S.fin_win;
    const int auto_reset = S.auto_reset;
    if (play) {
        float r = ep_ret + (P ? rew1 : rew0);
        if (done) {
            if (!H) p_fin_ret[(size_t)e * 2 + P] = r;
            if (q == 0) { p_fin_len[e] = turn; p_fin_win[e] = (int8_t)winner; }
            if (auto_reset) { do_reset = true; r = 0.f; }
        }
        ep_ret = r;
    }
    if (valid && !observe_only && !H && (!MULTI || iter == nturns - 1)) S.ep_ret[(size_t)P * N + e] = ep_ret;
    {
        const bool fin = play && done && q == 0;
        const uint64_t mf = __ballot(fin);
        if (mf) {
            const uint64_t m0 = __ballot(fin && winner == EVG_WINNER_P0), m1 = __ballot(fin && winner == EVG_WINNER_P1);
            if (lane == 0) {
                const int nf = __popcll(mf), n0 = __popcll(m0), n1 = __popcll(m1);
                atomicAdd(&S.totals[0], (unsigned long long)nf);
                if (n0) atomicAdd(&S.totals[1], (unsigned long long)n0);
                if (n1) atomicAdd(&S.totals[2], (unsigned long long)n1);
                if (nf - n0 - n1) atomicAdd(&S.totals[3], (unsigned long long)(nf - n0 - n1));
            }
        }
    }
    if (do_reset) {
        // new episode: state of game_init (server.py:133-209)
        turn = 0; status = 0; episode += 1u;
        s_lo = s_hi = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) gw[k] = L.tab.init_grp[P * 12 + H * 6 + k];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int n = 3 * q + 1 + j;
            if (n <= NN) L.NW[n][E] = (uint16_t)L.tab.init_node[n];
        }
    }
    WAVE_SYNC();        // node words final; everybody is done adding to A
    PHASE(9);

    // ---------------- observation of this side (board_state :382-455, player_state :457-501, everglades_env.py:158-171): half 0
    // writes the turn, board slots 1..5 and groups 0..5, half 1 board slots 6..11 and groups 6..11, as int16 into the output image
    const bool want_obs = io.obs != nullptr;            // a rollout without an observation buffer skips the image and the write-out
    if (want_obs) {
    const uint64_t node_map = player_node_map(P, p1nib);
    int ns[6], ou_s[6];
    uint32_t nw_s[6];
    const uint32_t keep_units = do_reset ? 0u : ~0u;    // an env that starts a new episode shows the game_init position
    const uint32_t opp_base = do_reset ? (L.tab.init_grp[(1 - P) * 12] & G_LOC_M) : 0xFFu;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int i = 1 + j + 5 * H;                                              // slot; j = 5 of half 0 is a duplicate of slot 6 and not written
        ns[j] = (int)map_node(node_map, (uint32_t)i);                             // slot i of player 1 shows node p1_node_map[i] (:437-439)
        nw_s[j] = L.NW[ns[j]][E];
        const uint32_t listed = L.u.A[ns[j]][col ^ 1] >> 16;                     // opposing units listed at the node
        ou_s[j] = (int)((listed & keep_units) | ((uint32_t)ns[j] == opp_base ? (uint32_t)NU : 0u));
    }
    WAVE_SYNC();        // A is dead from here on: the union becomes the output image
    {
        int16_t* orow = &L.u.O[col * OBS];
        if (!H) orow[0] = (int16_t)turn;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            int16_t* o = orow + 4 * (j + 5 * H) + 1;
            int v[4];
            obs_node(v, L.tab.res[ns[j]], nw_s[j], ou_s[j]);
            if (j < 5 || H) {
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = (int16_t)v[t];
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            int16_t* o = orow + 45 + 5 * (H * 6 + k);
            int v[5];
            obs_group(v, gw[k], node_map, (typ_h >> (4 * k)) & 15u, __popc(gw[k] & G_MASK_M));
#pragma unroll
            for (int t = 0; t < 5; ++t) o[t] = (int16_t)v[t];
        }
    }
    }   // want_obs
    PHASE(10);

    // ---------------- store state (coalesced; multi-turn form: after the launch's last turn)
    if (valid && !observe_only && (MULTI ? iter == nturns - 1 : (play || do_reset)) && !ABLATED(32u)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) S.grp[(size_t)(P * 12 + H * 6 + k) * N + e] = gw[k];
        {
            // the side's three stamp words from the two halves' private pairs: W0 = lo(h0), W1 = hi(h0) | lo(h1) << 16, W2 = lo(h1) >> 16 | hi(h1) << 16
            const uint32_t o_lo = (uint32_t)xH((int)s_lo);
            if (!H) {
                S.stamp[(size_t)(P * 3 + 0) * N + e] = s_lo;
                S.stamp[(size_t)(P * 3 + 1) * N + e] = (s_hi & 0xFFFFu) | (o_lo << 16);
            } else {
                S.stamp[(size_t)(P * 3 + 2) * N + e] = (s_lo >> 16) | (s_hi << 16);
            }
        }
        {
            const int n0 = 2 * q + 1;
            S.node[(size_t)q * N + e] = (uint32_t)L.NW[n0][E] | ((uint32_t)L.NW[n0 + 1][E] << 16);
            if (q < 2) S.node[(size_t)(q + 4) * N + e] = (uint32_t)L.NW[n0 + 8][E] | (n0 + 9 <= NN ? (uint32_t)L.NW[n0 + 9][E] << 16 : 0u);
        }
        if (q == 0) {
            S.env[e] = (uint32_t)turn | ((uint32_t)status << 8);
            if (MULTI || do_reset) S.episode[e] = episode;
        }
    }
    if (MULTI) {                                        // the next turn of this launch starts from these words
#pragma unroll
        for (int k = 0; k < 6; ++k) L.G[H * 6 + k][col] = gw[k];
    }
    WAVE_SYNC();        // output image complete
    PHASE(11);

    // ---------------- observation write-out: the wave's 16 x 210 values are contiguous in the output; every lane converts 16 bytes'
    // worth per iteration (conflict-free LDS reads, fully coalesced stores)
    if (want_obs && !ABLATED(16u)) {
        constexpr int EP = 16 / (int)sizeof(OT);          // elements per 16-byte vector
        constexpr int NVEC = Step4Lds::COLS * OBS / EP;
        const int limit = nvalid * OBS2;
        OT* out = reinterpret_cast<OT*>(io.obs) + (size_t)e0 * OBS2;
        auto unpack = [&](int elem0, int (&vals)[EP]) {
            if constexpr (EP == 4) {
                const uint2 raw = *reinterpret_cast<const uint2*>(&L.u.O[elem0]);
                vals[0] = (int)(int16_t)(raw.x & 0xFFFFu); vals[1] = (int)(int16_t)(raw.x >> 16);
                vals[2] = (int)(int16_t)(raw.y & 0xFFFFu); vals[3] = (int)(int16_t)(raw.y >> 16);
            } else if constexpr (EP == 2) {
                const uint32_t raw = *reinterpret_cast<const uint32_t*>(&L.u.O[elem0]);
                vals[0] = (int)(int16_t)(raw & 0xFFFFu); vals[1] = (int)(int16_t)(raw >> 16);
            } else {
                const uint4 raw = *reinterpret_cast<const uint4*>(&L.u.O[elem0]);
                const uint32_t r4[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) { vals[2 * j] = (int)(int16_t)(r4[j] & 0xFFFFu); vals[2 * j + 1] = (int)(int16_t)(r4[j] >> 16); }
            }
        };
        if (nvalid == EPW) {
            constexpr int FULL = NVEC / WG, REM = NVEC % WG, BATCH = 8;
#pragma unroll
            for (int b0 = 0; b0 < FULL; b0 += BATCH) {
                int vals[BATCH][EP];
#pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    if (b0 + j < FULL) unpack((lane + (b0 + j) * WG) * EP, vals[j]);
#pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    if (b0 + j < FULL) store_obs_vec<OT>(out + (lane + (b0 + j) * WG) * EP, vals[j]);
            }
            if (REM && lane < REM) {
                int vals[EP];
                unpack((lane + FULL * WG) * EP, vals);
                store_obs_vec<OT>(out + (lane + FULL * WG) * EP, vals);
            }
        } else {
            for (int v = lane; v < NVEC; v += WG) {            // last, partial workgroup of the grid
                const int elem0 = v * EP;
                int vals[EP];
                unpack(elem0, vals);
                if (elem0 + EP <= limit) {
                    store_obs_vec<OT>(out + elem0, vals);
                } else {
#pragma unroll
                    for (int j = 0; j < EP; ++j)
                        if (elem0 + j < limit) out[elem0 + j] = (OT)vals[j];
                }
            }
        }
    }
    PHASE(12);

    // ---------------- health of envs that start a new episode: 1600 B each, written by the whole wave
    uint64_t rm = __ballot(do_reset && q == 0);
    while (rm) {
        const int l = __ffsll((unsigned long long)rm) - 1;
        rm &= rm - 1;
        double2* dst = reinterpret_cast<double2*>(S.health + (size_t)(e0 + (l >> 2)) * (2 * NU));
        for (int i = lane; i < NU; i += WG) dst[i] = make_double2(100.0, 100.0);
    }
    PHASE(13);
    if (MULTI) WAVE_SYNC();
    }   // turns
    STAMP_WAVE_END();
}
