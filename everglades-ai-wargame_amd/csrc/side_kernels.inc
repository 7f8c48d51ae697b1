// side_kernels.inc -- the small kernels around the step kernel: packed episode results, the chunk-queue check, reset, MT19937 seeding, the random_actions and
// scripted-agent generators as standalone kernels, the fog-of-war / knowledge / sightings planes, the Smart_State features.  Included by evg_kernels.hip
// inside namespace evg.
// ---------------------------------------------------------------------------------------------
// per-env results of the last finished episode, packed for the path's one exchange (SURVEY 8e): 16 bytes per env
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) evg_pack_results_kernel(DevState S, float4* __restrict__ out, long long* __restrict__ counts) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const bool live = e < S.N;
    if (*S.fault != 0u) {            // a faulted handle (evg_check_fault) hands out no results: poisoned rows, winner -2 is no EVG_WINNER_* value
        const float nan = __int_as_float(0x7FC00000);
        if (live) out[e] = make_float4(nan, nan, -2.f, -1.f);
        if (counts && e < 4) counts[e] = -1;
        return;
    }
    int w = -3;
    if (live) {
        const float2 r = reinterpret_cast<const float2*>(S.fin_ret)[e];
        w = (int)S.fin_win[e];
        out[e] = make_float4(r.x, r.y, (float)w, (float)S.fin_len[e]);      // small integers are exact in float32
    }
    if (counts) {                    // win bookkeeping of these rows (evaluate.py:155-160): one atomic per wavefront and class
        const unsigned long long m0 = __ballot(w == EVG_WINNER_P0), m1 = __ballot(w == EVG_WINNER_P1), m2 = __ballot(w == EVG_WINNER_TIE);
        const unsigned long long mu = __ballot(live && w < 0);
        if ((threadIdx.x & 63) == 0) {
            if (m0) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 0), (unsigned long long)__popcll(m0));
            if (m1) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 1), (unsigned long long)__popcll(m1));
            if (m2) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 2), (unsigned long long)__popcll(m2));
            if (mu) atomicAdd(reinterpret_cast<unsigned long long*>(counts + 3), (unsigned long long)__popcll(mu));
        }
    }
}

// behind every chunked launch, on its stream: every XCD's queue must have handed out all its units (an XCD that ran no workgroup of the
// launch would leave its sets unplayed without anybody waiting for them)
struct ChunkUnits { uint32_t per_xcd[16]; };
__global__ void __launch_bounds__(WG) evg_chunk_verify_kernel(DevState S, ChunkUnits want) {
    const int x = threadIdx.x;
    if (x < S.nxcd && S.queue[x * 64] < want.per_xcd[x]) raise_fault(S.fault, S.fault_seen, 4u);
}

// ---------------------------------------------------------------------------------------------
// reset (everglades_env.py:75-116 -> server.py:133-209): masked, per env
// ---------------------------------------------------------------------------------------------
template <typename OT>
__global__ void __launch_bounds__(WG) evg_reset_kernel(DevState S, const uint8_t* mask, void* obs) {
    const int lane = threadIdx.x;
    const int e0 = blockIdx.x * WG;
    const int e = e0 + lane;
    const size_t N = (size_t)S.N;
    const DevTables* __restrict__ T = S.T;
    const bool sel = e < S.N && (mask == nullptr || mask[e] != 0);
    if (sel) {
#pragma unroll
        for (int k = 0; k < 24; ++k) S.grp[(size_t)k * N + e] = T->init_grp[k];
#pragma unroll
        for (int j = 0; j < 6; ++j) S.stamp[(size_t)j * N + e] = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            S.node[(size_t)j * N + e] = (T->init_node[2 * j + 1] & 0xFFFFu) | (2 * j + 2 <= NN ? (T->init_node[2 * j + 2] & 0xFFFFu) << 16 : 0u);
        S.env[e] = 0;
        S.episode[e] += 1u;                 // 0xFFFFFFFF at create -> episode 0 on the first reset
        S.ep_ret[e] = 0.f;
        S.ep_ret[N + e] = 0.f;
        if (S.mt_key) {                     // stock entropy: game_init's focus draw (:205) and the one of its game_end (:338, turn 0)
            MtGen mt{S.mt_key + e, N, S.mt_pos[e]};
            (void)mt_randint(mt, 2u * NG + 1u);
            (void)mt_randint(mt, 2u * NG + 1u);
            S.mt_pos[e] = mt.pos;
        }
    }
    uint64_t rm = __ballot(sel);
    while (rm) {
        const int l = __ffsll((unsigned long long)rm) - 1;
        rm &= rm - 1;
        double2* dst = reinterpret_cast<double2*>(S.health + (size_t)(e0 + l) * (2 * NU));
        for (int i = lane; i < NU; i += WG) dst[i] = make_double2(100.0, 100.0);
        if (obs) {
            OT* o = reinterpret_cast<OT*>(obs) + (size_t)(e0 + l) * (2 * OBS);
            for (int i = lane; i < 2 * OBS; i += WG) o[i] = (OT)T->reset_obs[i];
        }
    }
}

// np.random.seed(s) per env (stock-entropy mode): seeds[e], or seed + global env id when seeds == NULL
__global__ void __launch_bounds__(256) evg_mt_seed_kernel(DevState S, const uint32_t* seeds) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S.N) return;
    MtGen mt{S.mt_key + e, (size_t)S.N, 0};
    mt_seed(mt, seeds ? seeds[e] : S.seed_lo + S.env_id_base + (uint32_t)e);
    S.mt_pos[e] = mt.pos;
}

// ---------------------------------------------------------------------------------------------
// random_actions stand-in (agents/State_Machine/random_actions.py:38-46): 7 distinct groups of 12,
// 7 distinct nodes of 1..11 per player, partial Fisher-Yates on nibble-packed permutations
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) evg_random_actions_kernel(DevState S, int32_t* actions, int seat) {
    // One thread per (env, player) draws its 7 rows; the block's 256 x 56 bytes are contiguous in the output, so they go through LDS and
    // leave as 16-byte-per-lane coalesced stores (a thread's own rows are 56 bytes apart from its neighbour's: direct stores would touch
    // 28 cache lines per instruction).
    __shared__ int2 rows_lds[256 * NA];
    // seat < 0: both seats, [N][2][7][2]; seat 0 / 1: that seat's rows only, [N][7][2] (one thread per env)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int total = seat < 0 ? 2 * S.N : S.N;
    if (idx < total) {
        const int e = seat < 0 ? idx >> 1 : idx, p = seat < 0 ? idx & 1 : seat;
        const int turn = (int)(S.env[e] & 0xFFu);
        const uint32_t episode = S.episode[e];
        const uint32_t env_id = S.env_id_base + (uint32_t)e;
        int2 rows[NA];
        gen_random_rows(S.seed_lo, S.seed_hi, env_id, episode, turn, p, rows);
#pragma unroll
        for (int i = 0; i < NA; ++i) rows_lds[threadIdx.x * NA + i] = rows[i];
    }
    __syncthreads();
    const int first = blockIdx.x * 256;                                 // first (env, player) of this block
    const int nrows = min(256, total - first) * NA;                      // int2 rows this block holds (a multiple of 7)
    const uint4* src = reinterpret_cast<const uint4*>(rows_lds);
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<int2*>(actions) + (size_t)first * NA);     // 256 x 56 B per block: 16-byte aligned
    for (int v = threadIdx.x; 2 * v + 1 < nrows; v += 256) dst[v] = src[v];
    if ((nrows & 1) && threadIdx.x == 0) reinterpret_cast<int2*>(dst)[nrows - 1] = rows_lds[nrows - 1];  // odd tail of the last block
}

// standalone form of the scripted opponents: one thread per env, view = the observation tensor
template <typename OT>
__global__ void __launch_bounds__(256) evg_scripted_actions_kernel(DevState S, int policy, int player, const OT* obs, int32_t* actions) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S.N) return;
    const size_t ai = (size_t)player * S.N + e;
    const ObsView<OT> v{obs + ((size_t)e * 2 + player) * OBS};
    int2 rows[NA];
    const AgentTabs atabs{S.T->maxnbr_nib, S.T->tar_to_1, S.T->tar_to_11, S.T};
    agent_rows(policy, v, atabs, S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, S.episode[e], player, true, ((S.env[e] >> 8) & 3u) == 0u,
               S.agent_cycle + ai, S.agent_swarm + ai, S.agent_dfs + ai, rows);
    int2* out = reinterpret_cast<int2*>(actions) + ((size_t)e * 2 + player) * NA;
#pragma unroll
    for (int i = 0; i < NA; ++i) out[i] = rows[i];
}

__global__ void evg_scripted_reset_kernel(DevState S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * S.N) return;
    S.agent_cycle[i] = 0x112u;             // first_turn = 1, group_num = 1, node_num = 2 (cycle_rush_turn25.py:49,56-57)
    S.agent_swarm[i] = 0xBA875421u;        // ATTACK_LIST = [1,2,4,5,7,8,10,11] (swarm_agent.py:29), nibble k = entry k
    S.agent_dfs[i] = 0u;                   // dfs_attack call counter
}

// ---------------------------------------------------------------------------------------------
// fog-of-war planes (SURVEY 8 f3): the `valid_nodes` mask of board_state (server.py:402-425) and the per-node knowledge
// levels of build_knowledge_output (server.py:779-832) -- both computed by the reference and never applied to the
// observation; exposed here as optional planes, plus the opposing-group sightings of :845-907.  One thread per (env, player);
// real node order.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) evg_fog_kernel(DevState S, uint8_t* fog, uint8_t* know, int8_t* sight) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * S.N) return;
    const int e = idx >> 1, p = idx & 1;
    const size_t N = (size_t)S.N;
    const DevTables* __restrict__ T = S.T;
    uint32_t ctrl = 0, towers = 0;         // nodes controlled by p; of those, the fully controlled OBSERVE nodes
    uint32_t seen_by_tower = 0;
#pragma unroll
    for (int n = 1; n <= NN; ++n) {
        const uint32_t nw = (S.node[(size_t)((n - 1) >> 1) * N + e] >> (16 * ((n - 1) & 1))) & 0xFFFFu;
        const int cb = (int)((nw >> 10) & 3u) - 1, cs = (int)(nw & 0x3FFu) - 512;
        const bool mine = cb == p, obs = (T->resource[n] & EVG_RES_OBSERVE) != 0;
        ctrl |= (mine ? 1u : 0u) << n;
        seen_by_tower |= (mine && obs) ? T->nbr_mask[n] : 0u;                                        // :415-418: the tower's OWN connections are revealed
        towers |= ((mine && obs && abs(cs) == T->control_points[n]) ? 1u : 0u) << n;
    }
    // server.py:794-804: node X has partial knowledge when one of X's connections leads to such a tower -- the edge X -> tower, not tower -> X.  The two are
    // the same set on DemoMap; a map with a one-way edge tells them apart (tests/golden/custom_varA.npz: 6 -> 5 only)
    uint32_t watch = 0;
#pragma unroll
    for (int x = 1; x <= NN; ++x) watch |= ((T->nbr_mask[x] & towers) ? 1u : 0u) << x;
    uint32_t idle = 0, incoming = 0;       // nodes with a listed non-moving group of p; nodes a group of p moves to from a neighbour
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const uint32_t w = S.grp[(size_t)(p * 12 + k) * N + e];
        const bool alive = (w & G_MASK_M) != 0, moving = ((w & G_MODE_M) >> G_MODE_S) == MODE_MOVING;
        const uint32_t loc = w & G_LOC_M, dest = (w & G_DEST_M) >> G_DEST_S;
        idle |= ((alive && !moving) ? 1u : 0u) << loc;                                                // :421-424, :784-787
        incoming |= ((alive && moving && ((T->nbr_mask[dest] >> loc) & 1u)) ? 1u : 0u) << dest;       // :806-812
    }
    const uint32_t valid = ctrl | seen_by_tower | idle;                                               // board_state :402-425
    const uint32_t full = ctrl | idle, partial = watch | incoming;                                    // build_knowledge_output :816-829
#pragma unroll
    for (int n = 1; n <= NN; ++n) {
        if (fog) fog[(size_t)idx * NN + n - 1] = (uint8_t)((valid >> n) & 1u);
        if (know) know[(size_t)idx * NN + n - 1] = (uint8_t)(((full >> n) & 1u) ? 2u : (((partial >> n) & 1u) ? 1u : 0u));
    }
    if (sight) {
        // opposing-group sightings `opp_k` (server.py:845-907): a listed opposing group is reported at its node when that node's
        // knowledge is 1 or 2 and it is either not moving (key -1) or headed for a node of knowledge > 0 (key = that node's
        // index in the node list, ID - 1, as the reference writes it): {seen, node, key, unit count} per opposing group
        const uint32_t known = full | partial;
        char4* out = reinterpret_cast<char4*>(sight) + (size_t)idx * NG;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const uint32_t w = S.grp[(size_t)((1 - p) * 12 + k) * N + e];
            const bool alive = (w & G_MASK_M) != 0, moving = ((w & G_MODE_M) >> G_MODE_S) == MODE_MOVING;
            const uint32_t loc = w & G_LOC_M, dest = (w & G_DEST_M) >> G_DEST_S;
            const bool seen = alive && ((known >> loc) & 1u) && (!moving || ((known >> dest) & 1u));
            out[k] = seen ? make_char4(1, (signed char)loc, (signed char)(moving ? (int)dest - 1 : -1), (signed char)__popc(w & G_MASK_M))
                          : make_char4(0, 0, 0, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 'smart state' preprocessing of agents/Smart_State/DQNAgent.py:200-300 (SURVEY 8 f4): obs[N][2][105] of one player
// -> features float32 [N][12][59] (the reference builds float64 and the network casts to float32: computed in f64,
// rounded once).
// ---------------------------------------------------------------------------------------------
// COMPACT (evg_smart_state_compact): the same values without their redundancy.  34 of the 59 features of a swarm are the same for all 12 swarms of an env and
// 12 more are the constant one-hot swarm id, so the 12 x 59 matrix is determined by `shared` [34] and `swarm` [12][13] = {one-hot node (11), average
// health x alive / 1000, in transit}: 760 B per env instead of 2 832.  (A consumer's first linear layer over the 59 inputs is W[:, :34] shared + W[:, 34:47]
// swarm
// + W[:, 47 + s]: the same numbers from a quarter of the bytes.)  With so little to write the kernel is no longer bound by bytes but by the ~200 instructions a
// wavefront spends per env (23 us at 65 536 envs against 40 for the full matrix).  A mapping of eight envs per wavefront with per-lane element descriptors was
// built
// and measured: 38 us -- every element then costs ~18 instructions (two LDS reads, the float64 product, selects) where the table costs one read; dropped.
template <typename OT, bool COMPACT = false>
__global__ void __launch_bounds__(256) evg_smart_state_kernel(int N, int player, int seat_only, const OT* obs, float* out, float* out_swarm) {
    // One wavefront per env and pass.  The 105-value observation row is staged in LDS once; every distinct output value of the
    // env goes into a small per-wave table -- the 34 features all swarms share and the 12 per-swarm health features are
    // one IEEE f64 division each (46 lanes: one division sequence per env instead of one per output element), then the
    // 12 in-transit flags, the constants 0 and 1 and the 12 x 11 one-hot node entries -- and the env's 12 x 59 floats
    // are streamed out as table[idx] in 16-byte-per-lane (1 KiB per wavefront) coalesced stores; idx depends only on the position in
    // the row and is computed once per lane.  HBM-bound by the 2 832 B written per env.  Every wavefront works on its own env with its own
    // LDS rows, so the phases are separated by wavefront-scope fences, not block barriers: a barrier would also wait (vmcnt(0)) for the
    // stores of the pass to be acknowledged before the next env's row is even requested.
    constexpr int F = 59, WPB = 4, NV = NG * F / 4, NIT = (NV + 63) / 64;          // 177 float4 per env: three per lane
    static_assert(NG * F % 4 == 0, "an env's features are a whole number of float4");
    constexpr int T_HP = 34, T_MOV = 46, T_ZERO = 58, T_ONE = 59, T_HOT = 64, T_SIZE = T_HOT + NG * NN;
    __shared__ int   row[WPB][128];
    __shared__ float tab[WPB][T_SIZE + 4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint8_t idx[NIT][4];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = 4 * (lane + 64 * i) + c, sw = j / F, f = j - sw * F;
            idx[i][c] = (uint8_t)(f < 34 ? f : (f < 45 ? T_HOT + sw * NN + (f - 34) : (f == 45 ? T_HP + sw : (f == 46 ? T_MOV + sw :
                                  (f - 47 == sw ? T_ONE : T_ZERO)))));
        }
    }
    if (lane == 0) { tab[w][T_ZERO] = 0.f; tab[w][T_ONE] = 1.f; }
    const int passes = (N + (int)gridDim.x * WPB - 1) / ((int)gridDim.x * WPB);
    for (int ps = 0; ps < passes; ++ps) {
        const long long e = ((long long)ps * gridDim.x + blockIdx.x) * WPB + w;
        const bool live = e < N;
        const OT* o = obs + (seat_only ? (size_t)(live ? e : 0) : (size_t)(live ? e : 0) * 2 + player) * OBS;     // seat_only: obs is [N][105]
        row[w][lane] = live ? (int)o[lane] : 0;                              // every observation value is an integer
        row[w][lane + 64] = (live && lane + 64 < OBS) ? (int)o[lane + 64] : 0;
        WAVE_SYNC();
        const int* r = row[w];
        // float32(n / d) of the reference's float64 quotient, taken as float32(n * (1 / d)): the float64 product differs from the quotient by an ulp of float64
        // at most, which never crosses a float32 rounding boundary for any numerator these features can have (turn 0..255, control -511..511, units 0..200,
        // groups 0..12, health x alive 0..1 663: checked exhaustively in tests/test_abi_and_host.py) -- one multiplication instead of a division sequence per
        // env
        double num = 0.0, rcp = 1.0;
        if (lane == 0) { num = (double)r[0]; rcp = 1.0 / 150.0; }                                    // :280
        else if (lane < 12) { num = (double)r[3 + 4 * (lane - 1)]; rcp = 1.0 / 100.0; }              // :282
        else if (lane < 23) { num = (double)r[4 + 4 * (lane - 12)]; rcp = 1.0 / 100.0; }             // :284
        else if (lane < 34) {                                                                       // :200-213, :286
            int cnt = 0;
#pragma unroll
            for (int k = 0; k < NG; ++k) cnt += (r[48 + 5 * k] == 0 && r[45 + 5 * k] - 1 == lane - 23) ? 1 : 0;
            num = (double)cnt; rcp = 1.0 / 12.0;
        } else if (lane < 46) {                                                                     // :294, swarm lane - 34
            const int sw = lane - 34;
            num = (double)(r[47 + 5 * sw] * r[49 + 5 * sw]); rcp = 1.0 / 1000.0;
        }
        if (lane < 46) tab[w][lane] = (float)(num * rcp);
        if (lane < NG) tab[w][T_MOV + lane] = (float)r[48 + 5 * lane];                                // :296
#pragma unroll
        for (int t = lane; t < NG * NN; t += 64) {                                                    // :288-292
            const int sw = t / NN, n = t - sw * NN;
            tab[w][T_HOT + t] = (r[45 + 5 * sw] == n + 1) ? 1.f : 0.f;
        }
        WAVE_SYNC();
        if constexpr (COMPACT) {
            constexpr int SF = 13, SV = NG * SF / 4;                                                  // 156 floats = 39 float4 per env
            static_assert(NG * SF % 4 == 0 && T_HP % 2 == 0, "whole vectors");
            if (live) {
                // shared [34]: 17 float2 (136 B per env: 8-byte aligned rows)
                if (lane < T_HP / 2)
                    reinterpret_cast<float2*>(out + (size_t)e * T_HP)[lane] = make_float2(tab[w][2 * lane], tab[w][2 * lane + 1]);
                if (lane < SV) {
                    float v[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int j = 4 * lane + c, sw = j / SF, f = j - sw * SF;
                        v[c] = tab[w][f < NN ? T_HOT + sw * NN + f : (f == NN ? T_HP + sw : T_MOV + sw)];
                    }
                    reinterpret_cast<float4*>(out_swarm + (size_t)e * NG * SF)[lane] = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        } else
        if (live) {
            float4* dst = reinterpret_cast<float4*>(out + (size_t)e * NG * F);                        // 2 832 B per env: 16-byte aligned rows
#pragma unroll
            for (int i = 0; i < NIT; ++i)
                if (lane + 64 * i < NV)                                                               // one-hot swarm id (:298) = the two constants
                    dst[lane + 64 * i] = make_float4(tab[w][idx[i][0]], tab[w][idx[i][1]], tab[w][idx[i][2]], tab[w][idx[i][3]]);
        }
        WAVE_SYNC();
    }
}

// ---------------------------------------------------------------------------------------------
// network output -> orders (SURVEY 8 f4, the other half): DQNAgent.get_best_actions (agents/Smart_State/DQNAgent.py:176-198) over
// get_all_swarm_decisions / swarm_think (:214-266), get_swarm_node_number (:302-310) and Move_Translation.get_move (Move_Translation.py:85-97).
// q [N][12][5] float32 is the policy network's output for every swarm (the network is the consumer's).  Every swarm reports its best direction
// (torch.argmax: the FIRST maximum), the node that direction leads to from where the observation says the swarm is, and its best Q; the
// decisions are sorted by best Q -- Python's sorted(): stable, ASCENDING -- and the FIRST seven become the 7 order rows: the reference acts with
// the seven swarms whose best Q is LOWEST (a quirk, pinned by tests/golden/smart_actions.npz).
// Mapping: one DPP row (16 lanes) per env, lane = swarm (12 active); a swarm's rank in the stable sort is the number of swarms that come before
// it, counted over the 15 rotations of the row (key and swarm id travel together, so nothing depends on the direction of the rotation).
// ---------------------------------------------------------------------------------------------
// (the rules themselves -- first maximum, get_move, the rank, the explore draws -- are smart_decode.inc's, shared with the step kernel's Q form)
//
// EXPLORE = true is DQNAgent.get_action (:130-146) as a whole: the epsilon coin `random.random() < self.epsilon`, then get_random_actions (:148-173) --
// swarms = np.random.choice(12, 7, replace=False), directions = np.random.choice(5, 7, replace=True), row i = [swarms[i], get_move(location of swarms[i],
// directions[i])] -- or the sort above.  The coin and the two choices are keyed draws of domain RNG_EXPLORE (oracle/rng_spec.py explore_draws: one agent
// call = (env id, episode, turn = obs[0], seat)).  They are per ENV, the rows per swarm: workgroups of 1 024 threads = 64 envs, whose first wavefront
// draws -- lane = env: two Philox blocks, the coin, the 7-of-12 permutation -- and leaves two words per env in LDS (explore flag | 7 x 3-bit directions;
// 7 swarm nibbles); behind one barrier swarm s looks its own row index up.  (All 16 lanes of a row drawing for themselves cost 5 us more per call at
// 65 536 envs: 16 times the Philox work.)  eps_env (may be NULL) overrides the scalar epsilon per env.
struct ExploreArgs {
    uint32_t seed_lo, seed_hi, env_id_base;
    const uint32_t* episode;     // DevState::episode
    int seat;                    // the agent's player number: part of the key of its draws
    float eps;
    const float* eps_env;        // [N] or NULL
    uint8_t* explored;           // [N] or NULL: 1 where the random branch ran
};
template <typename OT, bool EXPLORE>
__global__ void __launch_bounds__(EXPLORE ? 1024 : 256) evg_smart_actions_kernel(int N, int player, int seat_only, const OT* __restrict__ obs, const float* __restrict__ q,
                                                                int2* __restrict__ actions, int2* __restrict__ directions, ExploreArgs X) {
    constexpr int BLOCK = EXPLORE ? 1024 : 256;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int e = t >> 4, s = t & 15;
    const bool act = e < N && s < NG;
    [[maybe_unused]] __shared__ uint32_t draws[EXPLORE ? BLOCK / 16 : 1][2];
    if constexpr (EXPLORE) {
        const int ed = blockIdx.x * (BLOCK / 16) + (int)threadIdx.x;             // the first wavefront: lane = env of this workgroup
        if (threadIdx.x < BLOCK / 16 && ed < N) {
            const OT* o = obs + (seat_only ? (size_t)ed : (size_t)ed * 2 + player) * OBS;
            const int turn = (int)o[0];
            const uint32_t env_id = X.env_id_base + (uint32_t)ed, episode = X.episode[ed];
            const uint4 b0 = rng_block(X.seed_lo, X.seed_hi, env_id, episode, RNG_EXPLORE, 0u, turn, 0, X.seat, 0);
            const uint4 b1 = rng_block(X.seed_lo, X.seed_hi, env_id, episode, RNG_EXPLORE, 1u, turn, 0, X.seat, 0);
            const uint2 d = smart_explore_words(b0, b1, X.eps_env ? X.eps_env[ed] : X.eps);
            if (X.explored) X.explored[ed] = (d.x >> 31) ? 1 : 0;
            draws[threadIdx.x][0] = d.x;
            draws[threadIdx.x][1] = d.y;
        }
        __syncthreads();
    }
    float key = __int_as_float(0x7F800000);              // idle lanes: +inf with ids 12..15, never in front of a swarm
    int dir = 0, node = 0;
    [[maybe_unused]] int loc_mine = 0;
    if (act) {
        const float* qs = q + ((size_t)e * NG + s) * 5;
        float v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = qs[k];
        key = smart_best(v, dir);
        const OT* o = obs + (seat_only ? (size_t)e : (size_t)e * 2 + player) * OBS;
        const int loc = (int)o[45 + 5 * s];                 // get_swarm_node_number (+ 1): the swarm's node in the player's own numbering
        node = smart_move(loc, dir);
        loc_mine = loc;
    }
    int rank = smart_rank(key, s);
    if constexpr (EXPLORE) {
        const uint2 d = make_uint2(draws[threadIdx.x >> 4][0], draws[threadIdx.x >> 4][1]);
        if (e < N && (d.x >> 31)) {                                                           // get_random_actions (:148-173)
            rank = smart_explore_rank(d, s, dir);                                             // NA: not among the seven swarms drawn
            node = smart_move(loc_mine, dir);                                                 // get_move(get_swarm_node_number, direction) (:162-163)
        }
    }
    if (act && rank < NA) {                                 // sorted_swarm_decisions[:7] (:195-196) / final_action_array (:166-171)
        actions[(size_t)e * NA + rank] = make_int2(s, node);
        if (directions) directions[(size_t)e * NA + rank] = make_int2(s, dir);
    }
}

// ---------------------------------------------------------------------------------------------
// The Minimized agent's network output -> orders: DQNAgent.get_action of agents/Minimized/DQNAgent.py:121-242 (evg_minimized_get_action).  q [N][12][11]
// float32 is the policy network's output for every swarm, one Q per node; the rules are minimized_decode.inc's, the mapping evg_smart_actions_kernel's: one
// DPP row (16 lanes) per env, lane = swarm, and -- EXPLORE -- the first wavefront of a 1 024-thread workgroup draws for the workgroup's 64 envs.  The
// agent reads no observation: the turn that keys its draws is the handle's (what obs[0] of the env shows).  EXPLORE = false is get_best_actions alone.
// ---------------------------------------------------------------------------------------------
template <bool EXPLORE>
__global__ void __launch_bounds__(EXPLORE ? 1024 : 256) evg_minimized_actions_kernel(int N, const uint32_t* __restrict__ envw, const float* __restrict__ q,
                                                                                    int2* __restrict__ actions, ExploreArgs X) {
    constexpr int BLOCK = EXPLORE ? 1024 : 256;
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int e = t >> 4, s = t & 15;
    [[maybe_unused]] __shared__ uint32_t draws[EXPLORE ? BLOCK / 16 : 1][2];
    uint2 d = make_uint2(0u, 0u);
    if constexpr (EXPLORE) {
        const int ed = blockIdx.x * (BLOCK / 16) + (int)threadIdx.x;             // the first wavefront: lane = env of this workgroup
        if (threadIdx.x < BLOCK / 16 && ed < N) {
            const int turn = (int)(envw[ed] & 0xFFu);
            const uint32_t env_id = X.env_id_base + (uint32_t)ed, episode = X.episode[ed];
            const uint4 b0 = rng_block(X.seed_lo, X.seed_hi, env_id, episode, RNG_EXPLORE, 0u, turn, 0, X.seat, 0);
            const uint4 b1 = rng_block(X.seed_lo, X.seed_hi, env_id, episode, RNG_EXPLORE, 1u, turn, 0, X.seat, 0);
            const uint2 w = minimized_explore_words(b0, b1, X.eps_env ? X.eps_env[ed] : X.eps);
            if (X.explored) X.explored[ed] = (w.x >> 31) ? 1 : 0;
            draws[threadIdx.x][0] = w.x;
            draws[threadIdx.x][1] = w.y;
        }
        __syncthreads();
        d = make_uint2(draws[threadIdx.x >> 4][0], draws[threadIdx.x >> 4][1]);
    } else {
        if (X.explored && s == 0 && e < N) X.explored[e] = 0;
    }
    const bool act = e < N && s < NG;
    int node;
    const int rank = minimized_decide(q + (size_t)(e < N ? e : 0) * (NG * MIN_Q), act, e < N, s, d, node);
    if (act && rank < NA) actions[(size_t)e * NA + rank] = make_int2(s, node);
}
