// step_kernel_body.inc -- the body of the step kernel: a textual fragment of evg_step_kernel, evg_step_minimized_kernel and evg_step_minimized2_kernel
// (step_kernel.inc, which documents the forms), compiled with the names OT, LPW, MULTI, MT, CHUNKED, SEAT, WPB, QDEC, LEAGUE and HEAD in scope.
    static_assert(HEAD == HEAD_SMART || QDEC, "the 11-way head exists in the Q forms only (one seat or two)");
    static_assert(!MT || (!MULTI && LPW == WG), "the stock-entropy mode exists in the single-turn, 32-envs-per-wave form only");
    static_assert(!CHUNKED || (MULTI && LPW == WG && !MT), "the chunked form is an instantiation of the persistent two-lane kernel");
    static_assert(!SEAT || (!MULTI && !MT && LPW == WG), "the one-seat form is an instantiation of the single-turn two-lane kernel");
    static_assert(WPB == 1 || (!MULTI && !MT && !CHUNKED && !SEAT && LPW == WG), "several wavefronts per workgroup: the plain single-turn two-lane form only");
    static_assert(!QDEC || (!MULTI && !MT && LPW == WG && WPB == 1), "the Q form is an instantiation of the single-turn two-lane kernel (one seat or two)");
    static_assert(!LEAGUE || SEAT || (QDEC && HEAD == HEAD_MINIMIZED),
                  "the league forms are instantiations of the one-seat kernel (with or without the Q decode) or of the two-seat 11-way Q form");
    // the two-seat 11-way forms decode their orders or take them from the league's bots: io.gen_actions is 0 or 2 there, never 1 (orders drawn in the
    // kernel), and the tests for 1 -- a wave-wide condition the compiler otherwise keeps in scalar registers across the turn -- are compiled out
    constexpr bool DRAWS_ORDERS = !(QDEC && !SEAT && HEAD == HEAD_MINIMIZED);
    step_args_ptr A = (step_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int EPW = LPW / 2;                        // envs per wavefront
    constexpr int DP_CAP = CombatLds<LPW>::DP_CAP;
    // 8 wavefronts per CU (2 per SIMD) keep a whole 65 536-env batch resident: 160 KiB / 8 = 20 480 B each
    static_assert(sizeof(StepLds<LPW>) <= 20480, "step kernel LDS exceeds the 8-wavefronts-per-CU budget");
    __shared__ StepLds<LPW> Ls[WPB];
    const int wv = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WG));     // this wavefront's slice (wave-uniform)
    StepLds<LPW>& L = Ls[wv];
    const int lane = WPB == 1 ? (int)threadIdx.x : (int)(threadIdx.x % WG);
    const bool envlane = LPW == WG || lane < LPW;       // owns an env side; helper lanes only join the balanced phases
    const int E = envlane ? lane >> 1 : 0, P = lane & 1;
    // Which envs, which turns.  Plain launch: workgroup b plays all `turns` turns of envs env_lo + 32 b ...
    // CHUNKED launch (io.nsets > 0: a persistent rollout of more envs than the device holds at once, plan_step): the grid is as many
    // workgroups as the device holds; the rollout is cut into UNITS = (set of 32 envs) x (chunk of chunk_turns consecutive turns), and
    // every workgroup takes units from a queue until it is empty, handing a set on to whoever takes its next chunk through HBM
    // (DevState::progress).  Every wave slot holds useful work until the queue runs dry, where one launch of ceil(N / 32) whole-rollout
    // workgroups left its last, partial round running alone at low occupancy for a whole launch (98 304 envs: 30.9 us per turn).
    // Sets are OWNED BY AN XCD (set s belongs to XCD s mod nxcd; one queue per XCD, chunk-major; a workgroup serves the queue of the
    // XCD it runs on, read from XCC_ID): the hand-over then stays inside one L2 and needs no L2 write-back / invalidate (an agent-scope
    // release per chunk made this form 57 % SLOWER than the plain launch: 2 048 waves x buffer_wbl2 keep every L2 walking), only the
    // store drain of the producer and the L1 invalidate of the consumer.  Nothing depends on dispatch order or on how the dispatcher
    // places workgroups: a unit's predecessor was taken from the same queue earlier, by a workgroup that is running and waits for
    // nothing taken later -- no cycle; every workgroup leaves when its queue is empty.
    constexpr int QUEUE_STRIDE = 64;                           // words between the XCDs' queue counters (256 B)
    constexpr bool CHUNKABLE = CHUNKED;                        // an instantiation of its own: the plain persistent kernel carries no unit loop
    int q_xi = 0, q_nx = 0, q_units = 0;
    if (CHUNKABLE && io.nsets > 0) {
        const uint32_t xcc = __builtin_amdgcn_s_getreg(63508) & 15u;                  // HW_REG_XCC_ID
        // rank of this XCD among the device's (evg_create probes them); 15 = unknown
        q_xi = (int)((S.xcd_rank >> (4u * xcc)) & 15ull);
        if (q_xi < S.nxcd) {
            q_nx = (io.nsets - q_xi + S.nxcd - 1) / S.nxcd;                           // sets q_xi, q_xi + nxcd, ... are this XCD's
            q_units = q_nx * ((io.turns + io.chunk_turns - 1) / io.chunk_turns);
        } else if (threadIdx.x == 0) {
            raise_fault(S.fault, S.fault_seen, 2u);                                   // a workgroup on an XCD the probe did not see: never expected
        }
    }
    STAMP_WAVE_BEGIN();
    for (;;) {                                           // one pass per unit (exactly one pass in a plain launch)
    int wg_set = (int)blockIdx.x * WPB + wv, wg_chunk = 0;
    // a wavefront beyond the last set of a partial last workgroup (no barrier anywhere: it may leave)
    if (WPB > 1 && io.env_lo + wg_set * EPW >= io.env_hi) return;
    if (CHUNKABLE && io.nsets > 0) {
        int q = 0;
        if (threadIdx.x == 0) q = (int)atomicAdd(S.queue + q_xi * QUEUE_STRIDE, 1u);        // every XCD's counter on a line of its own
        q = __builtin_amdgcn_readfirstlane(q);
        if (q >= q_units) break;
        wg_chunk = q / q_nx;
        wg_set = (q - wg_chunk * q_nx) * S.nxcd + q_xi;
    }
    const int e0 = io.env_lo + wg_set * EPW;          // this launch plays envs [env_lo, env_hi) of the handle (launch_step)
    int nvalid_ = min(EPW, io.env_hi - e0);
    // (two-seat league form: opaque, so that `nvalid == EPW` at the turn's end is a test of this register -- the compiler otherwise tests env_hi - e0, keeps
    // that in a scalar register of its own across the whole turn and, in that form alone, spills it)
    if constexpr (LEAGUE && !SEAT) asm volatile("" : "+s"(nvalid_));
    const int nvalid = nvalid_;
    const bool valid = envlane && E < nvalid;
    const int e = valid ? e0 + E : e0;
    const size_t N = (size_t)S.N;
    const DevTables* T = S.T;

    STAMP(0);
    if (CHUNKABLE && wg_chunk > 0) {
        // wait for the set's previous chunk (relaxed polls that bypass the L1), then ONE agent-scope acquire: it invalidates this CU's L1,
        // which may still hold lines of this set from an earlier chunk.  The wait is bounded IN TIME (s_memrealtime: a constant 100 MHz
        // counter, so the bound does not depend on the shader clock or on how long a poll takes): a predecessor chunk is ~0.4 ms of work, a
        // wave that has waited 5 s gives up, flags the handle (fault word: every path on which results leave the handle reports it, the pack
        // kernel poisons its rows) and goes on, so the grid always drains.
        const uint32_t* flag = S.progress + (e0 >> 5);
        const uint32_t want = io.progress_base + (uint32_t)wg_chunk;
        constexpr unsigned long long kGiveUpTicks = 500000000ull;     // 5 s at 100 MHz
        unsigned long long t_wait0 = 0;
        bool waiting = false;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (!waiting) { waiting = true; t_wait0 = now; }
            if (now - t_wait0 > kGiveUpTicks) {
                if (threadIdx.x == 0) raise_fault(S.fault, S.fault_seen, 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(16);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
#ifdef EVG_DIAG      // experiment knobs (tools/stagger.py): delay = slot x a + simd x b sleeps of 64 cycles, a = ablate[15:8] - 1, b = ablate[23:16]
    const int kStaggerSlot = (A->io_.ablate >> 8) & 0xFFu ? (int)((A->io_.ablate >> 8) & 0xFFu) - 1 : 67, kStaggerSimd = (int)((A->io_.ablate >> 16) & 0xFFu);
#else
    constexpr int kStaggerSlot = 67, kStaggerSimd = 0;
                                                            // x 64 cycles (s_sleep 1).  Round-4 sweep of the final kernel
                                                            // (profiles/r04_f_stagger_single_turn.txt): a plateau from
                                                            // 59 to 75 x 64 cycles (26.8 us per launch), 27.5 at round 3's 84, 27.8-29.5 below 55 and above
                                                            // 100, 28.9 without

#endif
    // ---- prologue loads: the constant tables (one blob, already in its LDS layout) and this lane's state (env fastest; the two player rows of a group index
    // interleave
    // across lanes).  Every load is issued before the first LDS store, so the launch pays ONE memory round trip here
    // instead of one per table and one for the state.
    constexpr int TV = (int)(sizeof(LdsTables) / 16);   // 77 16-byte pieces: two loads per lane
    static_assert(TV > WG && TV <= 2 * WG, "table blob is copied in two rounds");
    const uint4* timg = reinterpret_cast<const uint4*>(&T->lds);
    const uint4 tv0 = timg[lane], tv1 = timg[lane + WG < TV ? lane + WG : 0];
    const uint32_t envw = S.env[e];
    uint32_t episode = S.episode[e];
    float ep_ret = S.ep_ret[(size_t)P * N + e];         // this player's running episode return: a register across the launch's turns
    uint32_t st[3], g_in[12], n_in[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) st[j] = S.stamp[(size_t)(P * 3 + j) * N + e];
#pragma unroll
    for (int k = 0; k < 12; ++k) g_in[k] = S.grp[(size_t)(P * 12 + k) * N + e];
#pragma unroll
    for (int j = 0; j < 3; ++j) n_in[j] = S.node[(size_t)(P * 3 + j) * N + e];   // player 0 lane: nodes 1..6, player 1 lane: nodes 7..11 (two per word)
    // fused scripted agents: this seat's agent object (three words) lives in registers across the launch's turns
    uint32_t ag_cycle = 0, ag_swarm = 0, ag_dfs = 0;
    const size_t ai = (size_t)P * N + e;
    if (io.gen_actions == 2) { ag_cycle = S.agent_cycle[ai]; ag_swarm = S.agent_swarm[ai]; ag_dfs = S.agent_dfs[ai]; }
    // league forms: the member this env plays (both lanes of the pair hold it: player 0's lane tallies, the league seat's lane plays and swaps)
    [[maybe_unused]] uint32_t lg_raw = 0u;
    if constexpr (LEAGUE) lg_raw = io.lg_assign[e];
    // caller-supplied orders (evg_step): this player's 7 rows are part of the same round trip
    int2 act_in[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) act_in[i] = make_int2(0, 0);
    if constexpr (SEAT && !QDEC) {                      // the caller's seat: [N][7][2], or its rows of a [N][2][7][2] tensor
        if (io.actions && P == io.seat) {
            const int2* ap = reinterpret_cast<const int2*>(io.actions) + (io.actions_both ? ((size_t)e * 2 + P) * NA : (size_t)e * NA);
#pragma unroll
            for (int i = 0; i < NA; ++i) act_in[i] = ap[i];
        }
    } else if (!MULTI && !SEAT && !QDEC && !io.gen_actions && io.actions) {
        const int2* ap = reinterpret_cast<const int2*>(io.actions) + ((size_t)e * 2 + P) * NA;
#pragma unroll
        for (int i = 0; i < NA; ++i) act_in[i] = ap[i];
    }
    // Q form: the caller's network output for the wave's envs -- 240 contiguous bytes each, 16 bytes per lane -- and its epsilon are part of the same round trip
    // (two-seat form: both seats' values, each seat's in pieces of its own; the lane's epsilon is its own seat's)
    constexpr int QSEATS = SEAT ? 1 : 2;                                       // seats whose rows the Q form decodes
    constexpr int QV = QDEC && HEAD == HEAD_SMART ? (EPW * NG * 5 / 4 + WG - 1) / WG : 1;   // 16-byte pieces per lane and seat (480 per wave: 8)
    [[maybe_unused]] uint4 qv[QSEATS][QV];
    [[maybe_unused]] float eps_q = 0.f;
    [[maybe_unused]] uint2 qdraw = make_uint2(0u, 0u);
    if constexpr (QDEC) {
        static_assert(NG * 5 % 4 == 0, "an env's Q values are a whole number of 16-byte pieces");
        [[maybe_unused]] const int nq = nvalid * (NG * 5 / 4);
        if constexpr (HEAD == HEAD_MINIMIZED) {                                // (the 11-way head's values are read by the decode itself)
            if constexpr (SEAT) eps_q = io.eps_env ? io.eps_env[e] : io.eps;
            else eps_q = io.eps_env ? io.eps_env[(size_t)e * 2 + P] : (P ? io.eps1 : io.eps);
        } else if constexpr (SEAT) {
            const uint4* qs = reinterpret_cast<const uint4*>(io.q) + (size_t)e0 * (NG * 5 / 4);      // 16-byte aligned (checked by the entry point)
#pragma unroll
            for (int i = 0; i < QV; ++i) {
                const int v = lane + WG * i;
                qv[0][i] = v < nq ? qs[v] : make_uint4(0u, 0u, 0u, 0u);
            }
            eps_q = io.eps_env ? io.eps_env[e] : io.eps;
        } else {
            // [N][2][12][5]: piece v of seat s is piece v % 15 of env v / 15's row s -- 240-byte runs 480 bytes apart
            const uint4* qs = reinterpret_cast<const uint4*>(io.q) + (size_t)e0 * (2 * NG * 5 / 4);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int i = 0; i < QV; ++i) {
                    const int v = lane + WG * i, ev = v / (NG * 5 / 4);
                    qv[s][i] = v < nq ? qs[(2 * ev + s) * (NG * 5 / 4) + v - ev * (NG * 5 / 4)] : make_uint4(0u, 0u, 0u, 0u);
                }
            }
            eps_q = io.eps_env ? io.eps_env[(size_t)e * 2 + P] : (P ? io.eps1 : io.eps);
        }
    }
    int turn = (int)(envw & 0xFFu);
    int status = (int)((envw >> 8) & 3u);
    if constexpr (CHUNKABLE) {
        // The words just loaded must be the ones the previous chunk's lane stored -- its LATEST, not an older copy left in a cache by a hand-over that did
        // not do what it relies on (see "what this relies on" at the publish below).  The producer handed on a checksum over (chunk number, every state word
        // of the lane); recomputed here over the loaded words.  A mismatch is fault bit 3: sticky, reported wherever results leave the handle.
        if (wg_chunk > 0 && valid) {
            const uint32_t seq = io.progress_base + (uint32_t)wg_chunk;
            uint32_t hsum = handoff_sum(seq, g_in, st, n_in, envw & 0x3FFu, episode, __float_as_uint(ep_ret));
            if (io.gen_actions == 2) hsum = handoff_mix(handoff_mix(handoff_mix(hsum, ag_cycle), ag_swarm), ag_dfs);
            if (hsum != S.handoff[(size_t)P * N + e]) raise_fault(S.fault, S.fault_seen, 8u);
        }
    }
    if constexpr (!MULTI) {
        // Single-turn launches: all 2 048 wavefronts start together and every SIMD's two waves would run the same phases in
        // lockstep, competing for the same issue slots phase by phase.  The wave in hardware slot 1 therefore waits STAGGER
        // cycles here, with its loads already in flight (tools/stagger.py: 35.0 -> 32.6 us per launch at 65 536 envs) ...
        {
            const uint32_t hw = __builtin_amdgcn_s_getreg(12292);                  // HW_ID[6:0]: wave_id (the wave's slot on its SIMD) [3:0], simd_id [5:4]
            // (only while the whole grid is resident at once -- STEP_F_STAGGER, set by launch_step from the device's capacity: up to
            // 2 048 workgroups = 65 536 envs on a whole MI355X; a larger grid queues behind itself and its waves start at different times anyway)
            const int nsleep = (io.flags & STEP_F_STAGGER) ? (int)(hw & 1u) * kStaggerSlot + (int)((hw >> 4) & 3u) * kStaggerSimd : 0;
            for (int i = 0; i < nsleep; ++i) __builtin_amdgcn_s_sleep(1);
            // (issue priority for either wave of the pair makes a single-turn launch no shorter: for the late wave 32.5 -> 38.0 us,
            // for the early wave no change; A/B on one box)
        }
        // ... and the orders this kernel draws itself need only the turn and the episode (the first two loads), so they are
        // drawn while the group / node words are still on their way
        if (DRAWS_ORDERS && io.gen_actions == 1) gen_random_rows(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, turn, P, act_in);
        if constexpr (QDEC) {
            // the caller's agent call draws two Philox blocks (smart_decode.inc): each lane of the pair draws one -- block P -- and the pair swaps them
            // (DPP), so that both lanes hold the env's coin and draws, no lane idles behind its partner
            // (two-seat form: each lane is its own seat's agent -- key seat P -- and draws both of its blocks; the seats' calls are independent)
            if constexpr (SEAT) {
                const uint4 b = rng_block(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, RNG_EXPLORE, (uint32_t)P, turn, 0, io.seat, 0);
                const uint4 o = make_uint4((uint32_t)xchg1((int)b.x), (uint32_t)xchg1((int)b.y), (uint32_t)xchg1((int)b.z), (uint32_t)xchg1((int)b.w));
                if constexpr (HEAD == HEAD_MINIMIZED) qdraw = minimized_explore_words(P ? o : b, P ? b : o, eps_q);
                else qdraw = smart_explore_words(P ? o : b, P ? b : o, eps_q);
            } else {
                const uint4 b0 = rng_block(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, RNG_EXPLORE, 0u, turn, 0, P, 0);
                const uint4 b1 = rng_block(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, RNG_EXPLORE, 1u, turn, 0, P, 0);
                if constexpr (HEAD == HEAD_MINIMIZED) qdraw = minimized_explore_words(b0, b1, eps_q);
                else qdraw = smart_explore_words(b0, b1, eps_q);
            }
        }
    }
    {
        uint4* lt = reinterpret_cast<uint4*>(&L.tab);
        lt[lane] = tv0;
        if (lane + WG < TV) lt[lane + WG] = tv1;
    }
    if (envlane) {
#pragma unroll
        for (int k = 0; k < 12; ++k) L.G[k][lane] = g_in[k];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int n = P ? 7 + j : 1 + j;
            if (n <= NN) L.NW[n][E] = (n_in[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        }
    }
    // (Q form: the values of the first seat decoded -- the caller's, or seat 0's -- and the agent calls' draws, held by the lanes of that seat)
    auto stage_q = [&](int s) {
        if constexpr (HEAD == HEAD_SMART) {
            uint4* ql = reinterpret_cast<uint4*>(&L.u.sq.q[0][0]);
#pragma unroll
            for (int i = 0; i < QV; ++i)
                if (lane + WG * i < EPW * NG * 5 / 4) ql[lane + WG * i] = qv[s][i];
        }
        if (P == s) L.u.sq.draws[E] = qdraw;
    };
    if constexpr (QDEC) stage_q(0);
    WAVE_SYNC();
    // Every prologue load is waited for here, before the turn loop: a register whose load may still be in flight on SOME path
    // makes the compiler put s_waitcnt vmcnt(0) in front of its first use inside the loop, where it would wait for the previous
    // turn's observation stores on every turn.
    asm volatile("" :: "v"(episode), "v"(ep_ret), "v"(ag_cycle), "v"(ag_swarm), "v"(ag_dfs));
    [[maybe_unused]] int lg_m = 0, lg_pol = 0;
    if constexpr (LEAGUE) {
        asm volatile("" :: "v"(lg_raw));
        // a value >= M (only a caller's own write can be one) plays member 0 and is reported
        if (lg_raw >= (uint32_t)io.lg_num) {
            if (valid && P != io.seat) atomicOr(io.lg_ctl, (unsigned long long)EVG_LEAGUE_S_BAD_ASSIGN);
            lg_raw = 0u;
        }
        lg_m = (int)lg_raw;
        lg_pol = (int)((io.lg_members >> (4u * lg_raw)) & 15ull);
    }
    if constexpr (QDEC) {
        // ---- Q form: the caller's 7 rows from its network output (DQNAgent.get_action, agents/Smart_State/DQNAgent.py:130-198), the whole wavefront at
        // once -- one DPP row (16 lanes) per env, lane = swarm, four envs per pass -- with the rules of evg_smart_actions_kernel (smart_decode.inc).  The
        // swarm's location is its group word's (the state this launch starts from is what the previous launch's observation shows: with auto_reset a
        // finished env's observation is the first of its next episode), in the caller's own numbering: what obs[45 + 5 s] holds.  Rows of every valid env
        // are decoded and written out, frozen ones included, as evg_smart_get_action writes every env.
        // (two-seat form: seat 0, then seat 1, each with its own numbering and its own draws)
        const int sw = lane & 15, sub = lane >> 4;
        // two-seat league form: the envs whose league seat the NETWORK plays (member io.lg_qmember), bit 2 E; the league seat's pass decodes those only
        [[maybe_unused]] uint64_t lg_qenvs = 0;
        if constexpr (LEAGUE && !SEAT) lg_qenvs = __ballot(P == 0 && lg_m == io.lg_qmember);
        auto decode = [&](int seat) {
            if constexpr (HEAD == HEAD_MINIMIZED) {
                // the 11-way head: {swarm, argmax + 1}, no location, no directions; envs beyond the launch's last read nothing
                for (int ps = 0; ps < EPW / 4; ++ps) {
                    const int ep = 4 * ps + sub;          // env slot of this lane's row
                    bool live = ep < nvalid;
                    if constexpr (LEAGUE && !SEAT) live = live && (seat == io.seat || ((lg_qenvs >> (2 * ep)) & 1ull));
                    const bool act = sw < NG && live;
                    int node;
                    // (two-seat form: seat p's [12][11] block of env e is block 2 e + p)
                    const size_t qblock = SEAT ? (size_t)(e0 + (live ? ep : 0)) : (size_t)(e0 + (live ? ep : 0)) * 2 + (size_t)seat;
                    const int rank = minimized_decide(io.q + qblock * (NG * MIN_Q), act, live, sw, L.u.sq.draws[ep], node);
                    if (act && rank < NA) L.u.sq.rows[ep][rank] = make_int2(sw, node);
                }
            } else {
                const uint64_t own_q = player_node_map(seat, L.tab.nib[0]);
                for (int ps = 0; ps < EPW / 4; ++ps) {
                    const int ep = 4 * ps + sub;              // env slot of this lane's row
                    const bool act = sw < NG && ep < nvalid;
                    float key = __int_as_float(0x7F800000);  // idle lanes: +inf with ids 12..15, never in front of a swarm
                    int dir = 0, node = 0, loc = 0;
                    if (act) {
                        float v[5];
#pragma unroll
                        for (int k = 0; k < 5; ++k) v[k] = L.u.sq.q[ep][5 * sw + k];
                        key = smart_best(v, dir);
                        loc = (int)map_node(own_q, L.G[sw][2 * ep + seat] & G_LOC_M);
                        node = smart_move(loc, dir);
                    }
                    int rank = smart_rank(key, sw);
                    const uint2 d = L.u.sq.draws[ep];
                    if (ep < nvalid && (d.x >> 31)) {        // get_random_actions
                        rank = smart_explore_rank(d, sw, dir);
                        node = smart_move(loc, dir);
                    }
                    if (act && rank < NA) {
                        L.u.sq.rows[ep][rank] = make_int2(sw, node);
                        L.u.sq.dirs[ep][rank] = make_int2(sw, dir);
                    }
                }
            }
            WAVE_SYNC();
        };
        if constexpr (!SEAT) {
            // rows [N][2][7][2]: a seat's 56 bytes per env, 112 bytes apart, stored 8 bytes per lane
            auto put_rows2 = [&](int32_t* out, const int2* src, int s) {
                int2* dst = reinterpret_cast<int2*>(out) + (size_t)e0 * 2 * NA;
                for (int v = lane; v < nvalid * NA; v += WG) {
                    const int ev = v / NA;
                    dst[(2 * ev + s) * NA + v - ev * NA] = src[v];
                }
            };
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s == 1) {
                    stage_q(1);
                    WAVE_SYNC();
                }
                decode(s);
                if (P == s) {
#pragma unroll
                    for (int i = 0; i < NA; ++i) act_in[i] = L.u.sq.rows[E][i];
                }
                // (two-seat league form: the rows PLAYED leave through io.actions_out in step_orders.inc -- the league seat's may be a bot's)
                if (io.q_actions) put_rows2(io.q_actions, &L.u.sq.rows[0][0], s);
                if constexpr (HEAD == HEAD_SMART)
                    if (io.q_directions) put_rows2(io.q_directions, &L.u.sq.dirs[0][0], s);
                WAVE_SYNC();                              // the next seat's values, then the turn's scratch, replace this seat's rows
            }
            if constexpr (LEAGUE) {                       // 2: the league seat of an env whose member is a bot -- not a transition of the second network
                if (valid && io.q_explored) io.q_explored[(size_t)e * 2 + P] = (P != io.seat && lg_m != io.lg_qmember) ? (uint8_t)2 : (uint8_t)(qdraw.x >> 31);
            } else {
                if (valid && io.q_explored) io.q_explored[(size_t)e * 2 + P] = (uint8_t)(qdraw.x >> 31);
            }
        } else {
            decode(io.seat);
            if (P == io.seat) {
#pragma unroll
                for (int i = 0; i < NA; ++i) act_in[i] = L.u.sq.rows[E][i];
            }
            if (valid && P == 0 && io.q_explored) io.q_explored[e] = (uint8_t)(qdraw.x >> 31);
            // rows played and directions: the wave's rows are contiguous in [N][7][2] (e0 * 56 bytes: 16-byte aligned), stored 16 bytes per lane
            auto put_rows = [&](int32_t* out, const int2* src) {
                int2* dst = reinterpret_cast<int2*>(out) + (size_t)e0 * NA;
                if (nvalid == EPW) {
#pragma unroll
                    for (int i = 0; i < (EPW * NA / 2 + WG - 1) / WG; ++i) {
                        const int v = lane + WG * i;
                        if (v < EPW * NA / 2) reinterpret_cast<uint4*>(dst)[v] = reinterpret_cast<const uint4*>(src)[v];
                    }
                } else {
                    for (int v = lane; v < nvalid * NA; v += WG) dst[v] = src[v];      // last, partial workgroup of the grid
                }
            };
            if (io.q_actions) put_rows(io.q_actions, &L.u.sq.rows[0][0]);
            if constexpr (HEAD == HEAD_SMART)
                if (io.q_directions) put_rows(io.q_directions, &L.u.sq.dirs[0][0]);
            WAVE_SYNC();                                  // the union is the turn's scratch from here on
        }
    }
    const bool observe_only = io.observe_only != 0;
    // stock-entropy mode: the env's MT19937 is advanced by the lane of player 0, in the reference's draw order
    MtGen mt{nullptr, 0, 0};
    const bool mt_lane = MT && valid && P == 0;
    if (MT && mt_lane) { mt.key = S.mt_key + e; mt.stride = N; mt.pos = S.mt_pos[e]; }

    // One iteration = one turn.  evg_step runs exactly one; the fused rollout driver lets every wavefront play
    // `turns` consecutive turns of its envs with the state resident in LDS/registers: outputs are still written every
    // turn, but no wave waits for the slowest wave of the grid between turns, and nothing is re-loaded.
    // (chunked launch: this workgroup's chunk_turns turns, the launch's last chunk what is left of io.turns)
    // the single-turn instantiation has no loop at all
    const int nturns = MULTI ? ((CHUNKABLE && io.nsets > 0) ? min(io.chunk_turns, io.turns - wg_chunk * io.chunk_turns) : io.turns) : 1;
    for (int iter = 0; iter < nturns; ++iter) {
    // Multi-turn form: the argument pointer and the lane id are made opaque once per turn, so that argument fields, table
    // entries and per-lane address arithmetic are recomputed next to their uses instead of being hoisted out of the loop
    // and kept live across it (which overflowed the register file).  The declarations below shadow the prologue's.
    int lane_ = WPB == 1 ? (int)threadIdx.x : (int)(threadIdx.x % WG);
    if (MULTI) { asm volatile("" : "+s"(A)); asm volatile("" : "+v"(lane_)); T = S.T; }
    const int lane = lane_;
    if constexpr (MULTI) {
        // The two waves of a SIMD share its issue slots; the arbiter goes by priority, then by age.  With equal priorities the older
        // wave (hardware slot 0) is favoured throughout: it finishes a 150-turn launch 25 % earlier and its partner then runs alone,
        // which uses the SIMD less well than two waves do (profiles/r02_c_wave_times.txt, r02_d_*).  Taking turns at priority 1 / 0
        // (one turn each) removed most of that (17.9 -> 17.2 us per turn) but left the older wave 7 % ahead, because half of the time
        // the two hold the same priority and age decides.  So no ties: the younger wave stays at 1, the older one takes 2 in three
        // turns of five and 0 in the other two -- with 1 : 1 the younger ends 12 us ahead in a 20-turn launch, with 2 : 1 the older
        // one does, with 3 : 2 the pair ends within 3 us of each other (tools/wave_times.py) -- 16.4 -> 16.0 us per turn (A/B on one box).
        if (__builtin_amdgcn_s_getreg(6148) & 1u) __builtin_amdgcn_s_setprio(1);
        else if ((0x15u >> (iter % 5)) & 1u) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(0);
    }
    if (MULTI) { PHASE(0); }                               // diagnostic build: the stamps of a launch are those of its last turn
    const bool envlane = LPW == WG || lane < LPW;
    const int E = envlane ? lane >> 1 : 0, P = lane & 1;
    const int col = envlane ? lane : 0;                 // LDS column (helpers never write; their reads are discarded)
    const bool valid = envlane && E < nvalid;
    const int e = valid ? e0 + E : e0;
    const size_t N = (size_t)S.N;
    const uint64_t p1nib = L.tab.nib[0];
    const uint64_t spd_n = L.tab.nib[1 + P], ctl_n = L.tab.nib[3 + P], cst_n = L.tab.nib[5 + P], typ_n = L.tab.nib[7 + P];
    const uint32_t misc = (uint32_t)L.tab.nib[9];
    const int max_turns = (int)(misc & 0xFFu);
#include "step_orders.inc"

#include "step_combat.inc"

#include "step_move_capture.inc"

#include "step_outputs.inc"
    }   // turns

    if (!(CHUNKABLE && io.nsets > 0)) break;
    // publish the chunk to the XCD's other workgroups: every store of this wave (state words, health rows, outputs) has reached the L2
    // they share (s_waitcnt vmcnt(0); the vector L1 is write-through), then the flag.  No L2 write-back: the set never leaves this XCD.
    // WHAT THIS RELIES ON (it is weaker than an agent-scope release, which the memory model would ask for and which costs a buffer_wbl2 walk
    // per chunk: 57 % slower, measured): (1) every array of the handle is ordinary coarse-grained device memory (hipMalloc; evg_create
    // checks the pointer attributes), cached in the L2 of the XCD that touches it; (2) producer and consumer of a set run on the same XCD
    // (HW_REG_XCC_ID picks the queue), hence share that L2; (3) 128-byte lines that hold words of sets owned by DIFFERENT XCDs (byte-per-env
    // arrays, ragged N) are only ever merged through byte-masked write-backs of the dirty bytes -- no XCD writes back bytes it did not
    // write.  The diagnostic library can publish with a real release instead (ablate bit 7) and the parity tests run both.
    // WHAT IT NO LONGER RELIES ON: luck.  A hand-over that served the consumer anything but the producer's latest state words is DETECTED: the lane's
    // checksum over (chunk number, its 21-24 state words) travels with the chunk (S.handoff) and the consumer recomputes it over what it loaded (fault bit 3;
    // tests: test_a_stale_chunk_hand_over_is_reported).  Covered: group, stamp, node, env, episode, return and agent words, i.e. every line of the
    // set's packed state.  Not covered: the float64 health rows (1 600 B per env, touched sparsely) -- they take the same path through the same L2 after
    // the same drain, and the parity tests compare them with the oracle bit for bit after chunked launches.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    {
        bool publish = true;
#ifdef EVG_DIAG      // fault-path test (ablate bit 6): the first chunk of the launch's first set is never published, its successor must give up and flag the
                     // handle
        publish = !(ABLATED(64u) && wg_chunk == 0 && wg_set == 0);
#endif
        if (publish && threadIdx.x == 0) {
            uint32_t* const pflag = S.progress + (e0 >> 5);
            const uint32_t pval = io.progress_base + (uint32_t)wg_chunk + 1u;
#ifdef EVG_DIAG      // ablate bit 7: publish with an agent-scope release (L2 write-back), what the memory model asks for
            if (ABLATED(128u)) __hip_atomic_store(pflag, pval, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            else
#endif
            __hip_atomic_store(pflag, pval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    WAVE_SYNC();                                         // the next unit's LDS traffic stays behind this one's
    }   // units

    STAMP_WAVE_END();
