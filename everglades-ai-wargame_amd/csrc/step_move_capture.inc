// step_move_capture.inc -- fragment of evg_step_kernel's turn loop (step_kernel.inc): movement, per-node aggregates, capture, scores, status,
// rewards / done / winner, episode bookkeeping and auto-reset.
// reads:  L.G, L.NW, L.tab, st[3], play, valid, turn, status, episode, ep_ret, spd_n / ctl_n / cst_n, max_turns
// writes: gw[12] (this lane's group words after the turn), st[3], cntv[12], L.NW (capture), L.u.A (units listed per node), score[2], status,
//         turn / episode (reset), ep_ret, do_reset, the per-env outputs (reward, done, winner, scores, status) and the episode results;
//         league forms: io.lg_counts (tally), and in the reset branch io.lg_assign, io.lg_objects, the agent words (member redraw and object swap)
    // ---------------- movement of this lane's groups (server.py:656-706), branch-free
    uint32_t gw[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) gw[k] = envlane ? L.G[k][col] : 0u;
    if (play && !ABLATED(4u)) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            bool arrive;
            gw[k] = move_group(gw[k], (uint32_t)((spd_n >> (4 * k)) & 15u), arrive);
            const uint32_t sh = 8 * (k & 3);
            st[k >> 2] = arrive ? ((st[k >> 2] & ~(0xFFu << sh)) | ((uint32_t)turn << sh)) : st[k >> 2];
        }
    }
    PHASE(7);

    // ---------------- per-node aggregates of this side (post-movement): capture points | units listed << 16
    zero_columns12<LPW>(L.u.A, lane, envlane);
    int my_unit_score = 0, my_alive = 0;
    int cntv[12];                      // alive units per group: also what the observation shows (:493)
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const uint32_t w = gw[k];
        int cnt = __popc(w & G_MASK_M);
        asm volatile("" : "+v"(cnt));           // keep the count in its register for the observation (the compiler would recompute it there)
        cntv[k] = cnt;
        if (envlane) atomicAdd(&L.u.A[w & G_LOC_M][lane], node_contribution(w, cnt, (uint32_t)((ctl_n >> (4 * k)) & 15u)));   // ds_add_u32 (0 for a destroyed group)
        my_unit_score += unit_score(cnt, (uint32_t)((cst_n >> (4 * k)) & 15u));
        my_alive += cnt;
    }
    WAVE_SYNC();

    // ---------------- capture (server.py:708-767) and node scores (:297-310): the pair splits the nodes
    int part0 = 0, part1 = 0;          // score contributions of this lane's nodes to player 0 / player 1
    int base_cap = 0;
    {
        // The pair splits the node IDs 0..11 in halves (player 0's lane: 0..5, where ID 0 does not exist; player 1's lane: 6..11), so
        // every LDS address below is one per-lane base plus a constant.  controlledBy is kept in its stored form (+1: 0 = nobody).
        const int nb = P ? 6 : 0;
        uint32_t a0v[6], a1v[6], nwv[6];
        int cpv[6], tsv[6];
        const uint32_t* const pa = &L.u.A[nb][col & ~1];
        const uint32_t* const pn = &L.NW[nb][E];
        const int* const pc = &L.tab.cp[nb];
        const int* const pt = &L.tab.ts[nb];
#pragma unroll
        for (int j = 0; j < 6; ++j) {                  // all LDS / table reads first, then pure ALU
            a0v[j] = pa[j * LPW];
            a1v[j] = pa[j * LPW + 1];
            nwv[j] = pn[j * (LPW / 2)];
            cpv[j] = pc[j];
            tsv[j] = pt[j];
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const NodeTurn r = capture_node(nwv[j], (int)(a0v[j] & 0xFFFFu), (int)(a1v[j] & 0xFFFFu), cpv[j], tsv[j], j > 0 || P != 0, play);
            // (an unconditional store: the word is unchanged when nothing is captured; row 0 does not exist and is never read.  Helper lanes of the
            // 16-envs-per-wave variant alias env slot 0 and must not store)
            if (envlane) L.NW[nb + j][E] = r.nw;
            base_cap |= r.base_cap ? 1 : 0;
            part0 += r.part0;
            part1 += r.part1;
        }
    }
    // combine the pair: scores (server.py:291-317) and status (:321-328) are then known to both lanes
    const int opp_unit_score = xchg1(my_unit_score), opp_alive = xchg1(my_alive);
    part0 += xchg1(part0);
    part1 += xchg1(part1);
    base_cap |= xchg1(base_cap);
    int score[2];
    score[0] = part0 + (P ? opp_unit_score : my_unit_score);
    score[1] = part1 + (P ? my_unit_score : opp_unit_score);
    status = play ? status_after_turn(status, turn, max_turns, my_alive + opp_alive, base_cap != 0) : status;      // :321-328
    if constexpr (MT) {
        if (play && mt_lane && turn % 10 == 0) (void)mt_randint(mt, 2u * NG + 1u);  // :337-338 focus draw: unobservable, but it consumes output
    }
    PHASE(8);

    // ---------------- reward / done / winner (everglades_env.py:37-61, evaluate.py:155-160)
    const bool done = status != 0;
    const TurnOutcome out = turn_outcome(done, score[0], score[1]);
    const float rew0 = out.rew0, rew1 = out.rew1;
    const int winner = out.winner;
    {
        // the output pointers are fetched together (one scalar-load batch), not one by one inside the branches below
        float* const p_reward = io.reward;
        uint8_t* const p_done = io.done;
        int8_t* const p_winner = io.winner;
        int32_t* const p_scores = io.scores;
        uint8_t* const p_status = io.status;
        if (valid && !observe_only && P == 0) {
            reinterpret_cast<float2*>(p_reward)[e] = make_float2(rew0, rew1);
            p_done[e] = done ? 1 : 0;
            if (p_winner) p_winner[e] = (int8_t)winner;
            if (p_scores) reinterpret_cast<int2*>(p_scores)[e] = make_int2(score[0], score[1]);
            if (p_status) p_status[e] = (uint8_t)status;
        }
    }

    // ---------------- episode bookkeeping + auto-reset (each lane keeps its own player's return)
    bool do_reset = false;
    float* const p_fin_ret = S.fin_ret;
    int32_t* const p_fin_len = S.fin_len;
    int8_t* const p_fin_win = S.fin_win;
    const int auto_reset = S.auto_reset;
    if (play) {
        float r = ep_ret + (P ? rew1 : rew0);
        if (done) {
            p_fin_ret[(size_t)e * 2 + P] = r;
            if (P == 0) { p_fin_len[e] = turn; p_fin_win[e] = (int8_t)winner; }
            if (auto_reset) { do_reset = true; r = 0.f; }
        }
        ep_ret = r;
    }
    if (valid && !observe_only && (!MULTI || iter == nturns - 1)) S.ep_ret[(size_t)P * N + e] = ep_ret;
    {
        const bool fin = play && done && P == 0;
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
            if constexpr (LEAGUE) {
                // ... and per league member, seen from the caller's seat (include/evg.h, evg_league COUNTERS: the winner code is the script's decision
                // from the final rewards), in the same pattern: one pass per member that finished a game in this wave, lane 0 adds the pass's counts
                uint64_t rest = mf;
                while (rest) {
                    const int m = __builtin_amdgcn_readlane(lg_m, __ffsll((unsigned long long)rest) - 1);
                    const bool mine = fin && lg_m == m;
                    const uint64_t mm = __ballot(mine);
                    // (EVG_WINNER_P0 / P1 are the seats' numbers)
                    const int ng = __popcll(mm), nw = __popcll(__ballot(mine && winner == io.seat)), nt = __popcll(__ballot(mine && winner == EVG_WINNER_TIE));
                    if (lane == 0) {
                        unsigned long long* const c = io.lg_counts + 4 * m;
                        atomicAdd(&c[0], (unsigned long long)ng);
                        if (nw) atomicAdd(&c[1], (unsigned long long)nw);
                        if (nt) atomicAdd(&c[2], (unsigned long long)nt);
                        if (ng - nw - nt) atomicAdd(&c[3], (unsigned long long)(ng - nw - nt));
                    }
                    rest &= ~mm;
                }
            }
        }
    }
    if (do_reset) {
        // new episode: state of game_init (server.py:133-209)
        turn = 0; status = 0; episode += 1u;
        if (MT && mt_lane) { (void)mt_randint(mt, 2u * NG + 1u); (void)mt_randint(mt, 2u * NG + 1u); }   // game_init :205 and its game_end :338 (turn 0)
#pragma unroll
        for (int j = 0; j < 3; ++j) st[j] = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) { gw[k] = L.tab.init_grp[P * 12 + k]; cntv[k] = __popc(gw[k] & G_MASK_M); }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int n = P ? 7 + j : 1 + j;
            if (n <= NN) L.NW[n][E] = L.tab.init_node[n];
        }
        // ... and the units this side lists per node (what the opponent's observation shows): the whole army stands on its base
#pragma unroll
        for (int n = 0; n < 12; ++n) L.u.A[n][lane] = 0;
        L.u.A[gw[0] & G_LOC_M][lane] = (uint32_t)NU << 16;
        if constexpr (LEAGUE) {
            // the league seat's lane: the member of the episode that starts (the draw is keyed by the NEW episode index), and when it is another one, the
            // object swap -- the live words to the old member's slot, the new member's become the live ones.  The weights (at most 16 doubles) and the
            // swap's loads and stores are touched only here, once per episode and env
            if (P != io.seat && io.lg_resample) {
                bool bad = false;
                // (the seed is made opaque here: the draw's key schedule is then computed in this branch, once per episode, instead of being shared with
                // the prologue's Philox blocks and kept in scalar registers across the whole turn, which spilled six of them in the Q form)
                uint32_t lg_seed_lo = S.seed_lo, lg_seed_hi = S.seed_hi;
                asm volatile("" : "+s"(lg_seed_lo), "+s"(lg_seed_hi));
                const int m_new = league_choice(lg_seed_lo, lg_seed_hi, S.env_id_base + (uint32_t)e, episode, P, io.lg_weights, io.lg_num, lg_m, bad);
                if (bad) atomicOr(io.lg_ctl, (unsigned long long)EVG_LEAGUE_S_BAD_WEIGHTS);
                if (m_new != lg_m) {
                    league_swap(io.lg_objects, N, (size_t)e, lg_m, m_new, ag_cycle, ag_swarm, ag_dfs);
                    const size_t ai_ = (size_t)P * N + e;
                    S.agent_cycle[ai_] = ag_cycle; S.agent_swarm[ai_] = ag_swarm; S.agent_dfs[ai_] = ag_dfs;
                    io.lg_assign[e] = (uint8_t)m_new;
                }
            }
        }
    }
    WAVE_SYNC();        // node words final; everybody is done adding to A
    PHASE(9);
