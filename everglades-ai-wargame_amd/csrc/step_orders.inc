// step_orders.inc -- fragment of evg_step_kernel's turn loop (step_kernel.inc): the 7 order rows of this lane's player and their application.
// reads:  L (LDS: G, tab), lane / col / E / P / valid / e / N, turn, status, episode, act_in (prologue), ag_cycle / ag_swarm / ag_dfs, p1nib, iter / nturns
// writes: act[NA] (also to io.actions_out), L.G (accepted orders), turn (+1 when the env plays), the agent objects; defines `frozen`, `play`
    // this player's 7 order rows: read from the caller's tensor (in the prologue), or -- in the fused rollouts -- produced
    // here by the same generators as evg_random_actions / evg_scripted_actions and written out
    int2 act[NA];
    if (io.gen_actions) {
        if (DRAWS_ORDERS && io.gen_actions == 1) {
            if constexpr (MULTI) {
                uint32_t rk[20];
#pragma unroll
                for (int i = 0; i < 20; ++i) rk[i] = S.keys.k[i];          // scalar loads from the argument segment
                gen_random_rows(rk, S.env_id_base + (uint32_t)e, episode, turn, P, act);
            } else {
#pragma unroll
                for (int i = 0; i < NA; ++i) act[i] = act_in[i];         // drawn in the prologue, under the state loads
            }
        } else {                                        // on-device scripted agents of both seats (evg_rollout_policies, fused)
            const ChipView<StepLds<LPW>> view{&L, col, E, P, turn, p1nib};
            // both seats' policy ids as scalars, selected per lane (the compiler would otherwise turn the select into a per-lane
            // global load from the argument segment, and wait for vmcnt(0) -- i.e. for last turn's stores -- in front of its use)
            int pol0 = io.policy0, pol1 = io.policy1;
            asm volatile("" : "+s"(pol0), "+s"(pol1));
            const AgentTabs atabs{L.tab.nib[11], L.tab.nib[12], L.tab.nib[13], T};
            bool bot_lane = !SEAT || P != io.seat;              // one-seat form: the caller's lane has no agent (its object is neither consulted nor stored)
            // two-seat league form: only the league seat of an env whose member is a bot (member io.lg_qmember is the caller's second network: its rows
            // were decoded in the prologue, its bot is never consulted and its object words stay as they are)
            if constexpr (LEAGUE && !SEAT) bot_lane = P != io.seat && lg_m != io.lg_qmember;
            int pol = P ? pol1 : pol0;
            if constexpr (LEAGUE) pol = lg_pol;                 // a per-lane value: the env's member (the caller's lane is not a bot lane)
            agent_rows(pol, view, atabs, S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, episode, P, true, status == 0 && bot_lane,
                       &ag_cycle, &ag_swarm, &ag_dfs, act);
            if constexpr (SEAT || LEAGUE) {
#pragma unroll
                for (int i = 0; i < NA; ++i) act[i] = bot_lane ? act[i] : act_in[i];
            }
            if (valid && bot_lane && (!MULTI || iter == nturns - 1)) {      // padding lanes of a partial last workgroup never write
                const size_t ai_ = (size_t)P * N + e;
                S.agent_cycle[ai_] = ag_cycle; S.agent_swarm[ai_] = ag_swarm; S.agent_dfs[ai_] = ag_dfs;
            }
        }
        if (valid && io.actions_out) {
            int2* ao = reinterpret_cast<int2*>(io.actions_out) + ((size_t)e * 2 + P) * NA;
#pragma unroll
            for (int i = 0; i < NA; ++i) ao[i] = act[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NA; ++i) act[i] = act_in[i];             // loaded in the prologue (single-turn form only)
    }
    PHASE(1);

    const bool frozen = status != 0;                    // finished, not auto-reset: repeat terminal outputs
    const bool play = valid && !frozen && !observe_only;

    if (play) {
        turn += 1;                                                               // server.py:214
        // ---------------- orders of this lane's player (server.py:218-271)
        // Accepting an order changes neither the group's location nor whether it is `moving`, so tests 2 and 3
        // of every row can be taken from the pre-order words; rows interact only through test 1 (an id already
        // commanded this turn) and, for aliased ids, through the order of the writes (the later row wins, as in
        // the reference).  That makes the 7 LDS lookups independent instead of a 7-deep dependent chain.
        const uint64_t node_map = player_node_map(P, p1nib);
        if (DRAWS_ORDERS && !ABLATED(1u) && io.gen_actions == 1) {
            // Orders drawn in this kernel by gen_random_rows: 7 DISTINCT group ids in 0..11 and node ids in 1..11 by construction, so
            // the domain checks, the Python-list negative indices and the "already commanded this turn" test of the general path
            // below cannot trigger; every row is independent.
            uint32_t wv[NA], nv[NA], dv[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                nv[i] = map_node(node_map, (uint32_t)act[i].y);
                wv[i] = L.G[act[i].x][lane];
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) dv[i] = order_dist(L.tab.adj[wv[i] & G_LOC_M], nv[i]);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                // (seven DISTINCT groups: every word is written once, so a rejected row can store the word it read -- an unconditional LDS store of a select
                // instead of a predicated one: no exec-mask juggling and no branch per row)
                const bool accept = order_accepted(wv[i], dv[i]);
                const uint32_t ordered = ordered_word(wv[i], nv[i], dv[i]);
                L.G[act[i].x][lane] = accept ? ordered : wv[i];
            }
        } else if (!ABLATED(1u)) {
            int gidv[NA], nidv[NA], rawv[NA];
            uint32_t wv[NA], dv[NA];
            bool okv[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                gidv[i] = act[i].x; nidv[i] = act[i].y;
                okv[i] = order_ids(gidv[i], nidv[i], rawv[i], node_map, P);
                wv[i] = L.G[gidv[i]][lane];
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) dv[i] = order_dist(L.tab.adj[wv[i] & G_LOC_M], (uint32_t)nidv[i]);
            uint32_t used = 0;                                                   // the "already commanded this turn" chain (:241, :252)
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const bool accept = okv[i] & !((used >> rawv[i]) & 1u) & order_accepted(wv[i], dv[i]);
                used |= (accept ? 1u : 0u) << rawv[i];
                if (accept) L.G[gidv[i]][lane] = ordered_word(wv[i], (uint32_t)nidv[i], dv[i]);
            }
        }
    }
    PHASE(2);
