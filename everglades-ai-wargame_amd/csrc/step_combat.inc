// step_combat.inc -- fragment of evg_step_kernel's turn loop (step_kernel.inc): combat at contested nodes (server.py:503-654).
// reads:  L.G (post-orders group words), st[3] (arrival stamps), play, turn, episode, e0, misc, mt / mt_lane (stock entropy), S.health
// writes: S.health (the rows of groups that were hit), L.G (alive mask + cached average of those groups); uses the union L.u.c
    // ---------------- combat (server.py:503-654)
    // Stage 0 (lane = env side): pre-combat snapshot.  A group fights at its node if it is alive and not moving
    // (:525) and the node holds such groups of both players (:539).  The reference walks node.groups[p] in list
    // order, which is (arrival stamp, gid) order (SURVEY Appendix C); the target index uid counts alive units
    // along that order, so each fighting group gets the prefix `base` of alive units listed before it.
    uint32_t g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) g[k] = envlane ? L.G[k][col] : 0u;
    // (Round 5 tried a SPARSE stage 0 -- keys for the fighting groups only, the sorted positions visited only while some lane still has a group there: a
    // wavefront's busiest side has 5.1 fighting groups on average, not 12 -- and measured it SLOWER: 14.57 against 14.40 us per turn, four alternations on one
    // box.  The wave-uniform votes and branches between the positions (a v_cmp, a scalar branch and a VALU -> SALU round trip per position and pass) cost more
    // than the seven positions they skip.  profiles/r05_c_instruction_experiments.txt)
    uint32_t occ = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const uint32_t w = g[k];
        const bool elig = (w & G_MASK_M) != 0 && ((w & G_MODE_M) >> G_MODE_S) != MODE_MOVING;
        occ |= (elig ? 1u : 0u) << (w & G_LOC_M);
    }
    const uint32_t contested = (play && !ABLATED(2u)) ? (occ & (uint32_t)xchg1((int)occ)) : 0u;
    if (__any(contested != 0)) {                          // wave-uniform: skip when none of the 32 envs fights
        zero_columns12<LPW>(L.u.c.FS, lane, envlane);
        uint32_t key[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const uint32_t w = g[k];
            const uint32_t mask = (w & G_MASK_M) >> G_MASK_S;
            const uint32_t elig = (mask != 0 && ((w & G_MODE_M) >> G_MODE_S) != MODE_MOVING) ? 1u : 0u;
            const uint32_t stamp = (st[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            key[k] = (stamp << 21) | ((uint32_t)k << 17) | ((w & G_LOC_M) << 13) | (mask << 1) | elig;
        }
#define EVG_CE(a, b) { const uint32_t lo_ = min(key[a], key[b]); key[b] = max(key[a], key[b]); key[a] = lo_; }
        EVG_SORT12_CES(EVG_CE)
#undef EVG_CE
        // List order (server.py:549-566 walks node.groups[p]): the prefix `base` of alive fighting units listed before a group at its
        // node comes from one returning LDS add per group into this side's per-node total (the FS column of the lane, high half;
        // the low half receives the damage-pool offset in stage 1): the LDS executes a wavefront's adds in issue order.
        uint32_t fmask = 0, basev[12];
        bool fightv[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const uint32_t kk = key[i];
            const uint32_t loc = (kk >> 13) & 15u, mask = (kk >> 1) & 0xFFFu;
            fightv[i] = (kk & 1u) && ((contested >> loc) & 1u);
            basev[i] = envlane ? atomicAdd(&L.u.c.FS[loc][lane], fightv[i] ? (uint32_t)__popc(mask) << 16 : 0u) : 0u;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const uint32_t kk = key[i];
            const uint32_t gid = (kk >> 17) & 15u;
            fmask |= (fightv[i] ? 1u : 0u) << gid;
            // fights | prefix << 16 | node << 12 | alive mask: bits 16..1 of the key are already node << 12 | mask
            if (envlane) L.u.c.SNAP[gid][lane] = fightv[i] ? (0x80000000u | basev[i] | ((kk >> 1) & 0xFFFFu)) : 0u;
        }
        if (envlane) { L.u.c.TURN[lane] = (uint32_t)turn; L.u.c.EPI[lane] = episode; }
        // damage bytes this side needs: one per alive fighting unit, rounded up to a word per node
        int ndw = 0;
        {
            uint32_t c = contested;
            while (c) {
                const uint32_t n = (uint32_t)__ffs(c) - 1u;
                c &= c - 1;
                ndw += (int)(((L.u.c.FS[n][col] >> 16) + 3u) >> 2);
            }
        }
        PHASE(3);

        // Stage 1: wave-wide work list (one item per fighting group) and damage-pool layout, by prefix scan.  The items of the
        // 12-unit group (gid 11) are listed BEFORE all others: only that group needs a second block of draws (more than 8 units)
        // and the health slots 8..11, so only the FIRST round of 64 items -- whose lanes are all busy anyway -- runs the long code,
        // and the last round, 18 items on average, holds 8-unit groups only: phase B deals those to two lanes each.
        const int nf_a = __popc(fmask & 0x7FFu), nf_b = (int)((fmask >> 11) & 1u);
        const int packed = nf_a | (nf_b << 10) | (ndw << 17);   // three counts in one scan: <= 704 items (10 bits), <= 64 (7 bits), <= 2112 words (12 bits)
        int incl = packed;
        // inclusive scan over the 64 lanes in registers: log-steps inside each row of 16 lanes (DPP row_shr, zero fill),
        // then the row totals are carried across rows (DPP row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xA, 0xF, false);
        incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xC, 0xF, false);
        const int excl = incl - packed;
        const int tot = __builtin_amdgcn_readlane(incl, WG - 1), mid = __builtin_amdgcn_readlane(excl, LPW / 2);
        const int excl_a = excl & 0x3FF, excl_b = (excl >> 10) & 0x7F, excl_d = excl >> 17;
        const int tot_a = tot & 0x3FF, tot_b = (tot >> 10) & 0x7F, tot_d = tot >> 17, mid_a = mid & 0x3FF, mid_b = (mid >> 10) & 0x7F, mid_d = mid >> 17;
        // the pool holds every fight of the wave in the common case; otherwise two passes of 16 envs each
        const int npass = tot_d <= DP_CAP ? 1 : 2;
        const uint32_t dmg_nib = (misc >> 8) & 0xFFFFu;
        const bool fast_div = ((misc >> 24) & 1u) != 0;
        for (int ps = 0; ps < npass; ++ps) {
            const bool inpass = npass == 1 || (lane / (LPW / 2)) == ps;     // helper lanes own no items
            const bool second = npass == 2 && ps == 1, first = npass == 2 && ps == 0;
            const int ref_a = second ? mid_a : 0, ref_b = second ? mid_b : 0, ref_d = second ? mid_d : 0;
            const int end_a = first ? mid_a : tot_a, end_b = first ? mid_b : tot_b, end_d = first ? mid_d : tot_d;
            const int na = end_a - ref_a, nitems = na + (end_b - ref_b), ndwords = end_d - ref_d;
            const int nb = nitems - na;                          // items of the 12-unit group: listed FIRST (see phase B)
            if (inpass) {
                int wi = nb + excl_a - ref_a;
                uint32_t f = fmask & 0x7FFu;
                while (f) {
                    const uint32_t gid = (uint32_t)__ffs(f) - 1u;
                    f &= f - 1;
                    L.u.c.W[wi++] = (uint16_t)((uint32_t)lane | (gid << 6));
                }
                if (nf_b) L.u.c.W[excl_b - ref_b] = (uint16_t)((uint32_t)lane | (11u << 6));
                int doff = excl_d - ref_d;
                uint32_t c = contested;
                while (c) {
                    const uint32_t n = (uint32_t)__ffs(c) - 1u;
                    c &= c - 1;
                    const uint32_t tnw = L.u.c.FS[n][lane] & 0xFFFF0000u;     // alive fighting units of this side at the node (stage 0)
                    L.u.c.FS[n][lane] = tnw | (uint32_t)doff;
                    doff += (int)(((tnw >> 16) + 3u) >> 2);
                }
            }
            for (int i = lane; i < ndwords; i += WG) L.u.c.DP[i] = 0;
            WAVE_SYNC();
            PHASE(4);

            // health row of this lane's first item: issued now, consumed in phase B, so that the HBM latency hides
            // behind the draws (a fighting group is very likely to be hit; 64-96 B per group)
            constexpr bool kPrefetch = LPW == WG;      // the 16-env variant runs at 4 waves/SIMD and has no registers to spare
            double hpre[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (kPrefetch) {
                const uint32_t item0 = L.u.c.W[lane < nitems ? lane : 0];
                const int SL0 = (int)(item0 & 63u), gid0 = (int)(item0 >> 6);
                const double2* r2 = reinterpret_cast<const double2*>(S.health + (size_t)(e0 + (SL0 >> 1)) * (2 * NU) + (SL0 & 1) * NU + gid0 * 8);
                if (lane < nitems) {
#pragma unroll
                    for (int sl = 0; sl < 4; ++sl) { const double2 v = r2[sl]; hpre[2 * sl] = v.x; hpre[2 * sl + 1] = v.y; }
                    if (gid0 == 11) {
#pragma unroll
                        for (int sl = 4; sl < 6; ++sl) { const double2 v = r2[sl]; hpre[2 * sl] = v.x; hpre[2 * sl + 1] = v.y; }
                    } else {
                        hpre[8] = hpre[9] = hpre[10] = hpre[11] = 0.0;
                    }
                }
            }

            // ... and so is the half row of this lane's share of the sparse LAST round (see phase B: two lanes per item), whose loads would otherwise be issued
            // behind the first round's stores and waited for with nothing to overlap them (-0.6 % per turn; prefetching the eight slots of a second FULL round
            // as well costs nine more registers and measured the same: profiles/r05_c_instruction_experiments.txt)
            constexpr bool kSplitLastRound = LPW == WG;
            const int rem_items = nitems & (WG - 1), full_items = nitems - rem_items;
            const bool split_last = kSplitLastRound && rem_items > 0 && rem_items <= WG / 2 && full_items >= nb;
            double hpre2[4] = {0, 0, 0, 0};
            if (kPrefetch && split_last) {
                const int it2 = full_items + (lane >> 1);
                const uint32_t item2 = L.u.c.W[it2 < nitems ? it2 : 0];
                const int SL2 = (int)(item2 & 63u), gid2 = (int)(item2 >> 6);
                const double* row2 = S.health + (size_t)(e0 + (SL2 >> 1)) * (2 * NU) + (SL2 & 1) * NU + gid2 * 8 + (lane & 1) * 4;
                const double2* r2 = reinterpret_cast<const double2*>(row2);
                if (it2 < nitems) {
                    const double2 v0 = r2[0], v1 = r2[1];
                    hpre2[0] = v0.x; hpre2[1] = v0.y; hpre2[2] = v1.x; hpre2[3] = v1.y;
                }
            }

            // Phase A (:549-566): one lane per fighting group; each of its alive units draws one target among the
            // opposing side's alive fighting units at the node; damage accumulates in the pool (LDS atomics,
            // integer and order-free, hence deterministic)
            if constexpr (MT) {
                // stock entropy: one sequential stream per env, consumed exactly in the reference's loop order -- nodes
                // ascending (:505), attacking player 0 then 1 (:549), that player's groups in list order (ascending
                // `base`), one draw per alive unit (:562)
                if (mt_lane && inpass) {
                    uint32_t c = contested;
                    while (c) {
                        const int node = __ffs(c) - 1;
                        c &= c - 1;
                        for (int side = 0; side < 2; ++side) {
                            const int SL = lane | side;
                            const uint32_t fso = L.u.c.FS[node][SL ^ 1];
                            const uint32_t tot_o = fso >> 16, doff_o = fso & 0xFFFFu;
                            const uint64_t tn_s = L.tab.nib[7 + side];
                            int last = -1;
                            for (;;) {
                                int best = 256, bg = -1, bcnt = 0;
                                for (int k = 0; k < 12; ++k) {
                                    const uint32_t sp = L.u.c.SNAP[k][SL];
                                    const int b = (int)((sp >> 16) & 0xFFu);
                                    if ((sp >> 31) && (int)((sp >> 12) & 15u) == node && b > last && b < best) { best = b; bg = k; bcnt = __popc(sp & 0xFFFu); }
                                }
                                if (bg < 0) break;
                                last = best;
                                const uint32_t type = (uint32_t)((tn_s >> (4 * bg)) & 15u);
                                const uint32_t dmg = (dmg_nib >> (4 * type)) & 15u;
                                for (int j = 0; j < bcnt; ++j) {
                                    const uint32_t uid = mt_randint(mt, tot_o);
                                    atomicAdd(&L.u.c.DP[doff_o + (uid >> 2)], dmg << (8 * (uid & 3u)));
                                }
                            }
                        }
                    }
                }
            } else {
            const uint32_t id_base = S.env_id_base + (uint32_t)e0;
            uint32_t rk[20];
#pragma unroll
            for (int i = 0; i < 20; ++i) rk[i] = S.keys.k[i];              // the round keys: scalar loads from the argument segment
            for (int it = lane; it < nitems; it += WG) {
                const uint32_t item = L.u.c.W[it];
                const int SL = (int)(item & 63u), gid = (int)(item >> 6), side = SL & 1;
                const uint32_t sp = L.u.c.SNAP[gid][SL];
                const int node = (int)((sp >> 12) & 15u), cnt = __popc(sp & 0xFFFu);
                const uint32_t fso = L.u.c.FS[node][SL ^ 1];
                const uint32_t tot_o = fso >> 16, doff_o = fso & 0xFFFFu;
                const uint64_t tn_s = L.tab.nib[7 + side];
                const uint32_t type = (uint32_t)((tn_s >> (4 * gid)) & 15u);
                const uint32_t dmg = (dmg_nib >> (4 * type)) & 15u;
                const int turn_e = (int)L.u.c.TURN[SL];
                const uint32_t epi_e = L.u.c.EPI[SL], env_id_e = id_base + (uint32_t)(SL >> 1);
                // one block = eight 16-bit draws; a second one only for the 12-unit group -- taken by the whole wavefront when ANY of its items needs it (a
                // wave-uniform vote instead of a per-lane loop: the lanes without a ninth unit add zeros)
                auto draw_block = [&](int b) {
                    const uint4 x = rng_block(rk, env_id_e, epi_e, RNG_COMBAT, (uint32_t)b, turn_e, node, side, gid);
                    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        // (a unit the group no longer has adds 0 to a valid pool word instead of being predicated off: the atomic issues for the wave
                        // either way, the exec-mask juggling and the branch per draw do not)
                        const uint32_t uid = __umul24(rng_half(xs, i), tot_o) >> 16;                    // :562 (tot_o <= 100)
                        atomicAdd(&L.u.c.DP[doff_o + (uid >> 2)], b * 8 + i < cnt ? dmg << (8 * (uid & 3u)) : 0u);     // :563-566
                    }
                };
                draw_block(0);
                if (__any(cnt > 8)) draw_block(1);
            }
            }
            WAVE_SYNC();
            PHASE(5);

            // The prefetched rows are waited for HERE by every lane, used or not: a register with a load still in flight makes the
            // compiler wait for vmcnt(0) wherever that register is written next (the movement phase), and vmcnt(0) also waits for
            // the health stores of phase B to be acknowledged -- a full store round trip per turn.
            if (kPrefetch) {
#pragma unroll
                for (int sl = 0; sl < 12; ++sl) asm volatile("" :: "v"(hpre[sl]));
#pragma unroll
                for (int sl = 0; sl < 4; ++sl) asm volatile("" :: "v"(hpre2[sl]));
            }
            // Phase B (:573-644): one lane per fighting group; the uid-th alive unit of the snapshot (list-order
            // prefix + rank among the group's alive slots) takes its summed damage.  Both directions read only
            // the snapshot and the pool, so they are simultaneous like in the reference.
            // An instruction costs a wavefront the same whether 64 or 16 of its lanes are active (profiles/r03_m_exec_mask_issue_rates.txt),
            // and a wavefront has 82 items per turn on average: one full round and one with 18 items.  That sparse last round -- 8-unit
            // groups only, thanks to the list order -- is dealt to TWO lanes per item when it has at most 32 items: each lane takes four
            // of the eight unit slots, the pair exchanges the dead-unit mask and the half sums by DPP (the sum keeps numpy's pairwise
            // order: (h0+h1)+(h2+h3) is the left half, (h4+h5)+(h6+h7) the right one).
            const int nmain = split_last ? full_items : nitems;
            for (int it = lane; it < nmain; it += WG) {
                const uint32_t item = L.u.c.W[it];
                const int SL = (int)(item & 63u), gid = (int)(item >> 6), side = SL & 1;
                const uint32_t sp = L.u.c.SNAP[gid][SL];
                const int node = (int)((sp >> 12) & 15u);
                const uint32_t mask = sp & 0xFFFu;
                const uint32_t doff = L.u.c.FS[node][SL] & 0xFFFFu;
                const uint32_t base = (sp >> 16) & 0xFFu;
                // the group's alive units are consecutive target indices, so their damage bytes are one run of <= 12 bytes in the
                // pool starting at byte `run0` (<= 15 bytes with the misalignment: four words, read at once)
                const uint32_t run0 = doff * 4u + base, w0i = run0 >> 2, sh0 = run0 & 3u;
                uint32_t dw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) dw[q] = L.u.c.DP[min(w0i + (uint32_t)q, (uint32_t)(DP_CAP - 1))];
                // align the run to byte 0 (v_alignbyte_b32) and clear what lies beyond the group's own `cnt` bytes (the next
                // group's damage): byte r of {a0, a1, a2} is then the damage of the group's r-th alive unit
                const uint32_t cnt = (uint32_t)__popc(mask);                                          // 1..12
                uint32_t a0 = __builtin_amdgcn_alignbyte(dw[1], dw[0], sh0), a1 = __builtin_amdgcn_alignbyte(dw[2], dw[1], sh0);
                uint32_t a2 = __builtin_amdgcn_alignbyte(dw[3], dw[2], sh0);
                {
                    const uint64_t keep = cnt >= 8u ? ~0ull : ((1ull << (8u * cnt)) - 1ull);
                    a0 &= (uint32_t)keep; a1 &= (uint32_t)(keep >> 32);
                    a2 = cnt > 8u ? (cnt >= 12u ? a2 : (a2 & ((1u << (8u * (cnt - 8u))) - 1u))) : 0u;
                }
                if ((a0 | a1 | a2) != 0u) {
                    double* row = S.health + (size_t)(e0 + (SL >> 1)) * (2 * NU) + side * NU + gid * 8;
                    double h[12];
                    if (kPrefetch && it < WG) {                     // first round: prefetched before the draws
#pragma unroll
                        for (int sl = 0; sl < 12; ++sl) h[sl] = hpre[sl];
                    } else {
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
                    auto apply_hits = [&](auto fast) { deadmask = hit_slots<decltype(fast)::value>(h, 0, gid == 11, mask, a0, a1, a2, denom, rcp); };
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
            if (split_last) {
                const int it = full_items + (lane >> 1), hf = lane & 1;      // item and which half of its unit slots (0: slots 0..3, 1: slots 4..7)
                if (it < nitems) {
                    const uint32_t item = L.u.c.W[it];
                    const int SL = (int)(item & 63u), gid = (int)(item >> 6), side = SL & 1;      // gid < 11: an 8-unit group
                    const uint32_t sp = L.u.c.SNAP[gid][SL];
                    const int node = (int)((sp >> 12) & 15u);
                    const uint32_t mask = sp & 0xFFu;
                    const uint32_t doff = L.u.c.FS[node][SL] & 0xFFFFu;
                    const uint32_t base = (sp >> 16) & 0xFFu;
                    const uint32_t run0 = doff * 4u + base, w0i = run0 >> 2, sh0 = run0 & 3u;
                    uint32_t dw[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) dw[q] = L.u.c.DP[min(w0i + (uint32_t)q, (uint32_t)(DP_CAP - 1))];
                    const uint32_t cnt = (uint32_t)__popc(mask);                                      // 1..8
                    uint32_t a0 = __builtin_amdgcn_alignbyte(dw[1], dw[0], sh0), a1 = __builtin_amdgcn_alignbyte(dw[2], dw[1], sh0);
                    {
                        const uint64_t keep = cnt >= 8u ? ~0ull : ((1ull << (8u * cnt)) - 1ull);
                        a0 &= (uint32_t)keep; a1 &= (uint32_t)(keep >> 32);
                    }
                    if ((a0 | a1) != 0u) {                                                        // the same for both lanes of the pair
                        double* row = S.health + (size_t)(e0 + (SL >> 1)) * (2 * NU) + side * NU + gid * 8 + hf * 4;
                        double h[4];
                        if (kPrefetch) {                                // prefetched before the draws
#pragma unroll
                            for (int j = 0; j < 4; ++j) h[j] = hpre2[j];
                        } else {
                            const double2* r2 = reinterpret_cast<const double2*>(row);
                            const double2 v0 = r2[0], v1 = r2[1];
                            h[0] = v0.x; h[1] = v0.y; h[2] = v1.x; h[3] = v1.y;
                        }
                        const uint32_t type = (uint32_t)((L.tab.nib[7 + side] >> (4 * gid)) & 15u);
                        const int di = damage_index(type, L.NW[node][SL >> 1], side, node);      // node defence of the controlling side, :592-597
                        const double denom = L.tab.den[di], rcp = L.tab.rcp[di];
                        uint32_t deadmask = 0;                                                       // of this lane's slots
                        auto apply_hits4 = [&](auto fast) { deadmask = hit_slots<decltype(fast)::value>(h, 4 * hf, false, mask, a0, a1, 0u, denom, rcp); };
                        if (fast_div) apply_hits4(std::true_type{}); else apply_hits4(std::false_type{});     // quotient :601, subtraction :609
                        double2* w2 = reinterpret_cast<double2*>(row);
                        w2[0] = make_double2(h[0], h[1]);
                        w2[1] = make_double2(h[2], h[3]);
                        const uint32_t newmask = mask & ~(deadmask | (uint32_t)xchg1((int)deadmask));
                        const double mine = (h[0] + h[1]) + (h[2] + h[3]);
                        const double other = __hiloint2double(xchg1(__double2hiint(mine)), xchg1(__double2loint(mine)));
                        const double sum = hf ? other + mine : mine + other;                          // left half + right half (np.sum's pairwise order)
                        if (hf == 0) L.G[gid][SL] = hit_word(L.G[gid][SL], newmask, sum);
                    }
                }
            }
            WAVE_SYNC();
        }
    }
    PHASE(6);
