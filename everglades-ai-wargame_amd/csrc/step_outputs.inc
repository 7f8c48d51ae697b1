// step_outputs.inc -- fragment of evg_step_kernel's turn loop (step_kernel.inc): the observation image in LDS, the state store, the coalesced
// observation write-out and the health rows of envs that start a new episode.
// reads:  gw[12], cntv[12], st[3], L.NW, L.u.A, L.tab.res, turn, status, episode, do_reset, valid / nvalid / e0, iter / nturns
// writes: L.u.O (the image), io.obs, the state arrays (after the launch's last turn), L.G (next turn's words, persistent form), S.health (restarted envs),
//         io.feat_shared / io.feat_swarm (one-seat form, two-seat Q form)
    // ---------------- observation of this lane's player (board_state :382-455, player_state :457-501,
    // everglades_env.py:158-171), written as int16 straight into the wave's output image in LDS.
    // A lane's row of 105 values starts at byte 210 R of the image (R = its row), so nothing wider than a halfword is aligned in a row's own
    // terms -- stores merged from neighbouring values were 8 / 12 / 16 bytes at 2 or 4 mod 8, which the LDS replays at 64 cycles each (profiles/
    // r13_a_lds_store_alignment.txt).  The row is therefore assembled in REGISTERS, as the 53 dwords Z[d] = (v[2d], v[2d+1]) of an even row, and stored
    // on the dword grid of the flat image: an even row's dwords are Z[0..51] themselves, an odd row -- which starts half a dword in -- stores
    // (v[2d+1], v[2d+2]) = the 64-bit {Z[d+1], Z[d]} shifted right by 16, so ONE v_alignbit_b32 with the per-lane shift 16 (R & 1) serves both
    // parities.  The halfword left over on the row's odd side (value 104 of an even row, value 0 -- the turn -- of an odd one) is the lane's one 16-bit
    // store; the two halfwords of a dword that straddles two rows are so written by their own lanes, and no lane touches another's.
    // Board part by SLOT (the position in the row is then a compile-time one): slot s of player 1's view shows node p1_node_map[s] (:437-439),
    // player 0's view is the identity -- the node words, the unit counts and the flags are read at that runtime node (aligned 4-byte reads).
    // (a rollout without an observation buffer -- evg_rollout_*(obs_out = NULL): the evaluation harness, which reads only the episode
    // results -- skips the image and the write-out altogether: a sixth of the turn's instructions and 55 % of its bytes)
    const bool want_obs = io.obs != nullptr;
    if (want_obs) {
    const uint64_t own_n = player_node_map(P, p1nib);   // nibble s = the node slot s shows = node s in this player's numbering (:485-486)
    uint32_t nw_s[12], ou_s[12], res_s[12];
#pragma unroll
    for (int s = 1; s <= NN; ++s) {
        const uint32_t n = map_node(own_n, (uint32_t)s);
        nw_s[s] = L.NW[n][E];
        ou_s[s] = L.u.A[n][col ^ 1];                    // high half: opposing units listed at the node
        res_s[s] = (uint32_t)L.tab.res[n];              // DEFENSE flag | OBSERVE flag << 16
    }
    WAVE_SYNC();        // A is dead from here on (the reads above are issued, and the LDS keeps a wave's order): the union becomes the output image
    // one-seat form: the image is [env][105], built by the caller's lane only.  (Splitting that row between the two lanes of the pair -- half the
    // instructions -- and the 28 MB less to write change nothing measurable: 26.7 us either way, like evg_step with both rows; a single-turn launch
    // lasts as long as its slowest SIMD pair, not as long as its instruction or byte count: DESIGN.md section 6.)
    if (envlane && (!SEAT || P == io.seat)) {
        int v[OBS];
        v[0] = turn;
#pragma unroll
        for (int s = 1; s <= NN; ++s) {
            int t[4];
            obs_node(t, (int)res_s[s], nw_s[s], (int)(ou_s[s] >> 16));
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * s - 3 + j] = t[j];
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            int t[5];
            obs_group(t, gw[k], own_n, (uint32_t)((typ_n >> (4 * k)) & 15u), cntv[k]);
#pragma unroll
            for (int j = 0; j < 5; ++j) v[45 + 5 * k + j] = t[j];
        }
        static_assert(OBS == 105, "53 dwords per row, the last one half used");
        uint32_t Z[OBS / 2 + 1];
#pragma unroll
        for (int d = 0; d < OBS / 2; ++d) Z[d] = ((uint32_t)v[2 * d] & 0xFFFFu) | ((uint32_t)v[2 * d + 1] << 16);
        Z[OBS / 2] = (uint32_t)v[OBS - 1];
        const uint32_t R = (uint32_t)(SEAT ? E : col), odd = R & 1u;
        const uint32_t sh = odd << 4;
        // the row's first whole dword, as an LDS address the compiler takes as given: the 52 stores are then constant dword offsets from ONE register
        // (left to itself it folds the image's offset in the workgroup's LDS into every store, beyond what a paired store's 8-bit offsets hold,
        // and forms 26 addresses)
        typedef __attribute__((address_space(3))) uint32_t lds_u32;
        lds_u32* ow = (lds_u32*)reinterpret_cast<uint32_t*>(&L.u.O[0]) + ((OBS * R + odd) >> 1);
        asm("" : "+v"(ow));
#pragma unroll
        for (int d = 0; d < OBS / 2; ++d) ow[d] = __builtin_amdgcn_alignbit(Z[d + 1], Z[d], sh);
        L.u.O[OBS * R + (odd ? 0u : (uint32_t)(OBS - 1))] = (int16_t)(odd ? Z[0] : Z[OBS / 2]);
    }
    }   // want_obs
    PHASE(10);

    // ---------------- store state (coalesced)
    // (multi-turn form: the state lives on chip between turns and goes back to HBM after the launch's last turn)
    if (valid && !observe_only && (MULTI ? iter == nturns - 1 : (play || do_reset)) && !ABLATED(32u)) {
        bool store_groups = true;
#ifdef EVG_DIAG      // stale-data test (ablate bit 24): the first chunk of the launch's first set keeps its group words to itself -- the L2 then still holds the
                     // words of the chunk's START, which is what a consumer served from a stale line would read -- but hands on the checksum of the true ones
        if constexpr (CHUNKED) store_groups = !(ABLATED(1u << 24) && io.nsets > 0 && wg_chunk == 0 && wg_set == 0);
#endif
        if (store_groups) {
#pragma unroll
            for (int k = 0; k < 12; ++k) S.grp[(size_t)(P * 12 + k) * N + e] = gw[k];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) S.stamp[(size_t)(P * 3 + j) * N + e] = st[j];
        uint32_t nw_out[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int n = (P ? 7 : 1) + 2 * j;          // word P*3+j holds nodes n (low half) and n+1 (high half; ID 12 does not exist)
            const uint32_t hi = n + 1 <= NN ? (L.NW[(n + 1) % 12][E] & 0xFFFFu) : 0u;
            nw_out[j] = (L.NW[n][E] & 0xFFFFu) | (hi << 16);
            S.node[(size_t)(P * 3 + j) * N + e] = nw_out[j];
        }
        if constexpr (CHUNKED) {
            // chunk hand-over: the checksum of what this lane hands on (recomputed by the lane that takes the set's next chunk over what it loads)
            if (io.nsets > 0) {
                uint32_t hsum = handoff_sum(io.progress_base + (uint32_t)wg_chunk + 1u, gw, st, nw_out, (uint32_t)turn | ((uint32_t)status << 8), episode,
                                            __float_as_uint(ep_ret));
                if (io.gen_actions == 2) hsum = handoff_mix(handoff_mix(handoff_mix(hsum, ag_cycle), ag_swarm), ag_dfs);
                S.handoff[(size_t)P * N + e] = hsum;
            }
        }
        if (P == 0) {
            S.env[e] = (uint32_t)turn | ((uint32_t)status << 8);
            if (MULTI || do_reset) S.episode[e] = episode;
            if (MT) S.mt_pos[e] = mt.pos;
        }
    }
    if (MULTI && envlane) {                             // the next turn of this launch starts from these words
#pragma unroll
        for (int k = 0; k < 12; ++k) L.G[k][lane] = gw[k];
    }
    WAVE_SYNC();             // output image complete
    if constexpr (SEAT) {
        // ---------------- Smart_State features of the caller's seat (evg_step_vs_policy_smart; agents/Smart_State/DQNAgent.py:200-300), compact form: the
        // values evg_smart_state_compact computes from the observation tensor, taken here from the observation IMAGE while it is in LDS -- the learner's next
        // network input leaves the step kernel itself and the 23 us feature kernel (and its read-back of the row) drop out of the turn.  The pair splits
        // the env: the seat's lane writes shared [34] = {turn / 150, 11 x control / 100, 11 x opposing units / 100, 11 x idle allied groups / 12} (:280-286),
        // its partner swarm [12][13] = {one-hot node (11), average health x alive / 1000, in transit} (:288-296).  Every quotient is the float64 product
        // with the rounded reciprocal, rounded once to float32 -- exactly the standalone kernel's arithmetic (side_kernels.inc; exhaustive CPU test).
        if (io.feat_shared) {                                                // (wave-uniform)
            // Staged through the part of the union the one-seat image leaves free (the image is [32][105] int16 = 6 720 B of 14 336) and stored 16 bytes per
            // lane: a lane's own 136 / 624 bytes lie 136 / 624 bytes from its neighbour's -- written straight from registers, the 56 stores of a pair touched
            // 32 lines each and the turn took 12 us longer (measured); staged, 4 passes of <= 6.7 KB.
            constexpr int IMG_BYTES = EPW * OBS * 2;
            static_assert(IMG_BYTES % 16 == 0 && sizeof(L.u) - IMG_BYTES >= (size_t)EPW * 52 * 4 && sizeof(L.u) - IMG_BYTES >= (size_t)EPW * 34 * 4,
                          "the feature staging area behind the one-seat image");
            float* const stg = reinterpret_cast<float*>(reinterpret_cast<char*>(&L.u) + IMG_BYTES);
            const int16_t* r = &L.u.O[E * OBS];
            const bool mine = valid && P == io.seat, partner = valid && P != io.seat;
            // ---- shared [34], by the seat's lane
            if (mine) {
                const uint64_t idle = smart_idle_nibbles(r);             // (the feature values: smart_decode.inc)
                float2* sp = reinterpret_cast<float2*>(stg + E * 34);
#pragma unroll
                for (int j = 0; j < 17; ++j) sp[j] = make_float2(smart_shared_feature(r, 2 * j, idle), smart_shared_feature(r, 2 * j + 1, idle));
            }
            WAVE_SYNC();
            {
                const int n2 = nvalid * 17;                               // float2 pieces of this wave's envs (contiguous in the output)
                const float2* src = reinterpret_cast<const float2*>(stg);
                float2* dst = reinterpret_cast<float2*>(io.feat_shared + (size_t)e0 * 34);
                if (nvalid == EPW) {                                      // whole wave: 272 float4 (e0 is a multiple of 32: 16-byte aligned)
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const int v = lane + WG * i;
                        if (v < EPW * 34 / 4) reinterpret_cast<float4*>(dst)[v] = reinterpret_cast<const float4*>(src)[v];
                    }
                } else {
                    for (int v = lane; v < n2; v += WG) dst[v] = src[v];
                }
            }
            WAVE_SYNC();
            // ---- swarm [12][13], by the partner lane, four swarms per pass
            int loc[NG];
            float hp[NG], mov[NG];
            if (partner) {
#pragma unroll
                for (int k = 0; k < NG; ++k) {
                    loc[k] = r[45 + 5 * k];
                    hp[k] = smart_swarm_health(r, k);
                    mov[k] = (float)r[48 + 5 * k];
                }
            }
#pragma unroll
            for (int pass = 0; pass < 3; ++pass) {
                if (partner) {
                    auto val = [&](int j) -> float {                       // j = 13 swarm + feature, compile-time
                        const int sw = j / 13, f = j - 13 * sw;
                        return smart_swarm_feature(loc[sw], hp[sw], mov[sw], f);
                    };
                    float4* sp = reinterpret_cast<float4*>(stg + E * 52);
#pragma unroll
                    for (int v = 0; v < 13; ++v) sp[v] = make_float4(val(52 * pass + 4 * v), val(52 * pass + 4 * v + 1), val(52 * pass + 4 * v + 2), val(52 * pass + 4 * v + 3));
                }
                WAVE_SYNC();
                const int nv = nvalid * 13;                                // float4 pieces of this pass: 13 per env, 208 contiguous bytes each in the output
                float4* dst = reinterpret_cast<float4*>(io.feat_swarm + (size_t)e0 * (NG * 13)) + 13 * pass;
#pragma unroll
                for (int i = 0; i < (EPW * 13 + WG - 1) / WG; ++i) {
                    const int v = lane + WG * i;
                    if (v < nv) {
                        const int env_ = v / 13, k_ = v - 13 * env_;
                        dst[env_ * 39 + k_] = reinterpret_cast<const float4*>(stg)[v];
                    }
                }
                WAVE_SYNC();
            }
        }
    }
    PHASE(11);

    // ---------------- observation write-out: the wave's 32 x 210 values are contiguous in the output; every lane
    // converts 16 bytes' worth per iteration (conflict-free LDS reads, fully coalesced 1 KiB stores per wave)
    if (want_obs && !ABLATED(16u)) {
        constexpr int EP = 16 / (int)sizeof(OT);          // elements per 16-byte vector
        constexpr int ROW_E = SEAT ? OBS : OBS2;           // values per env in the output
        constexpr int NVEC = (LPW / 2) * ROW_E / EP;
        static_assert((LPW / 2) * ROW_E % EP == 0, "the wave's image is a whole number of 16-byte vectors");
        const int limit = nvalid * ROW_E;
        OT* out = reinterpret_cast<OT*>(io.obs) + (size_t)e0 * ROW_E;
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
            // full workgroup (wave-uniform): straight-line batches of 8 LDS reads, then 8 convert + store, no bounds checks
            constexpr int FULL = NVEC / WG, REM = NVEC % WG, BATCH = 8;
            // Store v of a lane lies v KiB behind its first one: scalar base (the wave's output pointer) + a 32-bit lane offset formed once per batch of eight
            // (`lane * VB + the batch's middle`) + the store's distance from that middle, -4 .. +3 KiB, in the instruction's 13-bit signed immediate.
            // (-DEVG_NO_OBS_BASE, `make noobsbase`: per-store int indexing, three address instructions per store, for the A/B.)
#ifdef EVG_NO_OBS_BASE
            auto dst_of = [&](int v) -> OT* { return out + (lane + v * WG) * EP; };
#else
            constexpr int VB = EP * (int)sizeof(OT);                   // bytes per lane and store
            char* const out_b = reinterpret_cast<char*>(out);          // wave-uniform
            const uint32_t lane_b = (uint32_t)lane * (uint32_t)VB;
            auto dst_of = [&](int v) -> OT* {
                const int mid = (v / BATCH) * BATCH + BATCH / 2;         // the batch's stores lie -4 .. +3 KiB around its middle
                const uint32_t off = lane_b + (uint32_t)(mid * WG * VB);
                return reinterpret_cast<OT*>(out_b + off + (ptrdiff_t)(v - mid) * (WG * VB));
            };
#endif
#pragma unroll
            for (int b0 = 0; b0 < FULL; b0 += BATCH) {
                int vals[BATCH][EP];
#pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    if (b0 + j < FULL) unpack((lane + (b0 + j) * WG) * EP, vals[j]);
#pragma unroll
                for (int j = 0; j < BATCH; ++j)
                    if (b0 + j < FULL) store_obs_vec<OT>(dst_of(b0 + j), vals[j]);
            }
            if (REM && lane < REM) {
                int vals[EP];
                unpack((lane + FULL * WG) * EP, vals);
                store_obs_vec<OT>(dst_of(FULL), vals);
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
    if constexpr (QDEC && !SEAT) {
        // ---------------- Smart_State features of BOTH players (evg_step_smart_q, self-play; agents/Smart_State/DQNAgent.py:200-300), compact form: each lane
        // those of its own observation row, with the values of the one-seat form above (smart_decode.inc).  The two-seat image fills 13 440 B of the union's
        // 14 336, so nothing can be staged behind it: each lane first copies the 59 values of its row that the features read into registers, and once the
        // observation write-out above has read the image, the whole union is the staging area -- shared [2][34] of the wave's envs at once (8 704 B), swarm
        // [2][12][13] in three passes of four swarms (13 312 B) -- stored 16 bytes per lane into outputs that hold the wave's envs contiguously.
        if (io.feat_shared) {                                                // (wave-uniform)
            static_assert(sizeof(L.u) >= (size_t)LPW * 52 * 4 && sizeof(L.u) >= (size_t)LPW * 34 * 4, "the two-seat feature staging area");
            int rv[OBS];                                                     // (only the entries read below stay live)
            {
                const int16_t* r = &L.u.O[col * OBS];
#pragma unroll
                for (int i = 0; i < OBS; ++i) rv[i] = r[i];
            }
            const uint64_t idle = smart_idle_nibbles(rv);
            WAVE_SYNC();                                                     // the image is dead: the union becomes the staging area
            float* const stg = reinterpret_cast<float*>(&L.u);
            const float4* const src = reinterpret_cast<const float4*>(stg);
            if (valid) {
                float2* sp = reinterpret_cast<float2*>(stg + col * 34);      // row col = [env][player]: the output's order
#pragma unroll
                for (int j = 0; j < 17; ++j) sp[j] = make_float2(smart_shared_feature(rv, 2 * j, idle), smart_shared_feature(rv, 2 * j + 1, idle));
            }
            WAVE_SYNC();
            {
                float4* dst = reinterpret_cast<float4*>(io.feat_shared + (size_t)e0 * (2 * 34));     // 272 B per env: 16-byte aligned
                for (int v = lane; v < nvalid * 17; v += WG) dst[v] = src[v];
            }
            WAVE_SYNC();
            float hp[NG], mov[NG];
#pragma unroll
            for (int k = 0; k < NG; ++k) {
                hp[k] = smart_swarm_health(rv, k);
                mov[k] = (float)rv[48 + 5 * k];
            }
#pragma unroll
            for (int pass = 0; pass < 3; ++pass) {
                if (valid) {
                    auto val = [&](int j) -> float {                         // j = 13 swarm + feature, compile-time
                        const int sw = j / 13, f = j - 13 * sw;
                        return smart_swarm_feature(rv[45 + 5 * sw], hp[sw], mov[sw], f);
                    };
                    float4* sp = reinterpret_cast<float4*>(stg + col * 52);
#pragma unroll
                    for (int v = 0; v < 13; ++v) sp[v] = make_float4(val(52 * pass + 4 * v), val(52 * pass + 4 * v + 1), val(52 * pass + 4 * v + 2), val(52 * pass + 4 * v + 3));
                }
                WAVE_SYNC();
                float4* dst = reinterpret_cast<float4*>(io.feat_swarm + (size_t)e0 * (2 * NG * 13)) + 13 * pass;     // 13 float4 per row and pass, rows 39 apart
                for (int v = lane; v < nvalid * 26; v += WG) {
                    const int row = v / 13;
                    dst[row * 39 + (v - 13 * row)] = src[v];
                }
                WAVE_SYNC();
            }
        }
    }
    PHASE(12);

    // ---------------- health of envs that start a new episode: 1600 B each, written by the whole wave
    uint64_t rm = __ballot(do_reset && P == 0);        // do_reset is false on helper lanes
    while (rm) {
        const int l = __ffsll((unsigned long long)rm) - 1;
        rm &= rm - 1;
        double2* dst = reinterpret_cast<double2*>(S.health + (size_t)(e0 + (l >> 1)) * (2 * NU));
        for (int i = lane; i < NU; i += WG) dst[i] = make_double2(100.0, 100.0);
    }
    PHASE(13);
    if (MULTI) WAVE_SYNC();                             // next turn's LDS traffic stays behind this turn's (global accesses of one wave are issued in order)
