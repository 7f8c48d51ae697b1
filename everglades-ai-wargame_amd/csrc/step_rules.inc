// step_rules.inc -- the game rules of one turn, written once for both lane mappings of the step kernel (the two-lane fragments step_orders /
// step_combat / step_move_capture / step_outputs .inc and the four-lane evg_step4.inc).  Every function is pure in registers: no LDS, no global
// memory, no cross-lane operation.  What stays in the kernels is what depends on the mapping: which lane owns which groups, nodes and rows, the DPP
// exchanges, the LDS layouts and the load / store schedules.  Each function cites the reference lines it implements.  The rules are written
// branch-free -- `&` on bools, both arms of a select computed --: inlined, short-circuit forms of them compile to divergent branches, each with its
// own exec-mask region.
// Included by evg_kernels.hip inside namespace evg (not a translation unit of its own).

// ---------------- node words: control sign + 512 in bits 0..9, controlledBy + 1 in bits 10..11 (0 = nobody)
__device__ __forceinline__ int node_cs(uint32_t nw) { return (int)(nw & 0x3FFu) - 512; }
__device__ __forceinline__ uint32_t node_cb1(uint32_t nw) { return (nw >> 10) & 3u; }

// ---------------- orders (server.py:218-271)
// The node map of a player as one nibble table (nibble n = the board's node n in that player's numbering; identity for player 0, p1_node_map
// for player 1: :92, :233-234, :437-439, :485-486): every lookup is then the same straight-line shift, not a divergent `P ? map[n] : n`.
__device__ __forceinline__ uint64_t player_node_map(int P, uint64_t p1nib) { return P ? p1nib : 0xBA9876543210ull; }
__device__ __forceinline__ uint32_t map_node(uint64_t map, uint32_t n) { return (uint32_t)((map >> (4 * n)) & 15u); }
// Domain of one order row: ids in [-12, 11] behave like the reference's Python lists (a negative index counts from the end: groups[gid] at :235,
// p1_node_map[nid] at :92 for player 1); for player 0 a negative node id matches no connection; anything else would raise in the reference and is an
// invalid order here.  Returns whether the row is valid; gid becomes the group, nid the node in the board's numbering (:233-234), raw the id as
// used_swarms keeps it (:241, :252: gid + 12).
__device__ __forceinline__ bool order_ids(int& gid, int& nid, int& raw, uint64_t node_map, int P) {
    const bool ok = (gid >= -12) & (gid < 12) & (nid >= (P ? -12 : 0)) & (nid < 12);
    raw = ok ? gid + 12 : 0;
    gid = ok ? (gid < 0 ? gid + 12 : gid) : 0;
    nid = (int)map_node(node_map, (uint32_t)(ok ? (nid < 0 ? nid + 12 : nid) : 0));
    return ok;
}
// distance of the ordered node from the group's location, 0 = not adjacent (adj_row = the location's row of the adjacency table; :245-250)
__device__ __forceinline__ uint32_t order_dist(uint64_t adj_row, uint32_t node) { return (uint32_t)((adj_row >> (4 * node)) & 15u); }
// the order is taken when the group is not already moving (:243) and the node is adjacent (:245-250)
__device__ __forceinline__ bool order_accepted(uint32_t w, uint32_t dist) { return (((w & G_MODE_M) >> G_MODE_S) != MODE_MOVING) & (dist != 0); }
// the ordered group: destination, distance, ready to move (:267-270)
__device__ __forceinline__ uint32_t ordered_word(uint32_t w, uint32_t node, uint32_t dist) {
    return (w & ~(G_DEST_M | G_DIST_M | G_MODE_M)) | (node << G_DEST_S) | (dist << G_DIST_S) | (MODE_READY << G_MODE_S);
}

// ---------------- combat damage (server.py:592-609)
// which quotient a hit on a group of unit type `type` at `node` takes: the node's defence applies to the side that controls it (:592-597; the
// fortress bonus of :595-597 is dead code in the reference)
__device__ __forceinline__ int damage_index(uint32_t type, uint32_t nw, int side, int node) {
    return (int)type * 12 + (node_cb1(nw) == (uint32_t)(side + 1) ? node : 0);
}
// the damage byte of the unit of rank `rank` (< 8) among a group's alive units: one v_perm_b32 (selector = rank, the other three selector bytes 0x0C =
// constant zero) from the group's run of damage bytes a0 (bytes 0..3), a1 (4..7)
__device__ __forceinline__ uint32_t damage_byte(uint32_t a0, uint32_t a1, uint32_t rank) { return __builtin_amdgcn_perm(a1, a0, rank | 0x0C0C0C00u); }
// ... of any rank of the 12-unit group (a2: bytes 8..11)
__device__ __forceinline__ uint32_t damage_byte12(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t rank) {
    const uint32_t lo = damage_byte(a0, a1, rank), hi = __builtin_amdgcn_perm(0u, a2, (rank - 8u) | 0x0C0C0C00u);
    return rank < 8u ? lo : hi;
}
// rank of unit slot sl among the group's alive slots
__device__ __forceinline__ uint32_t unit_rank(uint32_t mask, int sl) { return (uint32_t)__popc(mask & ((1u << sl) - 1u)); }
// One unit takes damage d: health -= 10 * d / defence-adjusted denominator (:601, :609), clamped at 0 = dead (:615-618).  FAST (DevTables::fast_div, a
// wave-uniform choice of the tables): the quotient from the rounded reciprocal and one fma correction, equal to the IEEE quotient for every table
// the host accepts for it.  A slot whose unit is already dead may pick another unit's byte: harmless, its health is 0.0 and stays 0.0.
template <bool FAST>
__device__ __forceinline__ bool unit_hit(double& h, uint32_t d, double denom, double rcp) {
    double loss;
    if constexpr (FAST) {
        const double a = (double)__umul24(10u, d);                            // exact, like 10. * tgt_dmg (d is one byte)
        const double q0 = a * rcp;
        loss = __builtin_fma(__builtin_fma(-denom, q0, a), rcp, q0);          // == a / denom
    } else {
        loss = (10.0 * (double)d) / denom;                                    // :601
    }
    const double hv = h - loss;                                               // :609
    const bool dead = hv <= 0.0;                                              // :615-618
    h = dead ? 0.0 : hv;
    return dead;
}
// Unit slots s0 .. s0 + N - 1 of a group (h[j] = the health of slot s0 + j; N = 12: the whole row, slots 8..11 only when `twelve`, the 12-unit group;
// N = 4: half of an 8-unit row) with alive mask `mask` and the damage bytes of its alive units a0..a2 in rank order.  Returns the mask of the slots
// that died.  The callers choose FAST (wave-uniform) through a generic lambda, `if (fast) f(true_type) else f(false_type)`: two direct calls of the
// two instantiations cost the two-lane kernel 18 more VGPRs.
template <bool FAST, int N>
__device__ __forceinline__ uint32_t hit_slots(double (&h)[N], int s0, bool twelve, uint32_t mask, uint32_t a0, uint32_t a1, uint32_t a2, double denom,
                                              double rcp) {
    uint32_t dead = 0;
#pragma unroll
    for (int j = 0; j < (N < 8 ? N : 8); ++j) {                               // rank <= slot < 8: bytes of a0, a1
        const int sl = s0 + j;
        dead |= unit_hit<FAST>(h[j], damage_byte(a0, a1, unit_rank(mask, sl)), denom, rcp) ? 1u << sl : 0u;
    }
    if constexpr (N == 12) {
        if (twelve) {
#pragma unroll
            for (int sl = 8; sl < 12; ++sl) dead |= unit_hit<FAST>(h[sl], damage_byte12(a0, a1, a2, unit_rank(mask, sl)), denom, rcp) ? 1u << sl : 0u;
        }
    }
    return dead;
}
// the summed health of a group's row in numpy's pairwise order (np.sum at :481): np_sum8 of slots 0..7, then -- the 12-unit group only -- the tail
// 8..11 sequentially (the callers add the tail inside their own `gid == 11` block, next to the stores of slots 8..11: a second block measured 2 % slower)
__device__ __forceinline__ double health_sum_tail(double s8, const double (&h)[12]) { return (((s8 + h[8]) + h[9]) + h[10]) + h[11]; }
// the group word after combat: the surviving units and their average health, truncated like int(np.sum / alive) (:491)
__device__ __forceinline__ uint32_t hit_word(uint32_t w, uint32_t newmask, double sum) {
    const int alive = __popc(newmask);
    const uint32_t avg = alive ? (uint32_t)(int)(sum / (double)alive) : 0u;
    return (w & ~(G_MASK_M | G_AVG_M)) | (newmask << G_MASK_S) | (avg << G_AVG_S);
}

// ---------------- movement of one group word (server.py:656-706), branch-free: spd = the group's speed.  Sets `arrive` when the group reaches its
// destination this turn (the caller stamps the arrival turn where it keeps the stamps).
__device__ __forceinline__ uint32_t move_group(uint32_t w, uint32_t spd, bool& arrive) {
    static_assert(MODE_READY == 1 && MODE_MOVING == 2, "ready -> moving is +1 in the mode field; bit 1 of the field is `moving`");
    const uint32_t spd_d = spd << G_DIST_S;                                   // aligned with the distance field
    const bool alive = (w & G_MASK_M) != 0;                                   // not destroyed, :663
    const bool ready = alive && (w & G_MODE_M) == (MODE_READY << G_MODE_S);
    const bool moving = alive && (w & (MODE_MOVING << G_MODE_S)) != 0;
    arrive = moving && (w & G_DIST_M) <= spd_d;                               // :671, :678-695
    const uint32_t w_arrive = (w & ~(G_LOC_M | G_DEST_M | G_DIST_M | G_MODE_M)) | ((w & G_DEST_M) >> G_DEST_S);
    uint32_t nw = ready ? w + (1u << G_MODE_S) : w;                          // :664-667: moves from the next turn on
    nw = moving ? w - spd_d : nw;                                             // in transit: distance_remaining -= speed (> 0 left)
    return arrive ? w_arrive : nw;
}

// ---------------- per-node aggregates (post-movement)
// one group's contribution to its side's word at its node: capture points of units that are not in transit (:720) | units listed << 16
__device__ __forceinline__ uint32_t node_contribution(uint32_t w, int cnt, uint32_t ctl) {
    const bool elig = ((w & G_MODE_M) >> G_MODE_S) != MODE_MOVING;
    return (elig ? (uint32_t)cnt * ctl : 0u) | ((uint32_t)cnt << 16);
}
// ... and to its side's unit score (:315-317)
__device__ __forceinline__ int unit_score(int cnt, uint32_t cst) { return cnt * (int)cst; }

// ---------------- capture (server.py:708-767) and node score (:297-310) of one node: nw = its word, pts0 / pts1 = the two sides' capture points there
// (low halves of the aggregate words), cp / ts = its control points / the player whose base it is (-1: none), real = the node exists
struct NodeTurn {
    uint32_t nw;           // the node word after the turn (unchanged when nothing is captured)
    bool base_cap;         // a base held by the other player (:299-304)
    int part0, part1;      // the node's contributions to the scores of player 0 / player 1
};
__device__ __forceinline__ NodeTurn capture_node(uint32_t nw, int pts0, int pts1, int cp, int ts, bool real, bool play) {
    int cs = node_cs(nw);
    uint32_t cb1 = node_cb1(nw);
    const bool c0 = pts0 > 0, c1 = pts1 > 0;                               // ctr >= 1 (control >= 1)
    const uint32_t pid1 = c0 ? 1u : 2u;                                    // capturing player + 1
    const bool capture = real && play && (c0 != c1) && (abs(cs) < cp || pid1 != cb1);   // :729-732
    const int cs2 = cs + (pts0 - pts1);                                    // :748 (turn > 0 here): exactly one of the two is non-zero
    const bool neutralize = (cs ^ cs2) < 0;                                // :747-750: the sign bit changed
    const bool full = abs(cs2) >= cp;                                      // :763-765
    const uint32_t cb1n = neutralize ? 0u : (full ? pid1 : cb1);           // :766-767
    const int csn = full ? (c0 ? cp : -cp) : cs2;
    cs = capture ? csn : cs;
    cb1 = capture ? cb1n : cb1;
    NodeTurn r;
    r.nw = (uint32_t)(cs + 512) | (cb1 << 10);
    r.base_cap = real && ts != -1 && cb1 != 0u && (int)cb1 != ts + 1;     // :299-304
    const int acs = abs(cs);
    const int pts = real ? acs + (acs == cp ? cp : 0) : 0;                 // :305-310
    r.part0 = (r.base_cap && cb1 == 1u ? 1000 : 0) + (cs > 0 ? pts : 0);
    r.part1 = (r.base_cap && cb1 == 2u ? 1000 : 0) + (cs < 0 ? pts : 0);
    return r;
}

// ---------------- status precedence TimeExpired > Annihilation > BaseCapture (server.py:321-328), as selects: three nested divergent branches otherwise
__device__ __forceinline__ int status_after_turn(int status, int turn, int max_turns, int alive_both, bool base_cap) {
    return turn >= max_turns ? EVG_TIME_EXPIRED : (alive_both == 0 ? EVG_ANNIHILATION : (base_cap ? EVG_BASE_CAPTURE : status));
}

// ---------------- reward / done / winner (everglades_env.py:37-61, evaluate.py:155-160)
struct TurnOutcome {
    float rew0, rew1;
    int winner;
};
__device__ __forceinline__ TurnOutcome turn_outcome(bool done, int score0, int score1) {
    TurnOutcome o;
    o.winner = EVG_WINNER_NONE;
    if (done) {
        o.winner = score0 > score1 ? EVG_WINNER_P0 : (score1 > score0 ? EVG_WINNER_P1 : EVG_WINNER_TIE);
        o.rew0 = score0 > score1 ? 1.f : 0.f;
        o.rew1 = score1 > score0 ? 1.f : (score0 > score1 ? -1.f : 0.f);
    } else {
        // scores[p] / 3700 (everglades_env.py:63-64) rounded to the float32 the reward tensor holds: the product with the rounded
        // reciprocal differs from the float64 quotient by an ulp of float64 at most, which never crosses a float32 rounding
        // boundary for an integer score below 2^22 (checked exhaustively: tests/test_abi_and_host.py)
        constexpr double kInvMaxScore = 1.0 / (double)EVG_MAX_SCORE;
        o.rew0 = (float)((double)score0 * kInvMaxScore);
        o.rew1 = (float)((double)score1 * kInvMaxScore);
    }
    return o;
}

// ---------------- observation values (board_state :382-455, player_state :457-501, everglades_env.py:158-171)
// the four board values of one node: its DEFENSE and OBSERVE flags (:442-443; LdsTables::res holds them as shown), the control sign (not mirrored
// for player 1) and the opposing units listed there, moving ones included (:446-449)
__device__ __forceinline__ void obs_node(int (&v)[4], int res, uint32_t nw, int opp_units) {
    v[0] = res & 0xFFFF;
    v[1] = res >> 16;
    v[2] = node_cs(nw);
    v[3] = opp_units;
}
// the five values of one group row (:485-493): location in the player's numbering, unit type, average health, in transit, alive units
__device__ __forceinline__ void obs_group(int (&v)[5], uint32_t w, uint64_t node_map, uint32_t type, int cnt) {
    static_assert(MODE_MOVING == 2 && MODE_READY == 1 && MODE_IDLE == 0, "bit 1 of the mode field is the `moving` flag");
    v[0] = (int)map_node(node_map, w & G_LOC_M);
    v[1] = (int)type;
    v[2] = (int)((w & G_AVG_M) >> G_AVG_S);
    v[3] = (int)((w >> (G_MODE_S + 1)) & 1u);
    v[4] = cnt;
}
