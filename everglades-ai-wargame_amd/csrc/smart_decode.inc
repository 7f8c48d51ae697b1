// smart_decode.inc -- the Smart_State agent's decode of its network output, network output -> 7 order rows (DQNAgent.get_action / get_best_actions /
// get_random_actions, agents/Smart_State/DQNAgent.py:130-198; Move_Translation.get_move), written once for the kernels that run it: the standalone
// evg_smart_actions_kernel (side_kernels.inc) and the step kernel's Q forms (step_kernel.inc: evg_step_vs_policy_smart_q, one seat; evg_step_smart_q, both).
// Both map one DPP row (16 lanes) to an env, lane = swarm (12 active).  At the end, the compact features of an observation row, shared by the step kernel's
// fused forms.  Included by evg_kernels.hip inside namespace evg.

// Move_Translation.py:3-82 as nibble tables: nibble n = node reached from node n (left, right, up, down, stay); a location outside 1..11 gives node 0 (an
// invalid order)
__device__ __forceinline__ int smart_move(int loc, int dir) {
    const uint64_t tab = dir == 0 ? 0xB7654321311ull << 4 : dir == 1 ? 0xBB9BA987651ull << 4 : dir == 2 ? 0x89887653222ull << 4
                       : dir == 3 ? 0xAAA97654434ull << 4 : 0xBA987654321ull << 4;
    return (loc >= 1 && loc <= NN) ? (int)((tab >> (4 * loc)) & 15ull) : 0;
}

// one swarm's decision (swarm_think, :233-266): its best direction -- torch.argmax / torch.max (:253, :260): the FIRST maximum, a NaN is the maximum
// (torch's rule) -- and the sort key, its best Q (a NaN key has no place in the reference's sort: counted as +inf)
__device__ __forceinline__ float smart_best(const float (&v)[5], int& dir) {
    float best = v[0];
    dir = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k) {
        const bool take = v[k] > best || (v[k] != v[k] && best == best);
        dir = take ? k : dir;
        best = take ? v[k] : best;
    }
    return best != best ? __int_as_float(0x7F800000) : best;
}

// a swarm's place in sorted(decisions) (:189-197: Python's sorted(), stable, ASCENDING): the number of swarms of its DPP row that come before it, counted
// over the 15 rotations of the row (key and swarm id travel together, so nothing depends on the direction of the rotation).  Idle lanes carry +inf with
// ids 12..15: never in front of a swarm.  Every lane of the row must be active.
#define EVG_ROW_ROTATIONS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)
__device__ __forceinline__ int smart_rank(float key, int s) {
    int rank = 0;
    const int kbits = __float_as_int(key);
#define EVG_COUNT_BEFORE(R)                                                                                          \
    {                                                                                                                \
        const float ko = __int_as_float(__builtin_amdgcn_update_dpp(0, kbits, 0x120 + R, 0xF, 0xF, false));          \
        const int io_ = __builtin_amdgcn_update_dpp(0, s, 0x120 + R, 0xF, 0xF, false);                                \
        rank += (ko < key || (ko == key && io_ < s)) ? 1 : 0;                                                         \
    }
    EVG_ROW_ROTATIONS(EVG_COUNT_BEFORE)
#undef EVG_COUNT_BEFORE
    return rank;
}
#undef EVG_ROW_ROTATIONS

// The two keyed Philox blocks of one agent call (oracle/rng_spec.py explore_draws: domain RNG_EXPLORE, key (env id, episode, turn, seat), blocks 0 and 1)
// -> the epsilon coin `random.random() < self.epsilon` (:140-141) and get_random_actions' draws (:148-173): swarms = np.random.choice(12, 7,
// replace=False), directions = np.random.choice(5, 7, replace=True).  Packed as the decode reads them: d0 = explore flag << 31 | 7 x 3-bit directions,
// d1 = 7 swarm nibbles.
__device__ __forceinline__ uint2 smart_explore_words(const uint4 b0, const uint4 b1, float eps) {
    const uint32_t w0[4] = {b0.x, b0.y, b0.z, b0.w}, w1[4] = {b1.x, b1.y, b1.z, b1.w};
    const uint32_t coin = (rng_half(w0, 7) << 16) | rng_half(w1, 7);
    const bool explore = (double)coin * (1.0 / 4294967296.0) < (double)eps;               // exact in float64
    uint64_t pool = 0xBA9876543210ull;
    uint32_t swarms = 0, dirs = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        swarms |= fy_draw(pool, rng_half(w0, i), (uint32_t)(12 - i)) << (4 * i);      // swarms[i] (:157)
        dirs |= ((rng_half(w1, i) * 5u) >> 16) << (3 * i);                            // directions[i] (:159)
    }
    return make_uint2((explore ? 0x80000000u : 0u) | dirs, swarms);
}

// the random branch for swarm s (get_random_actions, :160-171): its row index among the seven drawn (NA: not drawn) and, if drawn, its direction
__device__ __forceinline__ int smart_explore_rank(const uint2 d, int s, int& dir) {
    int rank = NA;
#pragma unroll
    for (int i = 0; i < NA; ++i)
        if ((int)((d.y >> (4 * i)) & 15u) == s) { rank = i; dir = (int)((d.x >> (3 * i)) & 7u); }
    return rank;
}

// ---- the agent's next input: the compact Smart_State features of one observation row (DQNAgent.py:200-300; evg_smart_state_compact's values), as the
// step kernel's fused forms compute them -- the one-seat form (evg_step_vs_policy_smart) from the row in LDS, the two-seat Q form (evg_step_smart_q) from a
// copy of it in registers.  `r` is anything indexed like the row [105]; every index below is a compile-time constant at each call.  Every quotient is the
// float64 product with the rounded reciprocal, rounded once to float32: exactly the standalone kernel's arithmetic (side_kernels.inc).
// nibble n: groups listed at node n (own numbering) that are not in transit (:200-213)
template <typename R>
__device__ __forceinline__ uint64_t smart_idle_nibbles(const R& r) {
    uint64_t idle = 0;
#pragma unroll
    for (int k = 0; k < NG; ++k) idle += (uint64_t)(r[48 + 5 * k] == 0 ? 1u : 0u) << (4 * (r[45 + 5 * k] & 15));
    return idle;
}
// shared[j], j < 34: {turn / 150, 11 x control / 100, 11 x opposing units / 100, 11 x idle allied groups / 12} (:280-286)
template <typename R>
__device__ __forceinline__ float smart_shared_feature(const R& r, int j, uint64_t idle) {
    if (j == 0) return (float)((double)r[0] * (1.0 / 150.0));
    if (j < 12) return (float)((double)r[3 + 4 * (j - 1)] * (1.0 / 100.0));
    if (j < 23) return (float)((double)r[4 + 4 * (j - 12)] * (1.0 / 100.0));
    return (float)((double)(int)((idle >> (4 * (j - 22))) & 15ull) * (1.0 / 12.0));
}
// swarm[k][f], f < 13: {one-hot node (11), average health x alive / 1000, in transit} (:288-296), from the swarm's location, health term and transit flag
template <typename R>
__device__ __forceinline__ float smart_swarm_health(const R& r, int k) { return (float)((double)((int)r[47 + 5 * k] * (int)r[49 + 5 * k]) * (1.0 / 1000.0)); }
__device__ __forceinline__ float smart_swarm_feature(int loc, float hp, float mov, int f) { return f < NN ? (loc == f + 1 ? 1.f : 0.f) : (f == NN ? hp : mov); }
