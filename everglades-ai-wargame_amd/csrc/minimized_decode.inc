// minimized_decode.inc -- the Minimized agent's decode of its network output, network output -> 7 order rows (DQNAgent.get_action / get_best_actions /
// get_random_actions / swarm_think, agents/Minimized/DQNAgent.py:121-242), written once for the kernels that run it: the standalone
// evg_minimized_actions_kernel (side_kernels.inc) and the step kernel's 11-way Q forms (step_kernel.inc: evg_step_vs_policy_minimized_q,
// evg_step_vs_league_minimized_q).  The network's head is 11 wide, one Q per NODE: a swarm's order is {swarm, argmax + 1} in the caller's own numbering --
// no Move_Translation, no location lookup, no observation.  Mapping and ordering are smart_decode.inc's (one DPP row per env, lane = swarm, smart_rank).
// Included by evg_kernels.hip inside namespace evg, after smart_decode.inc.

constexpr int MIN_Q = NN;                 // width of the head: one Q value per node

// one swarm's decision (swarm_think, :215-242): torch.argmax + 1 / torch.max (:233-235) with smart_best's rules -- the FIRST maximum, a NaN is the maximum,
// and as a sort key a NaN counts as +inf
__device__ __forceinline__ float minimized_best(const float (&v)[MIN_Q], int& node) {
    float best = v[0];
    int arg = 0;
#pragma unroll
    for (int k = 1; k < MIN_Q; ++k) {
        const bool take = v[k] > best || (v[k] != v[k] && best == best);
        arg = take ? k : arg;
        best = take ? v[k] : best;
    }
    node = arg + 1;
    return best != best ? __int_as_float(0x7F800000) : best;
}

// The two keyed Philox blocks of one agent call (the Smart_State call's: domain RNG_EXPLORE, key (env id, episode, turn, seat), blocks 0 and 1) -> the
// epsilon coin `random.random() < self.epsilon` (:133-134) and get_random_actions' draws (:141-153): swarms = np.random.choice(12, 7, replace=False) from
// halves 0..6 of block 0, nodes = np.random.choice(11, 7, replace=False) + 1 from halves 0..6 of block 1, both partial Fisher-Yates.  Packed as the decode
// reads them: d.x = explore flag << 31 | 7 node nibbles, d.y = 7 swarm nibbles.
__device__ __forceinline__ uint2 minimized_explore_words(const uint4 b0, const uint4 b1, float eps) {
    const uint32_t w0[4] = {b0.x, b0.y, b0.z, b0.w}, w1[4] = {b1.x, b1.y, b1.z, b1.w};
    const uint32_t coin = (rng_half(w0, 7) << 16) | rng_half(w1, 7);
    const bool explore = (double)coin * (1.0 / 4294967296.0) < (double)eps;               // exact in float64
    uint64_t spool = 0xBA9876543210ull;      // nibble i = i
    uint64_t npool = 0xBA987654321ull;       // nibble i = i + 1: the drawn element is already the node
    uint32_t swarms = 0, nodes = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        swarms |= fy_draw(spool, rng_half(w0, i), (uint32_t)(12 - i)) << (4 * i);     // actions[i, 0] (:150)
        nodes |= fy_draw(npool, rng_half(w1, i), (uint32_t)(MIN_Q - i)) << (4 * i);   // actions[i, 1] (:151)
    }
    return make_uint2((explore ? 0x80000000u : 0u) | nodes, swarms);
}

// the random branch for swarm s: its row index among the seven drawn (NA: not drawn) and, if drawn, its node
__device__ __forceinline__ int minimized_explore_rank(const uint2 d, int s, int& node) {
    int rank = NA;
#pragma unroll
    for (int i = 0; i < NA; ++i)
        if ((int)((d.y >> (4 * i)) & 15u) == s) { rank = i; node = (int)((d.x >> (4 * i)) & 15u); }
    return rank;
}

// One lane's part of an env's decode: swarm s of the DPP row reads its 11 Q values -- 44 contiguous bytes, the row's 12 lanes 528 -- straight from the
// caller's tensor (qs: the env's [12][11] block; live: the lane holds a swarm of an env that exists), ranks itself among the row's swarms and, where the
// env explores (d: its minimized_explore_words), takes its place among the seven drawn instead.  Returns the row index (>= NA: the swarm gives no order)
// and the node.  Every lane of the DPP row must be active.
__device__ __forceinline__ int minimized_decide(const float* __restrict__ qs, bool live, bool env_live, int s, const uint2 d, int& node) {
    float key = __int_as_float(0x7F800000);                  // idle lanes: +inf with ids 12..15, never in front of a swarm
    node = 0;
    if (live) {
        float v[MIN_Q];
#pragma unroll
        for (int k = 0; k < MIN_Q; ++k) v[k] = qs[s * MIN_Q + k];
        key = minimized_best(v, node);
    }
    int rank = smart_rank(key, s);                           // sorted(..., key=best_q_value)[:7] (:168-177): ascending, stable
    if (env_live && (d.x >> 31)) rank = minimized_explore_rank(d, s, node);
    return rank;
}
