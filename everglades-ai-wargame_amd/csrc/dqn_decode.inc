// dqn_decode.inc -- the agents/DQN family's decode of its network output and its exploring draws (include/evg_dqn.h: evg_dqn_actions,
// evg_dqn_get_action), the rules written once: DQNAgent.filter_actions (agents/DQN/DQNAgent.py:161-197) and the random branch of epsilon_greedy
// (:131-159).  The head is 132 wide, Q[group * 11 + node].  Included by evg_kernels.hip inside namespace evg, after minimized_decode.inc (fy_draw,
// rng_half); libevg_dqn.so only.

constexpr int DQ_OUT = NG * NN;           // width of the head: 12 groups x 11 nodes

// filter_actions' seven slots, in registers: every index below is a compile-time constant once the loops are unrolled
struct DqnSlots {
    float best[NA];
    int unit[NA], node[NA];
};

// One (node, group) step of the triple loop (:179-192) with its Q value v: the first slot i whose best_q v exceeds (a NaN exceeds nothing, and neither
// does a v <= 0 an unfilled slot's 0) takes {v, group, node} -- unless the group already stands in one of the seven unit values (an unfilled slot
// counts as unit 0) and slot i is not its own: then the walk goes on to the next slot.  The unit values change only with the store that ends the walk,
// so `group in best_action_units` is one value per step.
__device__ __forceinline__ void dqn_filter_step(DqnSlots& s, float v, int group, int node) {
    // (the two flags that outlive a slot are integers in vector registers, made opaque: as lane masks they would be kept in scalar register pairs
    // across the unrolled walk, which spilled)
    int in_units = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) in_units |= s.unit[i] == group ? 1 : 0;
    asm volatile("" : "+v"(in_units));
    int open = 1;                                      // no slot has taken v yet
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const bool take = open != 0 && v > s.best[i] && (in_units == 0 || s.unit[i] == group);
        s.best[i] = take ? v : s.best[i];
        s.unit[i] = take ? group : s.unit[i];
        s.node[i] = take ? node : s.node[i];
        open = take ? 0 : open;
        asm volatile("" : "+v"(open));
    }
}

// The two keyed Philox blocks of one agent call (minimized_explore_words' blocks, coin and draws: domain RNG_EXPLORE, key (env id, episode, turn, seat))
// -> epsilon_greedy's coin and its random branch, with the reference's two differences: `sample > eps_threshold` is the greedy branch (:149), so the
// env explores iff coin / 2^32 <= eps; and action[:, 1] = np.random.choice(11, 7, replace=False) (:157) is the drawn element itself, 0..10.
// Packed: d.x = explore flag << 31 | 7 node nibbles, d.y = 7 unit nibbles.
__device__ __forceinline__ uint2 dqn_explore_words(const uint4 b0, const uint4 b1, float eps) {
    const uint32_t w0[4] = {b0.x, b0.y, b0.z, b0.w}, w1[4] = {b1.x, b1.y, b1.z, b1.w};
    const uint32_t coin = (rng_half(w0, 7) << 16) | rng_half(w1, 7);
    const bool explore = (double)coin * (1.0 / 4294967296.0) <= (double)eps;              // exact in float64
    uint64_t upool = 0xBA9876543210ull;      // nibble i = i
    uint64_t npool = 0xA9876543210ull;       // nibble i = i: the drawn element is the node
    uint32_t units = 0, nodes = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        units |= fy_draw(upool, rng_half(w0, i), (uint32_t)(NG - i)) << (4 * i);      // action[i, 0] (:156)
        nodes |= fy_draw(npool, rng_half(w1, i), (uint32_t)(NN - i)) << (4 * i);      // action[i, 1] (:157)
    }
    return make_uint2((explore ? 0x80000000u : 0u) | nodes, units);
}
