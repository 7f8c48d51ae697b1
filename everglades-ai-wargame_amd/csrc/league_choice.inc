// league_choice.inc -- the opponent league's two device functions (include/evg.h, evg_league): the member draw and the object swap.  Both the step kernel's
// league forms (step_move_capture.inc, the reset branch) and evg_league_assign / evg_league_clear (league_kernels.inc) call them, so the rule is written once.
// Included by evg_kernels.hip inside namespace evg, ahead of the step kernel.
// ---------------------------------------------------------------------------------------------
// random.choices(range(M), weights)[0] restated on a keyed draw (DESIGN.md section 4, domain 5 = RNG_LEAGUE; tests/league_model.py is the host statement):
//   cum_weights = list(accumulate(weights)); total = cum_weights[-1] + 0.0; bisect(cum_weights, random() * total, 0, M - 1)
// with random() = word .x of the block (domain 5, block 0, turn 0, node 0, player, group 0, episode, env id) as a fraction of 2^32: a 32-bit uniform stands in
// for random.random()'s 53 bits, as the delay coin of random_actions_delay does (step_agents.inc).  float64 sums left to right (the build contracts nothing).
// total <= 0 or not finite -- the reference raises ValueError -- keeps `keep` and sets `bad`.  The weights are read twice (the total, then the running sums
// again) instead of being held in up to 32 registers: this runs once per episode and env.
__device__ __forceinline__ int league_choice(uint32_t seed_lo, uint32_t seed_hi, uint32_t env_id, uint32_t episode, int player, const double* weights, int M,
                                             int keep, bool& bad) {
    double total = weights[0];
    for (int j = 1; j < M; ++j) total = total + weights[j];
    total = total + 0.0;
    if (!(total > 0.0) || total == __longlong_as_double(0x7FF0000000000000ll)) {
        bad = true;
        return keep;
    }
    const uint4 b = rng_block(seed_lo, seed_hi, env_id, episode, RNG_LEAGUE, 0u, 0, 0, player, 0);
    const double x = ((double)b.x / 4294967296.0) * total;
    double cum = weights[0];
    int m = 0;
    for (int j = 0; j < M - 1; ++j) {
        if (j) cum = cum + weights[j];
        m += cum <= x ? 1 : 0;
    }
    return m;
}

// the member of env e changes from m_old to m_new: the live agent words go to m_old's slot of the store [M][3][N], m_new's are loaded into them
__device__ __forceinline__ void league_swap(uint32_t* objects, size_t N, size_t e, int m_old, int m_new, uint32_t& cycle, uint32_t& swarm, uint32_t& dfs) {
    uint32_t* const o = objects + (size_t)m_old * 3 * N + e;
    const uint32_t* const n = objects + (size_t)m_new * 3 * N + e;
    o[0] = cycle; o[N] = swarm; o[2 * N] = dfs;
    cycle = n[0]; swarm = n[N]; dfs = n[2 * N];
}

// a fresh agent object: what evg_scripted_reset writes (side_kernels.inc)
constexpr uint32_t kAgentFreshCycle = 0x112u, kAgentFreshSwarm = 0xBA875421u, kAgentFreshDfs = 0u;
