// league_kernels.inc -- the small kernels of the opponent league (include/evg.h, evg_league): clear, assign after an explicit reset, importance weights.
// The draw and the swap are league_choice.inc's, shared with the step kernel's league forms.  Included by evg_kernels.hip inside namespace evg.
struct LeagueArgs {              // evg_league as the kernels take it
    const double* weights;
    uint8_t* assign;
    uint32_t* objects;
    unsigned long long* counts;
    unsigned long long* ctl;
    int32_t num, seat, resample;
};

// draw (and swap) for one env and its CURRENT episode; `fresh`: every stored object has just been made fresh, so is the live one (evg_league_clear)
__device__ __forceinline__ void league_assign_env(const DevState& S, const LeagueArgs& g, int e, bool fresh) {
    const size_t N = (size_t)S.N;
    uint32_t raw = g.assign[e];
    if (raw >= (uint32_t)g.num) {
        if (!fresh) atomicOr(g.ctl, (unsigned long long)EVG_LEAGUE_S_BAD_ASSIGN);      // (clear: assign holds nothing yet)
        raw = 0u;
    }
    const int m_old = (int)raw, player = 1 - g.seat;
    bool bad = false;
    const int m_new = league_choice(S.seed_lo, S.seed_hi, S.env_id_base + (uint32_t)e, S.episode[e], player, g.weights, g.num, m_old, bad);
    if (bad) atomicOr(g.ctl, (unsigned long long)EVG_LEAGUE_S_BAD_WEIGHTS);
    if (fresh) {
        g.assign[e] = (uint8_t)m_new;
    } else if (m_new != m_old) {
        const size_t ai = (size_t)player * N + e;
        uint32_t c = S.agent_cycle[ai], s = S.agent_swarm[ai], d = S.agent_dfs[ai];
        league_swap(g.objects, N, (size_t)e, m_old, m_new, c, s, d);
        S.agent_cycle[ai] = c; S.agent_swarm[ai] = s; S.agent_dfs[ai] = d;
        g.assign[e] = (uint8_t)m_new;
    }
}

// counts and ctl are zeroed by a memset ahead of this kernel (launch_league_clear)
__global__ void __launch_bounds__(256) evg_league_clear_kernel(DevState S, LeagueArgs g) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S.N) return;
    const size_t N = (size_t)S.N;
    for (int m = 0; m < g.num; ++m) {
        uint32_t* const o = g.objects + (size_t)m * 3 * N + e;
        o[0] = kAgentFreshCycle; o[N] = kAgentFreshSwarm; o[2 * N] = kAgentFreshDfs;
    }
    const size_t ai = (size_t)(1 - g.seat) * N + e;
    S.agent_cycle[ai] = kAgentFreshCycle; S.agent_swarm[ai] = kAgentFreshSwarm; S.agent_dfs[ai] = kAgentFreshDfs;
    if (g.resample) league_assign_env(S, g, e, true);
}

__global__ void __launch_bounds__(256) evg_league_assign_kernel(DevState S, LeagueArgs g, const uint8_t* mask) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S.N || (mask && !mask[e])) return;
    league_assign_env(S, g, e, false);
}

// updateAgentWeights (dqn_smart_state_cycled_training_with_importance.py:166-173): 1.0 where games == 0, else 1.0 - wins / games + 0.05 in float64
__global__ void __launch_bounds__(WG) evg_league_importance_kernel(LeagueArgs g, double* out) {
    const int m = threadIdx.x;
    if (m >= g.num) return;
    const unsigned long long games = g.counts[4 * m], wins = g.counts[4 * m + 1];
    out[m] = games == 0ull ? 1.0 : (1.0 - (double)wins / (double)games) + 0.05;
}
