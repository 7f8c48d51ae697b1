// step_agents.inc -- the scripted opponents of agents/State_Machine/ as ONE device function over a small "view" (SURVEY 8 f1, BASELINE config 5).
// Included by evg_kernels.hip inside namespace evg.
// ---------------------------------------------------------------------------------------------
// scripted opponents (SURVEY 8 f1, BASELINE config 5): all bots of agents/State_Machine/, one agent object per
// (env, player) that lives across episodes like the reference's (evaluate.py:85-93).  The logic is written against a
// small "view" of what the bots read from their observation (turn, own group locations in own numbering, own moving
// flags, control state and opposing units of a board slot), so that the same code serves the standalone kernel (view =
// the observation tensor) and the fused rollout (view = the on-chip state at the start of the turn, which is what the
// observation of the previous turn was built from).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void cycle_advance(int& group_num, int& node_num) {
    group_num = (group_num + 1) % NG;
    if (group_num == 0) node_num = node_num % NN + 1;
}

// the routing tables the bots index: in the step kernel they come from the LDS copy (a load from the global table would be a
// per-lane vector load -- the kernel stores to global memory, so the compiler cannot keep it scalar -- and waiting for it
// means vmcnt(0): for the previous turn's observation stores as well)
struct AgentTabs {
    uint64_t maxnbr, tar1, tar11;       // DevTables::maxnbr_nib, tar_to_1, tar_to_11
    const DevTables* T;                 // dfs_attack's order sequence stays in global memory (that bot only)
};

template <class View>
__device__ __forceinline__ void agent_rows(int policy, const View& v, const AgentTabs& tabs, uint32_t seed_lo, uint32_t seed_hi, uint32_t env_id,
                                           uint32_t episode, int player, bool commit, bool active, uint32_t* p_cycle, uint32_t* p_swarm, uint32_t* p_dfs,
                                               int2 (&rows)[NA]) {
    // `commit` is false for the padding lanes of a partial last workgroup (they compute like everyone else but must not
    // advance the agent state of the env their indices are clamped to) and for a finished, not yet reset game: the harness
    // has left that game's loop (evaluate.py:147-152), its agents are not consulted -- zero rows, state untouched
    const int turn = v.turn();
#pragma unroll
    for (int i = 0; i < NA; ++i) rows[i] = make_int2(0, 0);                   // np.zeros(shape)
    if (!active) return;
    // cycling state shared by most bots: first_turn << 8 | group_num << 4 | node_num | strat_index << 9 | agentNumber==2 << 13
    const uint32_t cst = *p_cycle;
    int first = (int)((cst >> 8) & 1u), group_num = (int)((cst >> 4) & 15u), node_num = (int)(cst & 15u);
    int strat = (int)((cst >> 9) & 15u), agent2 = (int)((cst >> 13) & 1u);
    bool cyc_dirty = false;

    if (policy == EVG_POLICY_RANDOM || policy == EVG_POLICY_RANDOM_DELAY) {
        // random_actions.py:38-46, random_actions_2.py; random_actions_delay.py acts only when random.random() > 0.68
        bool go = true;
        if (policy == EVG_POLICY_RANDOM_DELAY) {
            const uint4 x = rng_block(seed_lo, seed_hi, env_id, episode, RNG_DELAY, 0u, turn, 0, player, 0);
            go = (double)x.x / 4294967296.0 > 0.68;
        }
        if (go) gen_random_rows(seed_lo, seed_hi, env_id, episode, turn, player, rows);
    } else if (policy == EVG_POLICY_CYCLE_RUSH_25 || policy == EVG_POLICY_CYCLE_RUSH_50 || policy == EVG_POLICY_BASE_RUSH_V1 ||
               policy == EVG_POLICY_ALL_CYCLE) {
        // cycle_rush_turn25.py:62-115 (gate 25 / 50), base_rush_v1.py:62-96 (row i only while group i is not at node 11),
        // all_cycle.py (always)
        const int gate = policy == EVG_POLICY_CYCLE_RUSH_25 ? 25 : 50;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int loc_i = v.loc(i);
            bool issue = !first;
            if (policy == EVG_POLICY_CYCLE_RUSH_25 || policy == EVG_POLICY_CYCLE_RUSH_50) issue = issue && ((loc_i != 11 && turn > gate) || turn < gate);
            if (policy == EVG_POLICY_BASE_RUSH_V1) issue = issue && loc_i != 11;
            if (issue) { rows[i] = make_int2(group_num, node_num); cycle_advance(group_num, node_num); }
        }
        first = 0; cyc_dirty = true;
    } else if (policy == EVG_POLICY_BULL_RUSH) {                           // bull_rush.py: all groups to 2, 2, 5, 5, 8, 8, 11, 11, ...
        if (!first) {
            if (strat == 8) strat = 0;
            const int node = (int)((0xB852u >> (4 * (strat >> 1))) & 15u);   // node_strat = [2, 5, 8, 11]
#pragma unroll
            for (int i = 0; i < NA; ++i) { rows[i] = make_int2(group_num, node); group_num = (group_num + 1) % NG; }
            strat += 1;
        }
        first = 0; cyc_dirty = true;
    } else if (policy >= EVG_POLICY_CYCLE_TARGET_NODE && policy <= EVG_POLICY_CYCLE_TARGET_NODE11P2) {
        // cycle_target_node.py (target 11, level 75), ..._node1.py (1, 75), ..._node11.py (11, 500), ..._node11P2.py (11, +-500)
        const int tar = policy == EVG_POLICY_CYCLE_TARGET_NODE1 ? 1 : 11, level = policy >= EVG_POLICY_CYCLE_TARGET_NODE11 ? 500 : 75;
        if (first) {
            if (policy == EVG_POLICY_CYCLE_TARGET_NODE11P2 && v.opp_units_slot(11) > 0) agent2 = 1;    // obs[44]
        } else {
            const int ctl = v.ctrl_slot(tar);                                                          // obs[tarNode * 4 - 1]
            const bool controlled = (policy == EVG_POLICY_CYCLE_TARGET_NODE11P2 && agent2) ? ctl <= -level : ctl >= level;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                if (controlled) {
                    rows[i] = make_int2(group_num, node_num);
                    cycle_advance(group_num, node_num);
                } else {
                    const int cur = v.loc(group_num);
                    const int nx = (int)(((tar == 1 ? tabs.tar1 : tabs.tar11) >> (4 * cur)) & 15ull);   // 15 encodes the bots' -1
                    rows[i] = make_int2(group_num, nx == 15 ? -1 : nx);
                    group_num = (group_num + 1) % NG;
                }
            }
        }
        first = 0; cyc_dirty = true;
    } else if (policy == EVG_POLICY_DFS_ATTACK) {
        // dfs_attack.py ignores the observation: its orders are an eventually periodic sequence of the call count,
        // tabulated on the host at evg_create (including the rows that persist in its mutable default argument)
        const uint32_t c = *p_dfs;
        const uint32_t idx = c < (uint32_t)tabs.T->dfs_mu ? c : (uint32_t)tabs.T->dfs_mu + (c - (uint32_t)tabs.T->dfs_mu) % (uint32_t)tabs.T->dfs_lambda;
        const uint64_t r = tabs.T->dfs_rows[idx];
#pragma unroll
        for (int i = 0; i < NA; ++i) rows[i] = make_int2((int)((r >> (8 * i)) & 15ull), (int)((r >> (8 * i + 4)) & 15ull));
        if (commit) *p_dfs = c + 1u;
    } else if (policy == EVG_POLICY_SAME_COMMANDS) {                        // same_commands.py / same_commands_2.py
#pragma unroll
        for (int i = 0; i < NA; ++i) rows[i] = make_int2(i + 1, i + 1);
    } else if (policy == EVG_POLICY_SWARM) {
        uint32_t lst = *p_swarm;                                           // attack list, 8 nibbles
        const uint4 x0 = rng_block(seed_lo, seed_hi, env_id, episode, RNG_SWARM, 0u, turn, 0, player, 0);
        const uint4 x1 = rng_block(seed_lo, seed_hi, env_id, episode, RNG_SWARM, 1u, turn, 0, player, 0);
        const uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int k = 0; k < 7; ++k) {                                      // i = 7 .. 1
            const int i = 7 - k;
            const int j = (int)__umulhi(w[k], (uint32_t)(i + 1));
            const uint32_t x = ((lst >> (4 * i)) ^ (lst >> (4 * j))) & 15u;
            lst ^= (x << (4 * i)) ^ (x << (4 * j));
        }
        if (commit) *p_swarm = lst;
#pragma unroll
        for (int i = 0; i < NA; ++i) rows[i] = make_int2(0, 1);            // np.tile([0, 1], (7, 1))
        const uint64_t mx = tabs.maxnbr;
        int n = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int g = (int)((lst >> (4 * k)) & 15u);
            const bool idle = v.moving(g) == 0;
            const int pos = v.loc(g);
            const int2 r = make_int2(g, (int)((mx >> (4 * pos)) & 15u));   // max(NODE_CONNECTIONS[pos]), :97
#pragma unroll
            for (int i = 0; i < NA; ++i) rows[i] = (idle && n == i) ? r : rows[i];
            n += (idle && n < NA) ? 1 : 0;
        }
    }                                                                      // EVG_POLICY_NO_ACTION: zeros
    if (cyc_dirty && commit)
        *p_cycle = (uint32_t)node_num | ((uint32_t)group_num << 4) | ((uint32_t)first << 8) | ((uint32_t)strat << 9) | ((uint32_t)agent2 << 13);
}

// what a bot reads from its observation row (everglades_env.py:158-171 layout)
template <typename OT>
struct ObsView {
    const OT* o;
    __device__ int turn() const { return (int)o[0]; }
    __device__ int loc(int k) const { return (int)o[45 + 5 * k]; }
    __device__ int moving(int k) const { return (int)o[48 + 5 * k]; }
    __device__ int ctrl_slot(int slot) const { return (int)o[4 * slot - 1]; }
    __device__ int opp_units_slot(int slot) const { return (int)o[4 * slot]; }
};

// the same quantities taken from the on-chip state at the start of a turn (fused rollout), over either lane mapping's LDS (StepLds<LPW> / Step4Lds:
// G = group words [gid][side column], NW = node words [node][env column])
template <typename Lds>
struct ChipView {
    const Lds* L;
    int col, E, P, turn_;
    uint64_t p1nib;
    __device__ int node_of_slot(int slot) const { return P ? (int)((p1nib >> (4 * slot)) & 15u) : slot; }
    __device__ int turn() const { return turn_; }
    __device__ int loc(int k) const { const uint32_t l = L->G[k][col] & G_LOC_M; return P ? (int)((p1nib >> (4 * l)) & 15u) : (int)l; }
    __device__ int moving(int k) const { return ((L->G[k][col] & G_MODE_M) >> G_MODE_S) == MODE_MOVING ? 1 : 0; }
    __device__ int ctrl_slot(int slot) const { return node_cs(L->NW[node_of_slot(slot)][E]); }
    __device__ int opp_units_slot(int slot) const {                        // units of every non-destroyed opposing group listed at the node
        const uint32_t n = (uint32_t)node_of_slot(slot);
        int u = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) { const uint32_t w = L->G[k][col ^ 1]; u += (w & G_LOC_M) == n ? __popc(w & G_MASK_M) : 0; }
        return u;
    }
};
