/*
 * evg.h -- C-ABI of the MI355X-native batched Everglades environment (libevg.so).
 *
 * This is the drop-in boundary for ONE hot path of jlehett/everglades-ai-wargame: the
 * everglades-server turn loop plus gym_everglades step()/reset(), vectorised over N
 * independent two-player DemoMap games whose state lives struct-of-arrays in HBM.
 * The reference has no FFI of its own -- its Gym class *is* the boundary
 * (gym-everglades/gym_everglades/envs/everglades_env.py:13-173).  Each entry point below
 * cites the reference code it replaces; the Python binding a maintainer would add is in
 * INTEGRATION.md and shipped as everglades-ai-wargame_amd/_lib.py.
 *
 * Conventions
 *   - plain C, no torch types; every pointer marked "device" is a HIP device pointer owned by the
 *     caller (e.g. torch.Tensor.data_ptr()); the handle owns only the persistent game state.
 *   - ALIGNMENT: every device buffer of observations, orders, features or packed results handed to the library must be 16-byte aligned
 *     (observation rows move 16 bytes per lane, order rows as int2 / uint4); reward and score buffers 8-byte aligned (one float2 / int2 per
 *     env, so any env offset into an [N][2] tensor is fine).  Any hipMalloc / torch allocation is 16-byte aligned; a slice of one need not be.
 *     Checked by every entry point: EVG_ERR_INVALID names the pointer.  Byte arrays (done, winner, status, mask, fog planes) have no
 *     requirement.
 *   - all calls return 0 on success or a negative evg_status; evg_last_error() gives the text
 *     (thread-local).  No C++ exception crosses the ABI.
 *   - step/reset/random_actions ENQUEUE on the caller's hipStream_t (`stream`, may be NULL for the
 *     default stream) and return without synchronising.  A handle belongs to ONE device and is not thread-safe; any
 *     number of handles may live on a device and run concurrently on different streams (they share nothing).
 *   - there is NO CPU fallback: evg_create fails with EVG_ERR_NO_DEVICE when no gfx950 device
 *     is usable.
 *   - env e of this handle has the global id env_id_base + e; random streams are keyed by the
 *     global id, so results do not depend on how envs are sharded over GPUs.
 */
#ifndef EVG_H
#define EVG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVG_ABI_VERSION 7
/* 7: evg_step_vs_policy_smart_q (the Smart_State learner's turn from its Q values: DQNAgent.get_action decoded inside the learner-seat step launch);
 *    evg_step_smart_q (the self-play turn: both seats' Q values decoded inside one step launch; an added function, no layout changed);
 *    evg_smart_qnet with its descriptor evg_qnet: the Smart_State Q network's forward pass in one launch (added, no layout changed);
 *    the opponent league: evg_league_clear / evg_league_assign / evg_league_importance / evg_step_vs_league / evg_step_vs_league_q with their descriptor
 *    evg_league -- added, no layout changed;
 *    the Minimized agents (agents/Minimized: a 59-h1-11 network, one Q per node): evg_minimized_get_action, evg_step_vs_policy_minimized_q,
 *    evg_step_vs_league_minimized_q, evg_minimized_qnet with its descriptor evg_mini_qnet -- added, no layout changed;
 *    Minimized self-play (a network on each seat): evg_step_minimized_q, evg_step_league_minimized_q (a league whose member q_member is the caller's
 *    second network) -- added, no layout changed;
 *    self-royale (a per-env Minimized network drawn from a population each episode): evg_population_clear / evg_population_assign /
 *    evg_population_qnet with their descriptor evg_population -- added, no layout changed;
 *    Smart_State self-royale (the same with the 59-h1-h2-5 network): evg_smart_population_clear / evg_smart_population_assign /
 *    evg_smart_population_qnet with their descriptor evg_smart_population -- added, no layout changed */
/* 6: evg_smart_get_action (DQNAgent.get_action with epsilon > 0), evg_step_vs_policy_smart (the learner-seat turn that also writes the Smart_State
 *    features), evg_get_run_state / evg_set_run_state (agent objects, returns, win counters: checkpoint / resume); reward / score buffers need 8-byte
 *    alignment only (5 asked 16 of every buffer)
 * 5: evg_smart_actions; evg_comm_unique_id / evg_comm_init / evg_gather_returns / evg_comm_destroy + EVG_ERR_COMM; every device buffer must be
 *    16-byte aligned (checked)
 * 4: evg_step_vs_policy / evg_observe_seat / evg_rollout_vs_policy / evg_random_actions_seat / evg_smart_state_seat, evg_smart_state_compact,
 *    evg_check_fault + EVG_ERR_FAULT, evg_pack_episode_results_counted, evg_config.cache_mib
 * 3: evg_launch_plan
 * 2: evg_pack_episode_results, node words as u32 */

/* The ABI is exactly the functions declared in this header: the library is built with -fvisibility=hidden and only they are exported. */
#define EVG_API __attribute__((visibility("default")))

/* Fixed dimensions of the reference environment (everglades_env.py:17-22). */
#define EVG_NUM_PLAYERS 2
#define EVG_NUM_GROUPS 12      /* num_groups            */
#define EVG_NUM_NODES 11       /* num_nodes (IDs 1..11) */
#define EVG_NUM_UNITS 100      /* num_units per player  */
#define EVG_NUM_ACTIONS 7      /* num_actions_per_turn  */
#define EVG_OBS_LEN 105        /* 1 + 4*11 + 5*12 (everglades_env.py:158-171) */
#define EVG_MAX_UNIT_TYPES 4
#define EVG_MAX_GROUP_SIZE 12
#define EVG_MAX_SCORE 3700     /* everglades_env.py:11 */

typedef enum evg_status {
    EVG_OK = 0,
    EVG_ERR_INVALID = -1,      /* bad argument / table out of the supported domain */
    EVG_ERR_ARG = EVG_ERR_INVALID,   /* the same status under the name the league entry points' contract uses */
    EVG_ERR_NO_DEVICE = -2,    /* no usable HIP device (there is no CPU path)        */
    EVG_ERR_HIP = -3,          /* a HIP runtime call failed                         */
    EVG_ERR_ALLOC = -4,
    EVG_ERR_FAULT = -5,        /* the handle's fault word is set (evg_check_fault): its results are not valid, destroy it */
    EVG_ERR_COMM = -6          /* RCCL is not available or one of its calls failed (evg_comm_*, evg_gather_returns)          */
} evg_status;

typedef enum evg_obs_dtype { EVG_OBS_F32 = 0, EVG_OBS_F64 = 1, EVG_OBS_I16 = 2 } evg_obs_dtype;

/* Source of the combat target draws (server.py:562).
 *   EVG_RNG_KEYED_PHILOX   the fast path: counter-based draws keyed by (seed, env id, episode, turn, node, player,
 *                          group, unit) -- DESIGN.md section 4; what every throughput figure is measured with.
 *   EVG_RNG_STOCK_MT19937  compatibility mode: every env owns the generator the unmodified reference
 *                          uses -- numpy's legacy MT19937 after np.random.seed(s), randint by masked rejection, consumed
 *                          in the reference's loop order including its two unobservable focus draws (server.py:205,
 *                          :338) -- so a game replays the reference process bit for bit.  2.5 KB of extra state per
 *                          env and sequential draws: for validation, not speed.  Single-turn launches only.        */
typedef enum evg_rng_mode { EVG_RNG_KEYED_PHILOX = 0, EVG_RNG_STOCK_MT19937 = 1 } evg_rng_mode;

/* game status (server.py:284-288) */
enum { EVG_IN_PROGRESS = 0, EVG_TIME_EXPIRED = 1, EVG_BASE_CAPTURE = 2, EVG_ANNIHILATION = 3 };
/* winner_out values; the harness rule evaluate.py:155-160 applied to the terminal rewards */
enum { EVG_WINNER_NONE = -1, EVG_WINNER_P0 = 0, EVG_WINNER_P1 = 1, EVG_WINNER_TIE = 2 };
/* node_resource bits (DemoMap.json "Resource") */
enum { EVG_RES_DEFENSE = 1, EVG_RES_OBSERVE = 2 };

/*
 * Flattened constant tables: what server.py:40-131 parses out of config/DemoMap.json and
 * config/UnitDefinitions.json plus the army of everglades_env.py:145-156.  Node arrays are
 * indexed by node ID (1..11; entry 0 unused).  Domain checked by evg_create:
 *   distances 0 (not connected) or 1..7; control_points 1..511; defense >= 0;
 *   unit damage/speed/control/cost 1..15, unit health 1..255, at most 4 unit types;
 *   the army SHAPE is the reference's hard-coded one (everglades_env.py:145-156): group_size must be 8 for groups 0..10 and
 *   12 for group 11 of both players -- anything else is refused with EVG_ERR_INVALID (the unit TYPE of every group is free);
 *   total damage of an army (sum of size x unit damage) <= 255; max_turns 1..255;
 *   global env ids are 32-bit keys of the random streams: env_id_base + num_envs <= 2^32.
 * PINNED AGAINST THE REFERENCE inside this domain (tests/golden/custom_*.npz: the imported reference playing on non-default map / unit files): directed
 * distances incl. one-way edges and edges with different lengths per direction, control points up to 511, non-dyadic defenses, DEFENSE / OBSERVE on any
 * node, bases on any two nodes, unit types in any order, a p1_node_map that is not its own inverse.  What this struct cannot express and a host parser must
 * therefore refuse (everglades_amd.tables_from_json does): a node list that is not in ascending ID order (the reference's own fog mask then mixes list
 * positions with IDs, server.py:409-418), a resource named 'DEFEND' (it would switch the reference's otherwise dead fortress bonus on, server.py:595 -- not
 * modelled), fractional values where the tables hold integers (the reference would compute with the float).  max_turns other than 150 and p1_node_map
 * other than DemoMap's have no file in the reference (hard-coded at server.py:321 and :89).
 */
typedef struct evg_tables {
    int32_t node_dist[EVG_NUM_NODES + 1][EVG_NUM_NODES + 1];
    int32_t node_control_points[EVG_NUM_NODES + 1];
    double  node_defense[EVG_NUM_NODES + 1];
    int32_t node_resource[EVG_NUM_NODES + 1];
    int32_t node_team_start[EVG_NUM_NODES + 1];        /* -1, 0 or 1                         */
    int32_t p1_node_map[EVG_NUM_NODES + 1];            /* server.py:89                       */
    int32_t num_unit_types;
    int32_t unit_health[EVG_MAX_UNIT_TYPES];           /* "armor" in the damage equation      */
    int32_t unit_damage[EVG_MAX_UNIT_TYPES];
    int32_t unit_speed[EVG_MAX_UNIT_TYPES];
    int32_t unit_control[EVG_MAX_UNIT_TYPES];
    int32_t unit_cost[EVG_MAX_UNIT_TYPES];
    int32_t group_type[EVG_NUM_PLAYERS][EVG_NUM_GROUPS];  /* unit type id of each group        */
    int32_t group_size[EVG_NUM_PLAYERS][EVG_NUM_GROUPS];  /* units per group at reset          */
    int32_t max_turns;                                    /* 150 (server.py:321)               */
} evg_tables;

typedef struct evg_config {
    uint32_t struct_size;      /* = sizeof(evg_config); ABI guard            */
    uint32_t abi_version;      /* = EVG_ABI_VERSION                          */
    int32_t  num_envs;         /* N >= 1                                     */
    int32_t  device_id;        /* HIP device ordinal                         */
    uint64_t seed;             /* Philox key                                 */
    uint64_t env_id_base;      /* global id of env 0 of this handle          */
    int32_t  obs_dtype;        /* evg_obs_dtype of obs_out buffers           */
    int32_t  auto_reset;       /* 1: an env that finishes in step() is reset in the same launch and
                                  obs_out holds the first observation of its next episode           */
    int32_t  rng_mode;         /* evg_rng_mode; in the stock mode env e starts as np.random.seed((uint32)(seed + env_id_base + e)) */
    int32_t  cache_mib;        /* 0 = derive: what a chunked rollout launch may cycle through, in MiB -- the memory-side (Infinity) cache share of this
                                  device, 256 MiB x compute units / 256 on MI355X (HIP has no query for it); > 0 overrides.  evg_launch_plan reports it */
    evg_tables tables;
} evg_config;

typedef struct evg_handle evg_handle;

/* Fills `t` with the DemoMap / UnitDefinitions / default-army tables. */
EVG_API void evg_default_tables(evg_tables* t);

/* Replaces EvergladesGame.__init__/board_init/unitTypes_init (server.py:14-131): tables are parsed
 * once by the host and copied to the device; state for N envs is allocated and every env is put in
 * the game_init position (episode counter -1, so the first evg_reset starts episode 0). */
EVG_API int evg_create(const evg_config* cfg, evg_handle** out);
EVG_API void evg_destroy(evg_handle* h);

/* Replaces EvergladesEnv.reset (everglades_env.py:75-116) -> game_init (server.py:133-209) ->
 * _build_observations (everglades_env.py:158-171).
 *   mask    device uint8[N] or NULL (= all): envs with mask != 0 start a new episode
 *   obs_out device [N][2][105] of cfg.obs_dtype or NULL; written for the envs that were reset */
EVG_API int evg_reset(evg_handle* h, const uint8_t* mask, void* obs_out, void* stream);

/* Replaces EvergladesEnv.step (everglades_env.py:32-73) -> EvergladesGame.game_turn
 * (server.py:211-279: orders, combat :503, movement :656, capture :708, game_end :281) ->
 * board_state/player_state (:382-501).  build_knowledge_output (:769-907) mutates nothing and is
 * not reproduced.
 *   actions    device int32 [N][2][7][2]  (group id, node id in the player's own numbering); ids in [-12, -1]
 *              index from the end like the reference's Python lists (group -1 is group 11; for player 1 node -1
 *              is p1_node_map[-1]; `used_swarms` dedupes on the id as given); any other out-of-range id is an
 *              invalid order, never undefined behaviour
 *   obs_out    device [N][2][105] of cfg.obs_dtype
 *   reward_out device float [N][2]   (everglades_env.py:37-61)
 *   done_out   device uint8 [N]
 *   winner_out device int8  [N]  or NULL
 *   scores_out device int32 [N][2] or NULL  (server.py:291-317)
 *   status_out device uint8 [N]  or NULL  (server.py:284-288)
 * Without auto_reset a finished env is frozen: further steps leave it unchanged and repeat its
 * terminal outputs. */
EVG_API int evg_step(evg_handle* h, const int32_t* actions, void* obs_out, float* reward_out, uint8_t* done_out,
             int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);

/* Observations of the current state without stepping (after evg_set_state, or to re-read them):
 * the board_state/player_state half of step (server.py:382-501). obs_out as in evg_step. */
EVG_API int evg_observe(evg_handle* h, void* obs_out, void* stream);

/* The turn of the loop every training and evaluation script of the reference runs: a caller (the learner) on ONE seat, a scripted
 * bot on the other (evaluate.py:85-93,143-152: `actions[p] = players[p].get_action(obs[p])` with one learned and one scripted player;
 * agents/Smart_State/training_scripts/dqn_smart_state_training.py:114-122) -- in ONE launch: the opponent's bot is evaluated inside the
 * step kernel from the on-chip state (exactly what its observation would hold; same agent objects as evg_scripted_actions, alive across
 * episodes), the caller's orders are read for the other seat, and only the caller's seat's observation is written (420 B per env less
 * than evg_step, half of the observation build, no second launch and no round trip of the opponent's observations and orders).
 *   seat             0 or 1: the caller's seat
 *   actions          device int32, the caller's 7 order rows per env: [N][7][2] (actions_both_seats == 0) or the rows [:, seat] of
 *                    a [N][2][7][2] tensor (actions_both_seats != 0; the other seat's rows are ignored).  Domain as in evg_step
 *   opponent_policy  EVG_POLICY_* played by seat 1 - seat
 *   obs_seat_out     device [N][105] of cfg.obs_dtype: the caller's seat's observation (everglades_env.py:158-171); 16-byte aligned
 *   reward_out, done_out, winner_out, scores_out, status_out: as in evg_step (both seats' rewards and scores: the harness compares
 *                    reward[0] with reward[1], evaluate.py:155-160)
 * Results are those of evg_scripted_actions(opponent) + evg_step on the same orders, bit for bit.  Keyed-Philox handles only.  The launch itself
 * lasts as long as evg_step's (26.7 us at 65 536 envs on an MI355X; a single-turn launch is bound by its latency chain, not by its bytes: DESIGN.md
 * section 6); what is saved is the bot's own kernel (7-9 us and 55 MB of observations read back) and the traffic listed above. */
EVG_API int evg_step_vs_policy(evg_handle* h, int seat, const int32_t* actions, int actions_both_seats, int opponent_policy, void* obs_seat_out,
                               float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);
/* The same turn for a Smart_State learner (agents/Smart_State/DQNAgent.py): besides the seat's observation the launch also writes the agent's network INPUT
 * of the next turn -- the features of DQNAgent.create_swarm_obs (:268-300) in the compact form of evg_smart_state_compact: shared_out device float [N][34]
 * (8-byte aligned), swarm_out device float [N][12][13] (16-byte aligned) -- computed from the observation image while it is still on chip.  Value for value
 * what evg_smart_state_compact(h, -1, obs_seat_out, shared_out, swarm_out) would write after this call, without that kernel (23 us at 65 536 envs) and
 * without reading the row back.  The first features of a loop (after evg_reset) come from evg_observe_seat + evg_smart_state_compact. */
EVG_API int evg_step_vs_policy_smart(evg_handle* h, int seat, const int32_t* actions, int actions_both_seats, int opponent_policy, void* obs_seat_out,
                                     float* shared_out, float* swarm_out, float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out,
                                     uint8_t* status_out, void* stream);
/* The Smart_State learner's whole turn in ONE launch, from its network's output to its network's next input
 * (agents/Smart_State/training_scripts/dqn_smart_state_training.py:114-122): the caller hands its Q values, not its orders.  The launch does
 * DQNAgent.get_action for the caller's seat -- the epsilon coin, then get_random_actions or get_best_actions, exactly as evg_smart_get_action -- plays the
 * scripted opponent, steps the game and writes the next observation and (optionally) the compact features, as evg_step_vs_policy_smart.  The order rows
 * never go through HBM unless asked for.
 *   seat             0 or 1: the caller's seat (also the agent's player number that keys its draws)
 *   q                device float [N][12][5] (16-byte aligned): the network's Q values of every swarm; domain as in evg_smart_actions (first maximum,
 *                    a NaN is the maximum and sorts like +inf, stable ascending sort, first seven)
 *   epsilon, epsilon_env  as in evg_smart_get_action (epsilon must lie in [0, 1] when epsilon_env is NULL)
 *   opponent_policy, obs_seat_out, reward_out, done_out, winner_out, scores_out, status_out: as in evg_step_vs_policy
 *   shared_out, swarm_out  both NULL or both set: the features of evg_step_vs_policy_smart; here shared_out must be 16-byte aligned
 *   actions_out      device int32 [N][7][2] or NULL: the rows the caller's seat played ({swarm, node})
 *   directions_out   device int32 [N][7][2] or NULL: {swarm, direction} (what the reference's replay memory stores)
 *   explored_out     device uint8 [N] or NULL: 1 where the random branch ran
 * The decode reads each swarm's location, the turn and the episode from the state the launch starts from: what the seat observation of the previous
 * launch (or evg_observe_seat) shows, also across auto-resets.  Results -- every output above, and the handle's state afterwards -- are bit for bit those
 * of evg_smart_get_action(h, seat, 1, obs_prev, q, epsilon, epsilon_env, a, d, x) followed by evg_step_vs_policy_smart(h, seat, a, 0, ...) (or
 * evg_step_vs_policy), with obs_prev the seat observation of the previous launch.  Every env's rows, directions and explored flag are written, finished
 * ones included (as evg_smart_get_action does).  Keyed-Philox handles only. */
EVG_API int evg_step_vs_policy_smart_q(evg_handle* h, int seat, const float* q, float epsilon, const float* epsilon_env, int opponent_policy,
                                       void* obs_seat_out, float* shared_out, float* swarm_out,
                                       int32_t* actions_out, int32_t* directions_out, uint8_t* explored_out,
                                       float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);
/* The self-play turn in ONE launch, a Smart_State DQNAgent on each seat (agents/Smart_State/training_scripts/dqn_smart_state_self_play.py:120-128,
 * dqn_smart_state_self_royale.py:135-143): both seats hand their Q values, not their orders.  The launch does DQNAgent.get_action for seat 0 and for seat 1
 * -- each its own epsilon coin, then get_random_actions or get_best_actions, exactly as evg_smart_get_action -- steps the game with both seats' rows and
 * writes the next observation and (optionally) the compact features of both players.  The order rows never go through HBM unless asked for.
 *   q                device float [N][2][12][5] (16-byte aligned): row [e][p] is seat p's network output; domain as in evg_smart_actions (first maximum,
 *                    a NaN is the maximum and sorts like +inf, stable ascending sort, first seven)
 *   epsilon0, epsilon1  each seat's epsilon, in [0, 1] (a training seat decays its own, a frozen one plays 0.0)
 *   epsilon_env      device float [N][2] or NULL: when set, it replaces both scalars
 *   obs_out, reward_out, done_out, winner_out, scores_out, status_out: as in evg_step (obs_out [N][2][105] in the handle's dtype)
 *   shared_out, swarm_out  both NULL or both set, both 16-byte aligned: shared [N][2][34], swarm [N][2][12][13], the features of evg_smart_state_compact for
 *                    player 0 and player 1
 *   actions_out      device int32 [N][2][7][2] or NULL: the rows both seats played ({swarm, node}: exactly the tensor evg_step takes)
 *   directions_out   device int32 [N][2][7][2] or NULL: {swarm, direction}
 *   explored_out     device uint8 [N][2] or NULL: 1 where the seat's random branch ran
 * Each seat's explore draws keep the key of evg_smart_get_action (env id, episode, turn, seat).  The decode reads each swarm's location (in the seat's own
 * numbering), the turn and the episode from the state the launch starts from: what the observation of the previous launch shows, also across auto-resets.
 * Results -- every output above, and the handle's state and run state afterwards -- are bit for bit those of evg_smart_get_action(h, 0, 1, obs_prev[:, 0],
 * q[:, 0], epsilon0, ...) and evg_smart_get_action(h, 1, 1, obs_prev[:, 1], q[:, 1], epsilon1, ...), then evg_step with both seats' rows, then
 * evg_smart_state_compact for player 0 and player 1, with obs_prev the observation of the previous launch.  Every env's rows, directions and explored flags are
 * written, finished ones included.  Keyed-Philox handles only. */
EVG_API int evg_step_smart_q(evg_handle* h, const float* q, float epsilon0, float epsilon1, const float* epsilon_env,
                             void* obs_out, float* shared_out, float* swarm_out,
                             int32_t* actions_out, int32_t* directions_out, uint8_t* explored_out,
                             float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);
/* evg_observe for one seat: obs_seat_out device [N][105] (after evg_reset / evg_set_state, to start a evg_step_vs_policy loop). */
EVG_API int evg_observe_seat(evg_handle* h, int seat, void* obs_seat_out, void* stream);

/* Fog-of-war planes of the current state, both computed by the reference and never applied to its observations:
 *   fog_out        device uint8 [N][2][11] or NULL: the `valid_nodes` mask of board_state (server.py:402-425);
 *                  [e][p][i] = 1 iff player p sees node ID i+1 (a node it controls, a neighbour of a controlled OBSERVE
 *                  node, or a node where it has a non-moving group)
 *   knowledge_out  device uint8 [N][2][11] or NULL: the knowledge level of build_knowledge_output (server.py:779-832):
 *                  2 full (controlled, or a non-moving group there), 1 partial (next to a fully controlled OBSERVE node
 *                  of the player, or one of its groups is moving there), 0 none
 * Real node order, not mirrored for player 1, exactly as the reference computes them. */
EVG_API int evg_fog_of_war(evg_handle* h, uint8_t* fog_out, uint8_t* knowledge_out, void* stream);

/* The opposing-group sightings `opp_k` of build_knowledge_output (server.py:845-907), also computed and dropped by the
 * reference.  sight_out: device int8 [N][2][12][4]; [e][p][g] = what player p knows of opposing group g:
 *   {seen, node ID, destination key, units alive}.  seen = 1 iff the group is listed at a node whose knowledge level is 1 or 2
 *   and it is either not moving (key -1) or moving to a node of knowledge > 0 (key = that node's index in the node list,
 *   i.e. ID - 1 -- the reference keys stationary groups by -1 and moving ones by the list index, :866-881); else 0,0,0,0. */
EVG_API int evg_sightings(evg_handle* h, int8_t* sight_out, void* stream);

/* Consumer-side preprocessing of the reference's strongest agent family (agents/Smart_State/DQNAgent.py:200-300,
 * create_swarm_obs): from `player`'s rows of obs (device [N][2][105] of cfg.obs_dtype) to features_out, device float
 * [N][12][59] (16-byte aligned): per swarm {turn/150, 11 x control/100, 11 x enemy units/100, 11 x idle allied groups/12, one-hot node,
 * avg health x alive / 1000, in transit, one-hot swarm id}; each value is the reference's float64 expression rounded to
 * float32.  evg_move_table fills table[11][5] with Move_Translation.get_move(node0, direction) (host memory). */
EVG_API int evg_smart_state(evg_handle* h, int player, const void* obs, float* features_out, void* stream);
/* The same features from a one-seat observation tensor (device [N][105], as evg_step_vs_policy / evg_observe_seat write it). */
EVG_API int evg_smart_state_seat(evg_handle* h, const void* obs_seat, float* features_out, void* stream);
/* The same features without their redundancy (what a bandwidth-bound consumer wants: the full matrix is 2 832 B per env, 185 MB per call at 65 536 envs).
 * Of the 59 features of a swarm, 34 are the same for all 12 swarms of an env ({turn/150, 11 x control/100, 11 x enemy units/100, 11 x idle allied groups/12})
 * and 12 are the constant one-hot swarm id; the matrix is therefore determined by
 *   shared_out  device float [N][34]       (8-byte aligned)   = features[e][s][0:34] for any s
 *   swarm_out   device float [N][12][13]   (16-byte aligned)  = features[e][s][34:47] = {one-hot node (11), avg health x alive / 1000, in transit}
 * (760 B per env); features[e][s] = shared[e] ++ swarm[e][s] ++ onehot(s), value for value what evg_smart_state writes.  player 0 / 1: obs is
 * [N][2][105]; player -1: obs is a one-seat tensor [N][105]. */
EVG_API int evg_smart_state_compact(evg_handle* h, int player, const void* obs, float* shared_out, float* swarm_out, void* stream);
EVG_API void evg_move_table(int32_t* table);
/* ... and the way back, network output -> orders: DQNAgent.get_best_actions (agents/Smart_State/DQNAgent.py:176-198) over swarm_think (:233-266),
 * get_swarm_node_number (:302-310) and Move_Translation.get_move (Move_Translation.py:85-97).
 *   q               device float [N][12][5]: the policy network's Q values of every swarm for the five directions left, right, up, down, stay (the network
 *                   itself -- QNetwork 59-60-60-5 in the reference -- is the consumer's); 16-byte aligned
 *   obs / player    as in evg_smart_state_compact: player 0 / 1 reads that seat's rows of [N][2][105], player -1 a one-seat tensor [N][105] (only the
 *                   swarm locations obs[45 + 5 s] are read)
 *   actions_out     device int32 [N][7][2]: {swarm, node} -- exactly the `actions` of evg_step_vs_policy (actions_both_seats == 0)
 *   directions_out  device int32 [N][7][2] or NULL: {swarm, direction} (what the reference's replay memory stores)
 * Every swarm's best direction is the FIRST maximum of its five Q values (torch.argmax), its order the node get_move gives for that direction from the
 * swarm's location, and the seven rows are the first seven decisions of a STABLE ASCENDING sort by best Q: the reference acts with the seven swarms whose
 * best Q is LOWEST (sorted(...)[:7], :189-197) -- reproduced as it is.  Q values must not be NaN (the reference's sort is undefined for them; here a NaN
 * is a swarm's maximum, as in torch, and sorts like +inf).  With evg_smart_state(_seat / _compact) this closes the learner's turn on the device:
 * observation -> features -> (consumer's network) -> orders -> evg_step_vs_policy, no host or framework glue between the kernels. */
EVG_API int evg_smart_actions(evg_handle* h, int player, const void* obs, const float* q, int32_t* actions_out, int32_t* directions_out, void* stream);
/* The whole of DQNAgent.get_action (agents/Smart_State/DQNAgent.py:130-146): `sample = random.random(); if sample < self.epsilon:
 * get_random_actions(obs) else get_best_actions(obs)`, i.e. evg_smart_actions plus the exploring branch (:148-173): swarms = np.random.choice(12, 7,
 * replace=False), directions = np.random.choice(5, 7, replace=True), row i = {swarms[i], get_move(location of swarms[i] - 1, directions[i])}.  With it the
 * learner's turn stays on the device during TRAINING (epsilon > 0) too.
 *   seat            0 / 1: the agent's player number; with obs_one_seat == 0 its rows of obs [N][2][105] are read, with obs_one_seat != 0 obs is a
 *                   one-seat tensor [N][105].  Only obs[0] (the turn, part of the key of the draws) and the swarm locations obs[45 + 5 s] are read.
 *   epsilon         the exploring probability of every env, in [0, 1]; epsilon_env (device float [N], may be NULL) gives one per env instead.
 *   actions_out / directions_out   as in evg_smart_actions;  explored_out  device uint8 [N] or NULL: 1 where the random branch was taken.
 * The coin and the two choices are keyed draws like every other (oracle/rng_spec.py `explore_draws`, domain 4): one agent call =
 * (seed, global env id, episode, turn = obs[0], seat) -- pinned against the reference's own get_action by tests/golden/smart_explore.npz.  The coin is a 32-bit
 * fraction compared with epsilon in float64 (epsilon 0 never explores, epsilon 1 always). */
EVG_API int evg_smart_get_action(evg_handle* h, int seat, int obs_one_seat, const void* obs, const float* q, float epsilon, const float* epsilon_env,
                                 int32_t* actions_out, int32_t* directions_out, uint8_t* explored_out, void* stream);

/* Input generator for the benchmark configs: the on-device equivalent of
 * agents/State_Machine/random_actions.py:38-46 for every env and both players, keyed by
 * (seed, env id, episode, turn, player).  actions_out: device int32 [N][2][7][2]. */
EVG_API int evg_random_actions(evg_handle* h, int32_t* actions_out, void* stream);

/* The same generator for ONE seat: actions_seat_out device int32 [N][7][2], identical to the rows [:, seat] of evg_random_actions
 * (a stand-in for a learner's policy output in benchmarks of evg_step_vs_policy). */
EVG_API int evg_random_actions_seat(evg_handle* h, int seat, int32_t* actions_seat_out, void* stream);

/* Scripted opponents on the device (agents/State_Machine/): one agent object per (env, player), kept in the handle
 * and alive across episodes like the reference's (evaluate.py:85-93).  Reads `player`'s rows of obs (device
 * [N][2][105] of cfg.obs_dtype, as written by evg_step/evg_reset) and writes that player's 7 order rows of
 * actions_out (device int32 [N][2][7][2]).
 * All 17 bots of agents/State_Machine/ are covered by the 15 ids below (two pairs of files are identical in
 * behaviour); their random draws (np.random.choice, np.random.shuffle, random.random) are keyed like every other
 * draw.  Order ids a bot emits outside [0, 11] (e.g. the -1 of cycle_target_node*.py) are passed
 * through; evg_step treats them like the reference's Python lists do.
 * The bots route by THEIR OWN constants on every map: each file of agents/State_Machine/ carries DemoMap's NODE_CONNECTIONS (and TAR_NODE) as a module
 * constant and never reads the map file, so on another map many of their orders are rejected by the server -- the reference's behaviour, reproduced
 * (tests/golden/custom_agents.npz).
 * An agent is not consulted for a game that is over and not yet reset (status != 0 without auto-reset): the harness has left
 * that game's loop (evaluate.py:147-152), so its rows are zero and its object does not advance.
 * evg_scripted_reset re-creates all agent objects (first_turn, cycling position, attack list). */
enum {
    EVG_POLICY_RANDOM = 0,                 /* random_actions.py, random_actions_2.py                         */
    EVG_POLICY_CYCLE_RUSH_25 = 1,          /* cycle_rush_turn25.py                                           */
    EVG_POLICY_CYCLE_RUSH_50 = 2,          /* cycle_rush_turn50.py                                           */
    EVG_POLICY_SWARM = 3,                  /* swarm_agent.py                                                 */
    EVG_POLICY_ALL_CYCLE = 4,              /* all_cycle.py                                                   */
    EVG_POLICY_BASE_RUSH_V1 = 5,           /* base_rush_v1.py                                                */
    EVG_POLICY_BULL_RUSH = 6,              /* bull_rush.py                                                   */
    EVG_POLICY_CYCLE_TARGET_NODE = 7,      /* cycle_target_node.py   (target 11, level 75)                   */
    EVG_POLICY_CYCLE_TARGET_NODE1 = 8,     /* cycle_target_node1.py  (target 1, level 75)                    */
    EVG_POLICY_CYCLE_TARGET_NODE11 = 9,    /* cycle_target_node11.py (target 11, level 500)                  */
    EVG_POLICY_CYCLE_TARGET_NODE11P2 = 10, /* cycle_target_node11P2.py                                       */
    EVG_POLICY_DFS_ATTACK = 11,            /* dfs_attack.py                                                  */
    EVG_POLICY_NO_ACTION = 12,             /* no_action.py                                                   */
    EVG_POLICY_RANDOM_DELAY = 13,          /* random_actions_delay.py                                        */
    EVG_POLICY_SAME_COMMANDS = 14,         /* same_commands.py, same_commands_2.py                           */
    EVG_POLICY_COUNT = 15
};
EVG_API int evg_scripted_actions(evg_handle* h, int policy, int player, const void* obs, int32_t* actions_out, void* stream);
EVG_API int evg_scripted_reset(evg_handle* h, void* stream);

/* Rollout driver for random-vs-random play (the reference's demo/random_demo.py:90-113 loop with both
 * agents = random_actions): enqueues `steps` x (evg_random_actions into actions_buf, then evg_step) on
 * `stream` from native code, so that launch cost, not the Python interpreter, bounds small batches.
 * fused == 1: the step kernel draws the orders itself (same generator, same values) and stores them in
 * actions_buf, which saves the second launch and the round trip of the action tensor through HBM.
 * fused >= 2: additionally each launch plays up to `fused` consecutive turns per wavefront (persistent form: the
 * state of a wavefront's envs stays in LDS/registers between turns; observations, rewards, actions ... are still
 * written every turn, so the buffers hold the last turn as before).  Results are identical in all three forms.
 * With fused >= 1 obs_out and actions_buf may be NULL: the rollout then writes no observations (the step kernel skips the
 * observation image and its write-out: a sixth of a turn's instructions and 55 % of its bytes) and / or does not record the orders --
 * what an evaluation loop needs, which reads only rewards, done flags and the episode results (evaluate.py:143-181).
 * A launch of the persistent form (fused >= 2) is a launch PLAN (evg_launch_plan: up to two step kernels, or memset + chunked kernel + queue check) that
 * keeps nothing on the host: when `stream` is being captured (e.g. torch.cuda.graph around this call) the plan becomes part of the caller's graph and
 * every replay plays the next turns.  (The library does not replay graphs of its own: measured slower than plain launches on ROCm 7.2, DESIGN.md
 * section 3.)  steps < 0 prepares a rollout of -steps turns with exactly these arguments -- whatever one-time work its launches need is done now, nothing
 * is enqueued and no state changes (a no-op in the product build; the graph-replay A/B build captures its graphs here).
 * Outputs as in evg_step (they hold the LAST step when the call returns).  If step_kernel_ms (host
 * pointer) is not NULL the work is bracketed by hipEvents on `stream`, the call synchronises the stream and stores the
 * stream time per turn in milliseconds: persistent form -- the duration of each launch (or launch plan, see
 * evg_launch_plan), summed, over the turns played; one launch per turn -- two events around the WHOLE loop over `steps`,
 * i.e. the step kernel plus the gap to the next launch plus, with fused == 0, the action kernel of the turn.  A timed call also returns
 * EVG_ERR_FAULT when the handle's fault word is set (evg_check_fault). */
EVG_API int evg_rollout_random(evg_handle* h, int steps, int fused, int32_t* actions_buf, void* obs_out, float* reward_out,
                       uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out,
                       float* step_kernel_ms, void* stream);

/* The same driver for any pair of on-device policies (EVG_POLICY_*; BASELINE config 5 is CYCLE_RUSH_25 vs SWARM).
 * fused == 0: per turn two agent launches read the previous observations in obs_out (which must hold the current
 * observations when the call starts, e.g. from evg_reset) and one step launch follows.  fused == 1: the step kernel
 * evaluates both agents itself from the on-chip state (the same quantities their observation holds) and stores the
 * orders in actions_buf; fused >= 2: persistent form as in evg_rollout_random.  Identical results in all forms. */
EVG_API int evg_rollout_policies(evg_handle* h, int steps, int fused, int policy0, int policy1, int32_t* actions_buf, void* obs_out,
                         float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out,
                         float* step_kernel_ms, void* stream);

/* Driver of the learner-seat loop for benchmarks: `steps` x (evg_random_actions_seat into actions_seat_buf [N][7][2] -- the stand-in for
 * the caller's policy output arriving in a tensor --, then evg_step_vs_policy(seat, actions_seat_buf, opponent_policy)), enqueued from
 * native code: two launches per turn.  Outputs and step_kernel_ms (stream time per turn between two events around the whole loop; the
 * call then synchronises) as in evg_rollout_random with fused == 0. */
EVG_API int evg_rollout_vs_policy(evg_handle* h, int steps, int seat, int opponent_policy, int32_t* actions_seat_buf, void* obs_seat_out, float* reward_out,
                                  uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, float* step_kernel_ms, void* stream);

/* Canonical state exchange (host order; used by parity tests and to load golden positions).
 * All pointers are HOST pointers; the call synchronises.  Any pointer may be NULL.
 *   groups int32 [N][2][12][8]: location, travel_destination (-1 none), distance_remaining, ready,
 *                               moving, destroyed, count, arrival stamp      (definitions.py:35-64)
 *   nodes  int32 [N][11][2]   : controlState, controlledBy                   (definitions.py:16-17)
 *   health double[N][2][100]  : unitHealth of the groups back to back         (definitions.py:62)
 *   env    int32 [N][4]       : current_turn, status, episode, reserved
 */
EVG_API int evg_get_state(evg_handle* h, int32_t* groups, int32_t* nodes, double* health, int32_t* env);
EVG_API int evg_set_state(evg_handle* h, const int32_t* groups, const int32_t* nodes, const double* health,
                  const int32_t* env);

/* Stock-entropy mode only (EVG_ERR_INVALID otherwise).
 * evg_seed_stock_entropy: np.random.seed(seeds[e]) for every env (HOST pointer, N entries; NULL = the create-time rule
 * (uint32)(seed + env_id_base + e)); enqueued on `stream` after a synchronous upload of the seeds.
 * evg_get/set_stock_entropy: the generators themselves, HOST uint32 [N][625] = 624 key words + position (the layout of
 * np.random.get_state()[1:3]); the calls synchronise.  Together with evg_get/set_state this checkpoints a game. */
EVG_API int evg_seed_stock_entropy(evg_handle* h, const uint32_t* seeds, void* stream);
EVG_API int evg_get_stock_entropy(evg_handle* h, uint32_t* out);
EVG_API int evg_set_stock_entropy(evg_handle* h, const uint32_t* in);

/* Checkpoint / resume of a RUNNING job: what evg_get_state / evg_set_state do not carry.  (the reference never serialises its env; its agents
 * pickle their own networks.  A handle restored with evg_set_state + evg_set_run_state -- + evg_set_stock_entropy in the stock mode -- on a handle created
 * with the same config continues bit for bit like the one that was saved: tests/test_gpu_parity.py::test_checkpoint_resume_continues_bit_for_bit.)
 * HOST pointers; the calls synchronise; any pointer may be NULL; evg_set_state zeroes the running returns, so restore the run state AFTER it.
 *   agents           uint32 [N][2][3]: the scripted agents' objects per (env, player) -- {first_turn / group_num / node_num word, SwarmAgent's attack list,
 *                    dfs_attack's call counter} (alive across episodes like the reference's agent objects, evaluate.py:85-93)
 *   running_returns  float [N][2]: the sum of rewards of the episode in progress
 *   returns, length, winner, totals: the arrays of evg_episode_stats (results of the last finished episode per env; episodes / wins since create)
 * evg_get_run_state fails with EVG_ERR_FAULT on a faulted handle, like evg_get_state. */
EVG_API int evg_get_run_state(evg_handle* h, uint32_t* agents, float* running_returns, float* returns, int32_t* length, int8_t* winner, int64_t* totals);
EVG_API int evg_set_run_state(evg_handle* h, const uint32_t* agents, const float* running_returns, const float* returns, const int32_t* length,
                              const int8_t* winner, const int64_t* totals);

/* Per-env results of the most recently finished episode, and running totals (device -> host copy,
 * synchronises).  Any pointer may be NULL.
 *   returns float [N][2]  sum of rewards over the episode
 *   length  int32 [N]     turns played
 *   winner  int8  [N]     EVG_WINNER_* (NONE if the env has not finished an episode yet)
 *   totals  int64 [4]     episodes finished, p0 wins, p1 wins, ties (this handle, since create)
 */
EVG_API int evg_episode_stats(evg_handle* h, float* returns, int32_t* length, int8_t* winner, int64_t* totals);
/* The handle's fault word (synchronises the device).  Chunked persistent rollout launches (batches beyond what the device holds at once,
 * evg_launch_plan) hand sets of envs from workgroup to workgroup; the word records: 1 = a workgroup gave up waiting for a predecessor
 * chunk (bounded wait, about 5 s), 2 = a workgroup ran on an XCD the create-time probe did not see, 4 = a queue of a chunked launch was
 * not drained (checked on the stream after every chunked launch), 8 = a hand-over delivered STALE state: every lane hands on a checksum over the chunk number
 * and every state word it stored, and the lane that takes the set's next chunk recomputes it over the words it loaded.  None is expected ever; all mean that state and results of the
 * handle are not valid.  The word is STICKY: evg_reset / evg_set_state do not clear it -- destroy the handle.  Returns EVG_OK or
 * EVG_ERR_FAULT (message in evg_last_error); *fault_out (may be NULL) receives the word.  Every path on which results leave the
 * handle checks it too: evg_episode_stats, evg_episode_stats_device and evg_get_state fail with EVG_ERR_FAULT, a timed rollout call
 * (step_kernel_ms != NULL, which synchronises anyway) fails with it, and evg_pack_episode_results writes POISONED rows
 * {NaN, NaN, -2, -1} for every env (winner -2 is no EVG_WINNER_* value), so a gather of packed rows cannot carry bad results unnoticed. */
EVG_API int evg_check_fault(evg_handle* h, uint32_t* fault_out);
/* Device pointers to the same per-env arrays (returns float[N][2], length int32[N], winner int8[N]),
 * for the multi-GPU gather of episode returns without a host round trip. */
EVG_API int evg_episode_stats_device(evg_handle* h, float** returns, int32_t** length, int8_t** winner);
/* The same per-env results packed for the path's ONE exchange between GPUs (the win bookkeeping of
 * evaluate.py:155-181 then runs on the gathered rows): out[e] = {return of player 0, return of player 1, winner, length} as
 * float32 (the small integers are exact), 16 bytes per env, written on `stream`.  out: device memory, [N][4], 16-byte aligned. */
EVG_API int evg_pack_episode_results(evg_handle* h, float* out, void* stream);
/* The same, and the win bookkeeping of the packed rows in the same kernel: counts_out device int64 [4] = rows with winner P0, P1, TIE and
 * rows without a finished episode (zeroed and filled on `stream`; all four are -1 when the rows are poisoned).  What a multi-GPU run
 * all-reduces next to the gather: the sum over ranks must equal what rank 0 counts in the gathered rows (bench.py). */
EVG_API int evg_pack_episode_results_counted(evg_handle* h, float* out, int64_t* counts_out, void* stream);

/* ---- Multi-GPU without torch.distributed: the path's ONE exchange over RCCL itself (SURVEY 8b `evg_gather_returns`, 8e) ----------------------------
 * Environments shard over GPUs by contiguous global id (env_id_base), one process and one handle per GPU, and nothing is exchanged but the per-env
 * results of finished episodes (win bookkeeping, evaluate.py:155-181).  A Python caller uses everglades_amd.ResultGather (torch.distributed, backend
 * "nccl" = RCCL); a caller without torch -- examples/c_client.c -- uses these four entry points.  librccl is opened at run time (dlopen("librccl.so.1"):
 * in a PyTorch process that is the instance torch already loaded); libevg.so itself does not depend on it, and the calls return EVG_ERR_COMM where RCCL is
 * missing.
 *   evg_comm_unique_id   ONE rank makes the communicator's id (ncclGetUniqueId); the caller hands the EVG_COMM_ID_BYTES bytes to every rank by its own means
 *                        (a file, a socket, MPI, an environment variable)
 *   evg_comm_init        every rank, collectively (it blocks until all `world` ranks have called): communicator of this handle's device.  counts: HOST
 *                        int32 [world], the num_envs of every rank's handle -- contiguous shards in rank order; counts[rank] must be this handle's
 *   evg_gather_returns   every rank, collectively, enqueued on `stream` (no synchronisation): evg_pack_episode_results of this handle + one grouped RCCL
 *                        send / receive.  recv_out: on rank `root` device float [sum(counts)][4], 16-byte aligned -- the rows {return p0, return p1,
 *                        winner, length} of ALL envs in global env order --, NULL on every other rank.  A rank whose handle is faulted sends poisoned rows
 *                        (winner -2), as evg_pack_episode_results does
 *   evg_comm_destroy     releases the communicator (evg_destroy does it as well)
 * ERRORS OF THESE CALLS ARE FATAL FOR THE WHOLE JOB.  evg_comm_init and evg_gather_returns validate their arguments (and RCCL's presence) BEFORE they enter
 * the collective: a rank that fails there returns its error at once while every other rank is already inside ncclCommInitRank / waiting for that rank's rows,
 * where RCCL has no timeout.  A caller must therefore treat any non-zero return of evg_comm_* / evg_gather_returns on ANY rank as the end of the job (tear the
 * process group down, e.g. let the launcher kill the ranks), never retry or continue on the ranks that succeeded; ranks agree on arguments that can differ
 * (counts, world, root) over their own channel before calling. */
#define EVG_COMM_ID_BYTES 128
EVG_API int evg_comm_unique_id(void* id_out);
EVG_API int evg_comm_init(evg_handle* h, const void* id, int world, int rank, const int32_t* counts);
EVG_API int evg_gather_returns(evg_handle* h, int root, float* recv_out, void* stream);
EVG_API int evg_comm_destroy(evg_handle* h);

/* Which step kernel(s) a rollout launch of `turns_per_launch` turns runs for this handle's batch on this device, as text in
 * buf (for benchmark records and logs): the kernel mapping (two / four lanes per env), the env range and wavefront count of
 * every launch of the plan, and the device capacity the plan was derived from (compute units from hipDeviceProp_t, resident
 * wavefronts from the kernels' own occupancy -- no 256-CU literal; the XCDs the create-time probe saw; the memory-side cache budget a chunked launch may
 * cycle through, evg_config.cache_mib, and the bytes per env it is compared with).  The plan described is the one of a rollout that writes observations and
 * records the orders (a rollout without them has a smaller footprint and may chunk a slightly larger batch).  turns_per_launch == 1 describes evg_step.
 * Returns the number of kernel launches per rollout launch (>= 1) or a negative evg_status. */
EVG_API int evg_launch_plan(const evg_handle* h, int turns_per_launch, char* buf, int buflen);

EVG_API int evg_num_envs(const evg_handle* h);
/* bytes of persistent device state per env (for the roofline accounting in DESIGN.md) */
EVG_API int evg_state_bytes_per_env(const evg_handle* h);
EVG_API const char* evg_last_error(void);
EVG_API int evg_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------------------------------------------
 * The Smart_State learner's n-step replay memory on the device (agents/Smart_State/Multi_Step.py NStepModule + NStepReplayMemory, DQNAgent.py:312-385
 * remember_game_state / end_of_episode / optimize_model's batch).  Added under ABI 7: new functions and one new descriptor struct; nothing that existed
 * changed.
 *
 * Storage is caller-owned device memory described by an evg_replay descriptor, allocated once (everglades_amd.SmartReplay does it).  It is a ring of `slots` TURNS,
 * not of transitions: slot t % slots holds record t, the turn-t state of every (env, seat) -- N envs x S seats, S = 1 for evg_step_vs_policy_smart_q,
 * S = 2 for evg_step_smart_q.  A record is the compact features of the observation the agent acted on (the `features` views a step writes for the NEXT
 * turn: pass slot t + 1 to step t), the {swarm, direction} rows step t wrote (`directions` view of slot t) and the metadata evg_replay_record writes.
 * While record t is the newest one, slot (t + 1) % slots already holds the features of record t + 1, so the ring keeps slots - 1 turns: records
 * t - slots + 2 .. t.  A record is sampled only once it is FINALISED (its n-step sum is known) and only while both it and its next record (n turns later,
 * same episode) are kept: slots >= n_step + 2.  One turn of 65 536 envs already holds more transitions than the reference's MEMORY_SIZE (100 000).
 *
 * Layout (record r = (slot * N + env) * S + seat; every buffer 16-byte aligned):
 *   shared      float [slots] x EVG_REPLAY_SHARED_STRIDE(N, S)   slot k = shared [N][S][34] at shared + k * stride (padded to 16 bytes)
 *   swarm       float [slots][N][S][12][13]
 *   directions  int32 [slots] x EVG_REPLAY_DIRS_STRIDE(N, S)     slot k = [N][S][7][2] {swarm, direction}
 *   reward      double [slots][N][S][2]   {shaped reward of the turn, n-step summed reward (valid once finalised)}
 *   meta        int32 [slots][N][S][4]    {turn number in the episode, episode index on the handle, flags EVG_REPLAY_F_*, 0}
 *   count       uint8 [slots][N][S]       transitions of the record: 0 until finalised
 *   env_state   int32 [N][4]              per env: turn, episode, records of the episode kept, frozen (set by evg_replay_clear, advanced by record)
 *   gamma_pow   double [n_step]           gamma ** k for k < n_step, computed on the HOST (Python's float power; a device pow may differ in the last bit)
 *   scan        int32 [EVG_REPLAY_SCAN_INTS(slots, N, S)]  work space of evg_replay_sample / evg_replay_size
 *   ctl         uint64 [4]                {sample calls so far, status bits EVG_REPLAY_S_*, transitions counted by the last scan, call index in use}
 *
 * Prioritized sampling (include/evg_replay_priority.h, libevg_priority.so) adds three caller-owned buffers next to these:
 *   plane       float [slots][N][S][8]    one 32-byte row per record, 16-byte aligned.  Entry k < 7: the weight w = priority ** alpha of the record's
 *                                         k-th transition (k counts the record's transition rows in ascending order-row order); 0.0f = never updated.
 *                                         Entry 7, as int bits: the stamp of the record the entries belong to,
 *                                             0x80000000 | (episode & 0x7FFFFF) << 8 | (turn & 0xFF)       from the record's meta {turn, episode}.
 *                                         A row whose stamp differs from its record's meta holds a previous occupant's weights: all its transitions
 *                                         count as never updated.  (So evg_replay_record knows nothing of the plane and recording costs nothing more.)
 *   pscan       uint64 [EVG_REPLAY_PSCAN_WORDS(slots, N, S)]  work space of the prioritized sample, 8-byte aligned
 *   pctl        uint64 [4]                {float bits of wmax: the largest weight stored since the last clear (1.0f after it); Q: the sum of the integer
 *                                         weights of the last scan; the least integer weight of the last batch; 0}, 8-byte aligned
 * ------------------------------------------------------------------------------------------------------------------------------------------------- */
#define EVG_REPLAY_SHARED_STRIDE(N, S) (((int64_t)(N) * (S) * 34 + 3) / 4 * 4)
#define EVG_REPLAY_DIRS_STRIDE(N, S) (((int64_t)(N) * (S) * 14 + 3) / 4 * 4)
#define EVG_REPLAY_SCAN_INTS(slots, N, S) (((int64_t)(slots) * (N) * (S) + 3) / 4 + ((int64_t)(slots) * (N) * (S) + 1023) / 1024)
enum { EVG_REPLAY_F_NOT_DONE = 1, EVG_REPLAY_F_FINAL = 2 };
/* status bits of ctl[1] (sticky until evg_replay_clear): a sample from an empty memory wrote zeros; a gather got a handle that names no transition */
enum { EVG_REPLAY_S_EMPTY = 1, EVG_REPLAY_S_BAD_HANDLE = 2 };
/* reward shaping of utils/reward_shaping.py(player, rewardArray, done, turnNum), evaluated in float64 in the reference's order of operations */
enum {
    EVG_SHAPE_NORMALIZED_SCORE = 0,     /* rewardArray[player]                                                    */
    EVG_SHAPE_BASIC_REWARD = 1,         /* done and won: 1.0, else 0.0                                            */
    EVG_SHAPE_PENALIZE_LONG_GAMES = 2,  /* done: won 100.0, else -0.1; not done: -0.001                           */
    EVG_SHAPE_REWARD_SHORT_GAMES = 3,   /* done: won (150.0 - turnNum) / 150.0, else -1.0; not done: 0.0          */
    EVG_SHAPE_TRANSITION = 4,           /* transition(from, to, K, i_episode): ratio = min(1.0, i_episode / K), from * (1.0 - ratio) + to * ratio */
    EVG_SHAPE_CUSTOM = 5                /* the caller's float32 [N][S] of evg_replay_record                       */
};

typedef struct evg_replay {
    int32_t slots;                 /* >= n_step + 2 (the ring keeps slots - 1 turns)                                        */
    int32_t num_seats;             /* S: 1 or 2                                                                             */
    int32_t seat;                  /* S == 1: the learner's seat, 0 or 1 (the reward's player); ignored for S == 2          */
    int32_t n_step;                /* >= 1 (N_STEP of DQNAgent.py)                                                          */
    int32_t shaping;               /* EVG_SHAPE_*                                                                           */
    int32_t shaping_from, shaping_to;   /* EVG_SHAPE_TRANSITION: the two functions (EVG_SHAPE_NORMALIZED_SCORE .. _REWARD_SHORT_GAMES) */
    int32_t transition_episodes;   /* EVG_SHAPE_TRANSITION: fully_transitioned_episode_num K >= 1                           */
    int64_t episode_base;          /* i_episode = episode_base + 1 + the env's episode index on the handle                  */
    float* shared;
    float* swarm;
    int32_t* directions;
    double* reward;
    int32_t* meta;
    uint8_t* count;
    int32_t* env_state;
    const double* gamma_pow;
    int32_t* scan;
    unsigned long long* ctl;
} evg_replay;

/* Empties the memory (count, meta, reward, status) and sets every env's counters from the handle's state as it will be when the stream reaches the
 * call: turn = current turn, episode = the handle's episode index, frozen = finished without auto_reset.  Call it after evg_reset / evg_set_state.
 * Enqueued on `stream`; no synchronisation. */
EVG_API int evg_replay_clear(evg_handle* h, const evg_replay* m, void* stream);
/* One launch after step `turn` (0, 1, 2, ... since the last clear; the caller's counter, so that a loop can be captured): writes record `turn`'s
 * metadata and finalises what the n-step rule allows (Multi_Step.py getSummedReward / addGameToReplayMemory):
 *   - the turn's shaped reward, from reward_in [N][2] (player = seat) and done_in [N] of the step, or from custom_in float [N][S] (EVG_SHAPE_CUSTOM);
 *   - record turn - n of the same episode: summed = r[s] + sum_{k<n} gamma_pow[k] * r[s+k+1] (the first future term is not discounted, as in the
 *     reference), not_done = 1 (its next record, turn, exists);
 *   - if the step ended the episode, records turn - n + 1 .. turn of it get their truncated sums and not_done = 0; the env's counters then start the
 *     next episode (turn 0, episode + 1) or, without auto_reset, freeze it: a frozen env records nothing;
 *   - a finalised record holds one transition per order row whose swarm is in 0..11, is not named by an earlier row, and whose direction is not 0
 *     (node_moved_to = direction - 1 and -1 means "no action"); the transition's action is direction - 1;
 *   - slot (turn + 1) % slots is emptied: the step has just overwritten its features with record turn + 1's.
 * reward_in / done_in / custom_in: device; reward_in 8-byte aligned. */
EVG_API int evg_replay_record(evg_handle* h, const evg_replay* m, int64_t turn, const float* reward_in, const uint8_t* done_in, const float* custom_in,
                              void* stream);
/* The number of transitions of the memory, counted on the device (a scan over the per-record counts) into ctl[2]; no host read-back. */
EVG_API int evg_replay_size(evg_handle* h, const evg_replay* m, void* stream);
/* optimize_model's batch (DQNAgent.py:336-385; three launches: count, draw, gather) for `batch` transitions drawn uniformly WITH replacement over the transitions of the memory (the
 * reference's random.sample draws without replacement): draw i is Philox(seed, call index, i), the call index being ctl[0] (incremented by the call,
 * on the device).  Outputs, row i (all 16-byte aligned):
 *   swarm_obs   float [batch][59]      shared(34) ++ swarm[s](13) ++ onehot(s)  (create_swarm_obs of the acted-on observation)
 *   action      int64 [batch]          direction - 1
 *   next_state  float [batch][12][59]  the 12 swarm rows of the record n turns later; zeros where not_done = 0
 *   reward      float [batch]          the float64 n-step sum rounded once
 *   not_done    uint8 [batch]          doesNotHitDone
 *   handles     int32 [batch][4]: {slot, env, seat, order row} of the drawn transitions (all -1 when the memory is empty); the gather reads them
 * An empty memory cannot be refused on the host (its size lives on the device): the outputs are then zeros and ctl[1] gets EVG_REPLAY_S_EMPTY. */
EVG_API int evg_replay_sample(evg_handle* h, const evg_replay* m, int batch, uint64_t seed, float* swarm_obs, int64_t* action, float* next_state,
                              float* reward, uint8_t* not_done, int32_t* handles, void* stream);
/* The same outputs for caller-chosen handles int32 [batch][4] (deterministic).  A handle that names no transition of the memory gets zeros and sets
 * EVG_REPLAY_S_BAD_HANDLE in ctl[1]. */
EVG_API int evg_replay_gather(evg_handle* h, const evg_replay* m, int batch, const int32_t* handles, float* swarm_obs, int64_t* action, float* next_state,
                              float* reward, uint8_t* not_done, void* stream);

/* ---- The Smart_State Q network, inference only (agents/Smart_State/QNetwork.py: relu(fc3(relu(fc2(relu(fc1(x))))))) ------------------------------
 * The consumer's network stays the consumer's: its weights are its own fp32 tensors (nn.Linear layout, contiguous, 16-byte aligned), read in place on
 * every call, so an optimizer step or a load_state_dict takes effect without rebinding.  Training (autograd, the optimizer) stays with the consumer.
 *   set p:   w1[p] [h1][59], b1[p] [h1], w2[p] [h2][h1], b2[p] [h2], w3[p] [5][h2], b3[p] [5]           h1, h2 in 1..64
 * Numerics (bit-exact, reproducible by a host model): every pre-activation is acc = b[j], then acc = fmaf(W[j][k], x[k], acc) for k ascending over the
 * layer's input index; then torch's ReLU, acc < 0 ? 0 : acc, on the two hidden layers, and on the output layer when final_relu is set (the reference's
 * QNetwork applies it).  A NaN stays a NaN through every ReLU (not fmaxf, which would drop it: a diverged network must not look finite); Inf, overflow
 * inside the chain, Inf * 0 = NaN and subnormals (kept, never flushed) all follow the IEEE fmaf chain.  The sign of a zero is not part of the contract.
 * Padding is never visible: hidden units the kernel pads a layer with (index >= h1, >= h2) enter the next layer as exact zeros whatever the row holds,
 * so a non-finite input reaches exactly the outputs the chain says it reaches and no other row.  Input row of a compact layout: x = shared(34) ++ swarm[s](13) ++ onehot(s)(12); the chain's prefix b1[j] + the 34 shared terms is computed once
 * per env and continued per swarm, the one-hot term at position 47 + s is acc + w1[j][47 + s] (a zero term leaves the chain unchanged), so the compact
 * and the expanded layouts give equal Q for the same features.
 * Layouts (rows R; any R >= 1 up to 2^30, independent of the handle's N: the handle only names the device):
 *   EVG_QNET_COMPACT        in0 = shared [R][34], in1 = swarm [R][12][13]        -> q_out [R][12][5]     (num_sets 1)
 *   EVG_QNET_COMPACT_SEATS  in0 = shared [R][2][34], in1 = swarm [R][2][12][13]  -> q_out [R][2][12][5]  (num_sets 2: seat p uses set p)
 *   EVG_QNET_EXPANDED       in0 = x [R][59], in1 = NULL                          -> q_out [R][5]         (num_sets 1)
 * One launch on `stream`, no synchronisation, nothing allocated.  Refused with EVG_ERR_INVALID (nothing launched): struct_size != sizeof(evg_qnet), h1 or
 * h2 outside 1..64, final_relu not 0/1, an unknown layout, a num_sets the layout does not take, a NULL or not 16-byte aligned pointer, R outside 1..2^30.
 * The output is a plain tensor of values: gradients of the network (optimize_model's policy forward) stay with the consumer. */
enum { EVG_QNET_COMPACT = 0, EVG_QNET_COMPACT_SEATS = 1, EVG_QNET_EXPANDED = 2 };
#define EVG_QNET_MAX_HIDDEN 64
#define EVG_QNET_MAX_ROWS (1LL << 30)
typedef struct evg_qnet {
    uint32_t struct_size;          /* sizeof(evg_qnet)                                                                      */
    int32_t h1, h2;                /* hidden sizes, 1..64 (fc1_size / fc2_size of the reference's pickles; default 60 / 60)  */
    int32_t final_relu;            /* 0 / 1: the ReLU (q < 0 ? 0 : q, NaN kept) on the output layer                         */
    int32_t num_sets;              /* 1, or 2 for EVG_QNET_COMPACT_SEATS                                                    */
    const float* w1[2];
    const float* b1[2];
    const float* w2[2];
    const float* b2[2];
    const float* w3[2];
    const float* b3[2];
} evg_qnet;
EVG_API int evg_smart_qnet(evg_handle* h, const evg_qnet* net, int layout, int64_t rows, const float* in0, const float* in1, float* q_out, void* stream);

/* ---- The opponent league: a per-env scripted opponent, redrawn by weight each episode -----------------------------------------------------------------
 * agents/Smart_State/training_scripts/dqn_smart_state_cycled_training_with_importance.py: every episode the opponent is
 * random.choices(opposing_agents, opposing_agent_weights)[0] from 15 scripted bots (:68-160, :210), games and wins are tallied per bot (:281-285) and every
 * 50 episodes the weights move towards the bots the learner loses to (updateAgentWeights, :166-173, :319-322); evaluate_all.py is the same need with a
 * fixed opponent per game.  Added under ABI 7: new functions and one new descriptor struct; nothing that existed changed.
 *
 * A league is an ordered list of M members, 1 <= M <= EVG_LEAGUE_MAX_MEMBERS, each an EVG_POLICY_* id.  Ids may repeat (the script lists random_actions
 * and random_actions_2, same_commands and same_commands_2): repeated ids are distinct members with their own agent objects and counters.  The league plays
 * seat 1 - seat against the caller's `seat`.  Storage is caller-owned device memory (everglades_amd.OpponentLeague allocates it):
 *   weights  const double [M]      read when an episode starts, so the caller may rewrite it on the stream at any time (evg_league_importance does)
 *   assign   uint8 [N]             the member env e plays in its current episode
 *   objects  uint32 [M][3][N]      member m's agent object of env e: the three words the handle keeps per (env, player) -- {cycle word, SwarmAgent's
 *                                  attack list, dfs_attack's call counter} at objects[(m * 3 + w) * N + e].  The CURRENT member's object is the handle's
 *                                  live one of the league seat (evg_get_run_state `agents`[e][1 - seat]); its slot here is stale until the member changes
 *   counts   uint64 [M][4]         {games, wins, ties, losses} against member m, seen from the caller's seat
 *   ctl      uint64 [2]            {status bits EVG_LEAGUE_S_* (sticky until evg_league_clear), reserved}
 * ASSIGNMENT.  resample = 1: the member of env e for its episode k is random.choices(range(M), weights) restated on a keyed draw (DESIGN.md section 4,
 * domain 5): cum[j] = weights[0] + ... + weights[j] in float64, left to right; total = cum[M - 1] + 0.0; x = u * total with u = (double)w / 4294967296.0,
 * w = word .x of the Philox block (domain 5, block 0, turn 0, node 0, player 1 - seat, group 0, episode k, global env id); member = the number of
 * j < M - 1 with cum[j] <= x, i.e. bisect(cum, x, 0, M - 1).  A 32-bit uniform stands in for random.random()'s 53 bits, as the coin of
 * random_actions_delay does.  If total is not finite or <= 0 (the reference raises ValueError) the env keeps its member and EVG_LEAGUE_S_BAD_WEIGHTS is set.
 * resample = 0: the caller writes assign (e.g. arange(N) % M) and it is never redrawn; a value >= M plays member 0 and sets EVG_LEAGUE_S_BAD_ASSIGN.
 * AGENT OBJECTS live across episodes like the script's 15 bot instances (:68-160).  When an env's member changes at an episode boundary the live words go
 * to the old member's slot and the new member's are loaded: a member playing for the first time still has first_turn set, a returning one continues
 * where it stopped.
 * COUNTERS.  The step that ends an episode (with or without auto_reset) increments counts[m][0] and one of counts[m][1..3].  The script decides from the
 * step's final rewards (:282-289: reward[0] > reward[1] win, == tie, else loss); the step's winner code is the same decision -- a finished game's rewards
 * are (1, -1), (0, 1) or (0, 0) for EVG_WINNER_P0 / P1 / TIE (everglades_env.py:37-61), so reward[seat] > reward[1 - seat] <=> winner == seat and
 * equality <=> EVG_WINNER_TIE, for either seat -- and is what the kernel uses.
 * WHERE.  With auto_reset the tally, the draw for episode k + 1 and the object swap run inside the step launch that ends episode k: the next launch finds
 * everything in place.  Without auto_reset the tally still happens in the step; draw and swap are evg_league_assign, enqueued after evg_reset(mask). */
#define EVG_LEAGUE_MAX_MEMBERS 16
enum { EVG_LEAGUE_S_BAD_WEIGHTS = 1, EVG_LEAGUE_S_BAD_ASSIGN = 2 };
typedef struct evg_league {
    int32_t num_members;                        /* M, 1..16                                             */
    int32_t members[EVG_LEAGUE_MAX_MEMBERS];    /* EVG_POLICY_* of member m (entries >= M are ignored)  */
    int32_t seat;                               /* the CALLER's seat, 0 or 1; the league plays 1 - seat */
    int32_t resample;                           /* 0 / 1                                                */
    const double* weights;
    uint8_t* assign;
    uint32_t* objects;
    unsigned long long* counts;
    unsigned long long* ctl;
} evg_league;
/* Every member object of every env becomes fresh (the values evg_scripted_reset writes), the handle's live objects of the league seat too; counters and
 * status are zeroed; with resample every env's member is drawn for its current episode index (resample = 0: assign is left to the caller). */
EVG_API int evg_league_clear(evg_handle* h, const evg_league* lg, void* stream);
/* Draw and swap for the envs of mask (device uint8 [N]; NULL = all), for their current episode: call it after an explicit evg_reset(mask).  A no-op for
 * resample = 0. */
EVG_API int evg_league_assign(evg_handle* h, const evg_league* lg, const uint8_t* mask, void* stream);
/* updateAgentWeights (:166-173) on the device: weights_out[m] = 1.0 where games == 0, else 1.0 - wins / games + 0.05, in float64 (both counters converted
 * exactly, one division, one subtraction, one addition -- Python's order).  weights_out: device double [M]; it may be lg->weights. */
EVG_API int evg_league_importance(evg_handle* h, const evg_league* lg, double* weights_out, void* stream);
/* evg_step_vs_policy_smart / evg_step_vs_policy_smart_q against the league: the argument lists of those two with `lg` where opponent_policy stands and
 * the caller's seat taken from lg->seat; shared_out / swarm_out are optional in both (both NULL or both set, both 16-byte aligned: the fused feature store
 * writes float4).  Argument checks, error codes, alignment rules and launch as in the seat family; a descriptor whose num_members, member ids or seat are out
 * of range (or that lacks a buffer) is refused with EVG_ERR_ARG before anything is enqueued.  Results -- every output, assign, and afterwards the handle's
 * state and run state, objects and counts -- are bit for bit those of playing every env against its member with the entry points above, the member's
 * object moved in and out of the handle at the episode boundaries.  Keyed-Philox handles only. */
EVG_API int evg_step_vs_league(evg_handle* h, const int32_t* actions, int actions_both_seats, const evg_league* lg, void* obs_seat_out,
                               float* shared_out, float* swarm_out, float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out,
                               uint8_t* status_out, void* stream);
EVG_API int evg_step_vs_league_q(evg_handle* h, const float* q, float epsilon, const float* epsilon_env, const evg_league* lg,
                                 void* obs_seat_out, float* shared_out, float* swarm_out,
                                 int32_t* actions_out, int32_t* directions_out, uint8_t* explored_out,
                                 float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);

/* ---- The Minimized agents (agents/Minimized: dqn_training, dqn_cycled_training(_with_importance), dqn_self_play, dqn_self_royale; Minimized_Rainbow) ----
 * Their input is the Smart_State feature vector (create_swarm_obs, DQNAgent.py:244-276: evg_smart_state_compact and the fused feature stores serve it) and
 * their n-step memory is the Smart_State one (the rows {swarm, node} below are what evg_replay_record takes as `directions`: action = node - 1).  What
 * differs is the head: the network output is 11 wide, one Q per NODE, and swarm_think (:215-242) orders {swarm, argmax + 1} -- no Move_Translation, no
 * location lookup, no observation.  Added under ABI 7: new functions and one new descriptor struct; nothing that existed changed.
 *
 * DECODE (q [N][12][11] float32, 16-byte aligned).  Per swarm: the FIRST maximum of its 11 values, a NaN is the maximum (torch.argmax / torch.max);
 * node = argmax + 1 in the caller's own numbering; sort key = the maximum, a NaN key counts as +inf.  Greedy rows (get_best_actions, :155-178): the swarms
 * sorted by key, ascending and stable; the first seven give rows {swarm, node}.  Exploration (get_action, :121-139; get_random_actions, :141-153) on the
 * two keyed Philox blocks of the Smart_State agent call (domain 4, key (env id, episode, turn, seat), blocks 0 and 1, halves h0[0..7], h1[0..7]; a seat
 * runs one agent family per turn): coin = (h0[7] << 16 | h1[7]) / 2^32 < epsilon in float64; swarms = partial Fisher-Yates over 0..11 with h0[0..6]
 * (j = i + ((h0[i] * (12 - i)) >> 16), swap); nodes = partial Fisher-Yates over the pool 0..10 with h1[0..6] (j = i + ((h1[i] * (11 - i)) >> 16), swap,
 * node_i = pool[i] + 1): np.random.choice(12, 7, replace=False) and np.random.choice(11, 7, replace=False) + 1.  The turn is the handle's.
 *
 * evg_minimized_get_action: DQNAgent.get_action for every env of the handle.  epsilon / epsilon_env as in evg_smart_get_action; epsilon == 0 with
 * epsilon_env == NULL is get_best_actions.  actions_out int32 [N][7][2] {swarm, node}; explored_out uint8 [N] or NULL. */
EVG_API int evg_minimized_get_action(evg_handle* h, const float* q, float epsilon, const float* epsilon_env, int seat, int32_t* actions_out,
                                     uint8_t* explored_out, void* stream);
/* The learner's turn from its Q values in one launch: evg_step_vs_policy_smart_q / evg_step_vs_league_q with the 11-way head -- their argument lists
 * without directions_out (actions_out is both the orders and what the replay memory records), q [N][12][11]; shared_out / swarm_out optional (both NULL or
 * both set, 16-byte aligned) and the same compact features.  Argument checks, error codes, alignment rules and launch as in those two.  Results -- every
 * output, and afterwards the handle's state and run state (league: assign, objects, counts) -- are bit for bit those of evg_minimized_get_action followed
 * by evg_step_vs_policy_smart / evg_step_vs_league with its rows.  Keyed-Philox handles only. */
EVG_API int evg_step_vs_policy_minimized_q(evg_handle* h, int seat, const float* q, float epsilon, const float* epsilon_env, int opponent_policy,
                                           void* obs_seat_out, float* shared_out, float* swarm_out, int32_t* actions_out, uint8_t* explored_out,
                                           float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);
EVG_API int evg_step_vs_league_minimized_q(evg_handle* h, const float* q, float epsilon, const float* epsilon_env, const evg_league* lg,
                                           void* obs_seat_out, float* shared_out, float* swarm_out, int32_t* actions_out, uint8_t* explored_out,
                                           float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);
/* Minimized SELF-PLAY in one launch (agents/Minimized/training_scripts/dqn_self_play.py: a DQNAgent on each seat, both learn): evg_step_smart_q with the
 * 11-way head -- its argument list without directions_out.  q float32 [N][2][12][11], row [e][p] seat p's network output (what a two-set evg_minimized_qnet
 * writes in one launch); epsilon0 / epsilon1 the seats' epsilons, or epsilon_env [N][2]; obs_out [N][2][105]; shared_out [N][2][34] / swarm_out
 * [N][2][12][13] both NULL or both set; actions_out int32 [N][2][7][2] {swarm, node} or NULL; explored_out uint8 [N][2] or NULL.  Alignment rules,
 * argument checks, error codes (bad input: EVG_ERR_ARG, nothing launched) and launch as evg_step_smart_q; keyed-Philox handles only.  Results -- every
 * output, and afterwards the handle's state and run state -- are bit for bit those of evg_minimized_get_action(q[:, p], eps_p, seat = p) for p = 0, 1,
 * evg_step with both seats' rows, evg_smart_state_compact for both players.  Rows are written for every env, frozen ones included. */
EVG_API int evg_step_minimized_q(evg_handle* h, const float* q, float epsilon0, float epsilon1, const float* epsilon_env, void* obs_out, float* shared_out,
                                 float* swarm_out, int32_t* actions_out, uint8_t* explored_out, float* reward_out, uint8_t* done_out, int8_t* winner_out,
                                 int32_t* scores_out, uint8_t* status_out, void* stream);
/* ... against a league ONE member of which is a network (dqn_staggered_self_play.py: seat 1 drawn once per episode from the second DQN or a scripted bot).
 * The league lg (layout unchanged) plays seat 1 - lg->seat exactly as in evg_step_vs_league_minimized_q: assignment, per-member tally, redraw at the
 * episode boundary, object swap, status bits.  q_member in 0..M-1 names the member that is the caller's second network, -1: none (every env bot-played);
 * anything else is EVG_ERR_ARG.  Where assign[e] == q_member the league seat's rows are evg_minimized_get_action(q[:, 1 - seat], eps, seat = 1 - seat)'s;
 * members[q_member] must still be a valid EVG_POLICY_* id (evg_league_clear / _assign / _importance are untouched by this), but that bot is never
 * consulted and the member's object words are carried through swaps unchanged.  The caller's seat is always decoded from q[e][seat].  Outputs as
 * evg_step_minimized_q (both seats' observations and features: the second network learns too), except:
 *   actions_out[e][league seat]   the rows PLAYED: the network's where it played, the bot's where a bot played, seven {0, 0} rows for a frozen
 *                                 bot-played env (its bot is not consulted)
 *   explored_out[e][league seat]  0 / 1 where the network played, 2 where a bot played (the second learner's own transitions are those != 2) */
EVG_API int evg_step_league_minimized_q(evg_handle* h, const float* q, float epsilon0, float epsilon1, const float* epsilon_env, const evg_league* lg,
                                        int q_member, void* obs_out, float* shared_out, float* swarm_out, int32_t* actions_out, uint8_t* explored_out,
                                        float* reward_out, uint8_t* done_out, int8_t* winner_out, int32_t* scores_out, uint8_t* status_out, void* stream);
/* The Minimized Q network, inference only (agents/Minimized/QNetwork.py: relu(fc2(relu(fc1(x)))), 59 -> h1 -> 11): evg_smart_qnet's contract -- weights
 * read in place on every call, the fmaf chain acc = b[j], fmaf(W[j][k], x[k], acc) for k ascending, torch's ReLU (acc < 0 ? 0 : acc: a NaN stays a NaN) on the hidden
 * layer and (final_relu: the reference applies it) on the output, padded hidden units (index >= h1) entering layer 2 as exact zeros, the compact prefix
 * and one-hot term -- with two layers:
 *   set p:   w1[p] [h1][59], b1[p] [h1], w2[p] [11][h1], b2[p] [11]           h1 in 1..128 (fc1_size of the reference's pickles; default 80)
 * Layouts and row limits as evg_smart_qnet, q_out [R][12][11], [R][2][12][11] or [R][11].  Refused with EVG_ERR_INVALID (nothing launched):
 * struct_size != sizeof(evg_mini_qnet), h1 outside 1..128, final_relu not 0/1, an unknown layout, a num_sets the layout does not take, a NULL or not
 * 16-byte aligned pointer, R outside 1..2^30. */
#define EVG_MINI_QNET_MAX_HIDDEN 128
typedef struct evg_mini_qnet {
    uint32_t struct_size;          /* sizeof(evg_mini_qnet)                                        */
    int32_t h1;                    /* hidden size, 1..128                                          */
    int32_t final_relu;            /* 0 / 1: the ReLU (NaN kept) on the output layer               */
    int32_t num_sets;              /* 1, or 2 for EVG_QNET_COMPACT_SEATS                           */
    const float* w1[2];
    const float* b1[2];
    const float* w2[2];
    const float* b2[2];
} evg_mini_qnet;
EVG_API int evg_minimized_qnet(evg_handle* h, const evg_mini_qnet* net, int layout, int64_t rows, const float* in0, const float* in1, float* q_out,
                               void* stream);

/* ---- Self-royale: a per-env Minimized Q network drawn from a population each episode ---------------------------------------------------------------------
 * agents/Minimized/training_scripts/dqn_self_royale.py (:42-62, :95-98, :157-166): each seat has a team of networks, random.choice(team) picks the member
 * that plays an episode, and only the members that played remember the game.  Per ENV here: member[e][p] is the network of team p that plays env e's
 * current episode.  Added under ABI 7: three functions and one descriptor struct; nothing that existed changed, and no step kernel knows about it -- the
 * forward writes the q [N][2][12][11] that evg_step_minimized_q takes, the assignment is a side kernel enqueued behind the step.
 *
 * A population is two teams of K[p] = num_members[p] networks (1..EVG_POP_MAX_MEMBERS each) of one hidden size h1, member m of team p being the weight
 * set {w1[p][m], b1[p][m], w2[p][m], b2[p][m]} in evg_mini_qnet's layout (read in place on every call).  Storage is caller-owned device memory
 * (everglades_amd.QPopulation allocates it):
 *   member   uint8 [N][2]          the member of team p that plays env e in its current episode
 *   counts   uint64 [2][16][4]     {games, wins, ties, losses} of member m of team p, seen from seat p
 *   ctl      uint64 [2]            {status bits EVG_POP_S_* (sticky until evg_population_clear), reserved}
 *   index    int32, 2 * scratch_rows words; first / count int32 [2][17]; hist int32, 2 * 17 * ceil(scratch_rows / 256) words: the bucket pass's results
 *                                  and scratch (below); scratch_rows >= the rows of every evg_population_qnet call.  scratch_rows BOUNDS index and
 *                                  hist, it is not their stride: a call of `rows` rows lays index out as [S][rows] (S seat slots: 2 for
 *                                  EVG_QNET_COMPACT_SEATS, else 1) -- seat slot s's list begins at index + s * rows, with the rows of THAT call -- and
 *                                  leaves the words behind S * rows as they were; hist is scratch, [S][17][ceil(rows / 256)] during the call
 * ASSIGNMENT.  The member of (env e, seat p) for episode k is random.choice(team) restated on a keyed draw (domain 6):
 * member = (w * K[p]) >> 32 with w = word .x of the Philox block (domain 6, block 0, turn 0, node 0, player p, group 0, episode k, global env id).  A team
 * of one draws nothing observable: its member is 0.  Keyed-Philox handles only.
 * FORWARD.  evg_population_qnet is evg_minimized_qnet with the weight set chosen per row; every Q row equals, bit for bit, what evg_minimized_qnet
 * writes for that row with the weights of team[seat][member[row]].  It first buckets the rows by member id -- a stable counting sort without global
 * atomics: with index read as [S][rows] of this call, index[s][first[s][m] .. + count[s][m]) lists the rows of member m of seat slot s in ascending order,
 * bin 16 the rows whose id is >= K; first / count [s] are the 17 bins' extents, valid until the next call -- and then runs one
 * workgroup set per (seat, member) over its list.  A row with an id >= K gets zeros and sets EVG_POP_S_BAD_MEMBER; such an id never selects weights. */
#define EVG_POP_MAX_MEMBERS 16
#define EVG_POP_MAX_ROWS (1 << 24)
enum { EVG_POP_S_BAD_MEMBER = 1 };
typedef struct evg_population {
    uint32_t struct_size;                       /* sizeof(evg_population)                          */
    int32_t h1;                                 /* hidden size of every member, 1..128             */
    int32_t final_relu;                         /* 0 / 1: the ReLU (NaN kept) on the output layer  */
    int32_t num_members[2];                     /* K[p], 1..16                                     */
    int32_t reserved;                           /* 0                                               */
    const float* w1[2][EVG_POP_MAX_MEMBERS];    /* entries >= K[p] are ignored                     */
    const float* b1[2][EVG_POP_MAX_MEMBERS];
    const float* w2[2][EVG_POP_MAX_MEMBERS];
    const float* b2[2][EVG_POP_MAX_MEMBERS];
    uint8_t* member;
    unsigned long long* counts;
    unsigned long long* ctl;
    int32_t* index;
    int32_t* first;
    int32_t* count;
    int32_t* hist;
    int64_t scratch_rows;
} evg_population;
/* Counts and status are zeroed and both seats' members of every env are drawn for the env's current episode. */
EVG_API int evg_population_clear(evg_handle* h, const evg_population* pop, void* stream);
/* For every env of mask (device uint8 [N]; NULL = all), in this order: history_out (uint8 [N][2] or NULL) receives the members that played, i.e. member
 * as it stands; winner (int8 [N], EVG_WINNER_*, or NULL) is tallied for both seats' members, each from its own seat (P0 / P1 = that seat's win, TIE, else
 * a loss; EVG_WINNER_NONE tallies nothing, a stored id >= K tallies nothing and sets EVG_POP_S_BAD_MEMBER); both seats' members are drawn for the episode
 * the handle's episode counter names when the call runs (evg_league_assign's convention).  With auto_reset call it behind every step with the step's
 * done_out as mask and its winner_out; after an explicit evg_reset(mask) with that mask and winner = NULL. */
EVG_API int evg_population_assign(evg_handle* h, const evg_population* pop, const uint8_t* mask, const int8_t* winner, uint8_t* history_out, void* stream);
/* The forward of `rows` rows (1..2^24, <= scratch_rows), layouts and tensors as evg_minimized_qnet:
 *   EVG_QNET_COMPACT_SEATS  member uint8 [rows][2] (e.g. pop->member itself); seat ignored; row [r][p] through team p
 *   EVG_QNET_COMPACT        member uint8 [rows]; every row through team `seat`
 *   EVG_QNET_EXPANDED       member uint8 [rows]; every row through team `seat` (the target networks on a sampled batch)
 * Four launches on `stream` (three of the bucket pass, one forward sized for the worst case: the counts stay on the device), no synchronisation, nothing
 * allocated.  Refused with EVG_ERR_INVALID (nothing launched): what evg_minimized_qnet refuses, struct_size, num_members outside 1..16, a NULL buffer of
 * the descriptor, a NULL member, seat outside 0..1, rows outside 1..2^24 or above scratch_rows. */
EVG_API int evg_population_qnet(evg_handle* h, const evg_population* pop, int layout, int64_t rows, int seat, const uint8_t* member, const float* in0,
                                const float* in1, float* q_out, void* stream);

/* ---- Smart_State self-royale: a per-env Smart_State Q network drawn from a population each episode ------------------------------------------------------
 * agents/Smart_State/training_scripts/dqn_smart_state_self_royale.py (:28, :51-70, :106-107, :148-201): evg_population's twin for the 59-h1-h2-5 network of
 * evg_smart_qnet.  Member m of team p is the weight set {w1, b1, w2, b2, w3, b3}[p][m] in evg_qnet's layouts (read in place on every call); all members
 * share h1, h2 and final_relu.  member, counts, ctl, index, first, count, hist and scratch_rows are evg_population's, with the same shapes and meaning.
 * ASSIGNMENT.  evg_smart_population_clear / _assign run the kernels of evg_population_clear / _assign: the same RNG domain 6, the same draw rule
 * member = (w * K[p]) >> 32 on the same Philox block.  The draw depends on the handle (seed, env id, episode, seat) and on K[p] alone, not on the
 * descriptor: on the same handle state they write the same member, counts and history as evg_population_* with the same team sizes, bit for bit -- TWO
 * POPULATIONS ON ONE HANDLE DRAW THE SAME MEMBERS (with equal team sizes; a Minimized and a Smart_State population, or two of one kind).  Keyed-Philox
 * handles only.
 * FORWARD.  evg_smart_population_qnet is evg_smart_qnet with the weight set chosen per row: every Q row equals, bit for bit, what evg_smart_qnet writes
 * for that row with the weights of team[seat][member[row]].  The bucket pass is evg_population_qnet's (rows of 5 or 60 floats); a row with an id >= K
 * gets zeros and sets EVG_POP_S_BAD_MEMBER, and such an id never selects weights. */
typedef struct evg_smart_population {
    uint32_t struct_size;                       /* sizeof(evg_smart_population)                    */
    int32_t h1, h2;                             /* hidden sizes of every member, 1..64             */
    int32_t final_relu;                         /* 0 / 1: the ReLU (NaN kept) on the output layer  */
    int32_t num_members[2];                     /* K[p], 1..16                                     */
    const float* w1[2][EVG_POP_MAX_MEMBERS];    /* entries >= K[p] are ignored                     */
    const float* b1[2][EVG_POP_MAX_MEMBERS];
    const float* w2[2][EVG_POP_MAX_MEMBERS];
    const float* b2[2][EVG_POP_MAX_MEMBERS];
    const float* w3[2][EVG_POP_MAX_MEMBERS];
    const float* b3[2][EVG_POP_MAX_MEMBERS];
    uint8_t* member;
    unsigned long long* counts;
    unsigned long long* ctl;
    int32_t* index;
    int32_t* first;
    int32_t* count;
    int32_t* hist;
    int64_t scratch_rows;
} evg_smart_population;
/* As evg_population_clear. */
EVG_API int evg_smart_population_clear(evg_handle* h, const evg_smart_population* pop, void* stream);
/* As evg_population_assign: history_out, the tally of winner, the draw, for the envs of mask. */
EVG_API int evg_smart_population_assign(evg_handle* h, const evg_smart_population* pop, const uint8_t* mask, const int8_t* winner, uint8_t* history_out,
                                        void* stream);
/* The forward of `rows` rows (1..2^24, <= scratch_rows), layouts and tensors as evg_smart_qnet, member as in evg_population_qnet:
 *   EVG_QNET_COMPACT_SEATS  member uint8 [rows][2]; seat ignored; row [r][p] through team p          -> q_out [rows][2][12][5]
 *   EVG_QNET_COMPACT        member uint8 [rows]; every row through team `seat`                       -> q_out [rows][12][5]
 *   EVG_QNET_EXPANDED       member uint8 [rows]; every row through team `seat`                       -> q_out [rows][5]
 * Four launches on `stream` (three of the bucket pass, one forward sized for the worst case), no synchronisation, nothing allocated.  Refused with
 * EVG_ERR_INVALID (nothing launched): what evg_smart_qnet and evg_population_qnet refuse; struct_size, h1 / h2 outside 1..64, num_members outside 1..16; a
 * NULL or misaligned weight or scratch pointer; seat outside 0..1; rows outside 1..2^24 or above scratch_rows. */
EVG_API int evg_smart_population_qnet(evg_handle* h, const evg_smart_population* pop, int layout, int64_t rows, int seat, const uint8_t* member,
                                      const float* in0, const float* in1, float* q_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVG_H */
