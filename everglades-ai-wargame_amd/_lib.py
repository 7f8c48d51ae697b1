"""ctypes binding of libevg.so (include/evg.h).  This is the whole FFI surface; no torch types cross it.

The library is built in-tree by `__graft_entry__.build()` / `make -C everglades-ai-wargame_amd/csrc`.
There is no CPU fallback: a missing library or a missing gfx950 device raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libevg.so")                # the product library; nothing in the environment changes that
DIAG_LIB_PATH = os.path.join(HERE, "libevg_diag.so")      # `make -C csrc diag`: phase ablation, 16-envs-per-wave variant, forced IEEE division
# `make -C csrc graphs`: rollout launch plans replayed as library-owned hipGraphs (A/B build; measured slower)
GRAPHS_LIB_PATH = os.path.join(HERE, "libevg_graphs.so")
# `make -C csrc priority`: the product plus the three entry points of include/evg_replay_priority.h (PrioritizedSmartReplay loads it: load_priority)
PRIORITY_LIB_PATH = os.path.join(HERE, "libevg_priority.so")
PRIORITY_EXPORTS = ["evg_replay_priority_clear", "evg_replay_update_priorities", "evg_replay_sample_prioritized"]
# `make -C csrc bf16`: the product plus the two entry points of include/evg_qnet_bf16.h (SmartQNetBf16 / MinimizedQNetBf16 load it: load_bf16)
BF16_LIB_PATH = os.path.join(HERE, "libevg_bf16.so")
BF16_EXPORTS = ["evg_smart_qnet_bf16", "evg_minimized_qnet_bf16"]
# `make -C csrc grad`: the product plus the two entry points of include/evg_qnet_grad.h (SmartQNet.with_grad / MinimizedQNet.with_grad load it: load_grad)
GRAD_LIB_PATH = os.path.join(HERE, "libevg_grad.so")
GRAD_EXPORTS = ["evg_smart_qnet_backward", "evg_minimized_qnet_backward"]
# EVG_QNET_GRAD_MAX_BLOCKS, EVG_SMART_QNET_GRAD_PARTIAL, EVG_MINI_QNET_GRAD_PARTIAL (floats per workgroup) of include/evg_qnet_grad.h
QNET_GRAD_MAX_BLOCKS, SMART_QNET_GRAD_PARTIAL, MINI_QNET_GRAD_PARTIAL = 512, 9360, 10384
# `make -C csrc learn`: the product plus GRAD_EXPORTS plus the two entry points of include/evg_learn.h (DqnLearner loads it: load_learn)
LEARN_LIB_PATH = os.path.join(HERE, "libevg_learn.so")
LEARN_EXPORTS = ["evg_td_head", "evg_adam_step"]
# EVG_TD_* modes, EVG_TD_HEAD_WORKSPACE_BYTES, EVG_TD_HEAD_MAX_BATCH, EVG_ADAM_MAX_TENSORS, EVG_ADAM_CTL_BYTES of include/evg_learn.h
TD_MODES = {"max_mean": 0, "max_max": 1, "double_mean": 2}
TD_HEAD_WORKSPACE_BYTES, TD_HEAD_MAX_BATCH, ADAM_MAX_TENSORS, ADAM_CTL_BYTES = 4096, 1 << 20, 6, 32
# `make -C csrc poplearn`: ... plus the six entry points of include/evg_pop_learn.h (PopulationLearner loads it: load_poplearn)
POPLEARN_LIB_PATH = os.path.join(HERE, "libevg_poplearn.so")
POPLEARN_EXPORTS = ["evg_pop_learn_expand_ids", "evg_pop_learn_take_rows", "evg_td_head_grouped", "evg_smart_population_backward", "evg_population_backward",
                    "evg_adam_step_grouped"]
# EVG_POP_LEARN_MAX_PARTIALS, EVG_TD_HEAD_GROUPED_WORKSPACE_BYTES, EVG_POP_LEARN_MAX_TENSORS of include/evg_pop_learn.h
POP_LEARN_MAX_PARTIALS, TD_HEAD_GROUPED_WORKSPACE_BYTES, POP_LEARN_MAX_TENSORS = 512 + 16, 4 * 1024 * 16, 6
# `make -C csrc popbf16`: the product plus BF16_EXPORTS plus the two entry points of include/evg_pop_bf16.h (QPopulationBf16 / SmartQPopulationBf16
# load it: load_popbf16)
POPBF16_LIB_PATH = os.path.join(HERE, "libevg_popbf16.so")
POPBF16_EXPORTS = ["evg_population_qnet_bf16", "evg_smart_population_qnet_bf16"]
# `make -C csrc dqn`: the product plus the three entry points of include/evg_dqn.h (DqnQNet, dqn_actions and dqn_get_action load it: load_dqn)
DQN_LIB_PATH = os.path.join(HERE, "libevg_dqn.so")
DQN_EXPORTS = ["evg_dqn_qnet", "evg_dqn_actions", "evg_dqn_get_action"]
# EVG_DQN_IN, EVG_DQN_OUT, EVG_DQN_MAX_HIDDEN, EVG_DQN_CHUNK, EVG_DQN_TINY_ROWS, EVG_DQN_SMALL_ROWS, EVG_DQN_MAX_BLOCKS and the input forms of
# include/evg_dqn.h
DQN_IN, DQN_OUT, DQN_MAX_HIDDEN, DQN_CHUNK, DQN_TINY_ROWS, DQN_SMALL_ROWS, DQN_MAX_BLOCKS = 105, 132, 528, 48, 4096, 16384, 256
DQN_ROWS, DQN_OBS_SEAT, DQN_OBS = 0, 1, 2
# `make -C csrc dqngrad`: libevg_dqn.so plus the entry point of include/evg_dqn_grad.h (DqnQNet.with_grad loads it: load_dqn_grad)
DQN_GRAD_LIB_PATH = os.path.join(HERE, "libevg_dqngrad.so")
DQN_GRAD_EXPORTS = ["evg_dqn_qnet_backward"]
# EVG_DQN_GRAD_MAX_ROWS, EVG_DQN_GRAD_TINY_ROWS, EVG_DQN_GRAD_MAX_BLOCKS, EVG_DQN_GRAD_SLICE_ROWS, EVG_DQN_GRAD_MAX_SLICES of include/evg_dqn_grad.h
DQN_GRAD_MAX_ROWS, DQN_GRAD_TINY_ROWS, DQN_GRAD_MAX_BLOCKS, DQN_GRAD_SLICE_ROWS, DQN_GRAD_MAX_SLICES = 1 << 16, 4096, 256, 128, 56
# `make -C csrc dqnlearn`: libevg_dqngrad.so plus the two entry points of include/evg_dqn_learn.h (DqnFamilyLearner loads it: load_dqn_learn)
DQN_LEARN_LIB_PATH = os.path.join(HERE, "libevg_dqnlearn.so")
DQN_LEARN_EXPORTS = ["evg_dqn_td_head", "evg_adam_step_wide"]
# EVG_DQN_TD_* modes, EVG_DQN_TD_ACTIONS, EVG_DQN_TD_MAX_BATCH, EVG_DQN_TD_MAX_BLOCKS, EVG_DQN_TD_WORKSPACE_BYTES, EVG_ADAM_WIDE_MAX_BLOCKS of
# include/evg_dqn_learn.h
DQN_TD_MODES = {"huber": 0, "squared": 1}
DQN_TD_ACTIONS, DQN_TD_MAX_BATCH, DQN_TD_MAX_BLOCKS, DQN_TD_WORKSPACE_BYTES, ADAM_WIDE_MAX_BLOCKS = 7, 1 << 20, 1024, 4096, 512
# `make -C csrc dqnreplay`: libevg_dqnlearn.so plus the five entry points of include/evg_dqn_replay.h (DqnReplay loads it: load_dqn_replay)
DQN_REPLAY_LIB_PATH = os.path.join(HERE, "libevg_dqnreplay.so")
DQN_REPLAY_EXPORTS = ["evg_dqn_replay_clear", "evg_dqn_replay_record", "evg_dqn_replay_size", "evg_dqn_replay_sample", "evg_dqn_replay_gather",
                      "evg_dqn_replay_priority_clear", "evg_dqn_replay_update_priorities", "evg_dqn_replay_sample_prioritized"]
# EVG_DQN_REPLAY_MAX_BATCH, _TILE, _GATHER_MAX_BLOCKS, _DRAW_MAX_BLOCKS, _S_BAD_ACTION, _TERMINAL_NEXT of include/evg_dqn_replay.h
DQN_REPLAY_MAX_BATCH, DQN_REPLAY_TILE, DQN_REPLAY_GATHER_MAX_BLOCKS, DQN_REPLAY_DRAW_MAX_BLOCKS = 1 << 20, 16, 2048, 256
DQN_REPLAY_S_BAD_ACTION, DQN_REPLAY_TERMINAL_NEXT = 8, 1
DQN_REPLAY_S_BAD_PRIORITY = 4                       # EVG_DQN_REPLAY_S_BAD_PRIORITY (= REPLAY_S_BAD_PRIORITY)


def dqn_replay_obs_stride(N, elem):
    """EVG_DQN_REPLAY_OBS_STRIDE: bytes from one slot's observations to the next (padded to 16)"""
    return (N * 105 * elem + 15) // 16 * 16


def dqn_replay_act_stride(N):
    """EVG_DQN_REPLAY_ACT_STRIDE: ints from one slot's order rows to the next"""
    return (N * 14 + 3) // 4 * 4


def dqn_replay_scan_ints(slots, N):
    """EVG_DQN_REPLAY_SCAN_INTS"""
    return (slots * N + 3) // 4 + (slots * N + 1023) // 1024


def dqn_replay_pscan_words(slots, N):
    """EVG_DQN_REPLAY_PSCAN_WORDS"""
    return (slots * N + 3) // 4 + 2 * ((slots * N + 1023) // 1024)


def dqn_grad_slices(rows):
    """EVG_DQN_GRAD_SLICES(rows)"""
    return 1 if rows <= DQN_GRAD_SLICE_ROWS else min((rows + DQN_GRAD_SLICE_ROWS - 1) // DQN_GRAD_SLICE_ROWS, DQN_GRAD_MAX_SLICES)


def dqn_grad_workspace_bytes(rows, h1):
    """EVG_DQN_GRAD_WORKSPACE_BYTES(rows, h1): a1 and d1 as [rows][h1 rounded up to 16] floats, and one partial per slice where there are several"""
    hp, s = (h1 + 15) // 16 * 16, dqn_grad_slices(rows)
    return 8 * rows * hp + (4 * s * (257 * hp + 144) if s > 1 else 0)
STAMPS_LIB_PATH =os.path.join(HERE, "libevg_stamps.so")  # `make -C csrc stamps`: in-kernel phase stamps (tools/stamps.py)

NUM_PLAYERS, NUM_GROUPS, NUM_NODES, NUM_UNITS, NUM_ACTIONS, OBS_LEN = 2, 12, 11, 100, 7, 105
MAX_SCORE = 3700
OBS_F32, OBS_F64, OBS_I16 = 0, 1, 2
ABI_VERSION = 7
ERR_COMM = -6         # EVG_ERR_COMM: RCCL missing or one of its calls failed (evg_comm_*, evg_gather_returns)
COMM_ID_BYTES = 128
ERR_FAULT = -5        # EVG_ERR_FAULT: the handle's fault word is set (evg_check_fault)
RNG_KEYED_PHILOX, RNG_STOCK_MT19937 = 0, 1
POLICY_NAMES = ["random", "cycle_rush_turn25", "cycle_rush_turn50", "swarm", "all_cycle", "base_rush_v1", "bull_rush",
                "cycle_target_node", "cycle_target_node1", "cycle_target_node11", "cycle_target_node11P2", "dfs_attack", "no_action",
                "random_actions_delay", "same_commands"]      # index = EVG_POLICY_* of include/evg.h (agents/State_Machine/<name>.py)
POLICY_ALIASES = {"random_actions": 0, "random_actions_2": 0, "swarm_agent": 3, "same_commands_2": 14}

EXPORTS = ["evg_default_tables", "evg_create", "evg_destroy", "evg_reset", "evg_step", "evg_observe", "evg_step_vs_policy", "evg_step_vs_policy_smart",
           "evg_step_vs_policy_smart_q", "evg_step_smart_q", "evg_replay_clear", "evg_replay_record", "evg_replay_size", "evg_replay_sample",
           "evg_replay_gather", "evg_smart_qnet",
           "evg_league_clear", "evg_league_assign", "evg_league_importance", "evg_step_vs_league", "evg_step_vs_league_q",
           "evg_minimized_get_action", "evg_step_vs_policy_minimized_q", "evg_step_vs_league_minimized_q", "evg_minimized_qnet",
           "evg_step_minimized_q", "evg_step_league_minimized_q",
           "evg_population_clear", "evg_population_assign", "evg_population_qnet",
           "evg_smart_population_clear", "evg_smart_population_assign", "evg_smart_population_qnet",
           "evg_observe_seat",
           "evg_random_actions_seat", "evg_smart_state_seat", "evg_smart_state_compact", "evg_check_fault", "evg_rollout_vs_policy", "evg_fog_of_war",
           "evg_sightings", "evg_smart_state", "evg_smart_actions", "evg_smart_get_action", "evg_move_table", "evg_random_actions", "evg_rollout_random", "evg_rollout_policies",
           "evg_scripted_actions", "evg_scripted_reset",
           "evg_get_state", "evg_set_state", "evg_get_run_state", "evg_set_run_state", "evg_seed_stock_entropy", "evg_get_stock_entropy", "evg_set_stock_entropy", "evg_episode_stats",
           "evg_episode_stats_device", "evg_pack_episode_results", "evg_pack_episode_results_counted", "evg_comm_unique_id", "evg_comm_init",
           "evg_gather_returns", "evg_comm_destroy", "evg_launch_plan", "evg_num_envs",
           "evg_state_bytes_per_env", "evg_last_error", "evg_abi_version"]


def kernel_source_files():
    """The files the product's device code is compiled from: every header and include of csrc/ (kernels, phases, RNG) plus the public header;
    NOT the host side (evg_abi.hip).  Sorted by name, so the hash does not depend on directory order."""
    import glob
    csrc = os.path.join(HERE, "csrc")
    files = sorted(f for pat in ("*.h", "*.inc", "evg_kernels.hip") for f in glob.glob(os.path.join(csrc, pat)))
    return files + [os.path.join(os.path.dirname(HERE), "include", "evg.h")]


_C_TOKEN = None


def _code_only(text):
    """C / C++ source without comments and with runs of white space collapsed (string and character literals kept as they are): what the compiler sees."""
    global _C_TOKEN
    import re
    if _C_TOKEN is None:
        _C_TOKEN = re.compile(r'''("(?:\\.|[^"\\])*"|'(?:\\.|[^'\\])*')|(/\*.*?\*/|//[^\n]*)''', re.S)
    text = _C_TOKEN.sub(lambda m: m.group(1) if m.group(1) is not None else " ", text)
    return " ".join(text.split())


def kernel_source_hash():
    """Identifies the kernel CODE a libevg.so was built from: the counter passes committed under profiles/ carry it, and bench.py uses
    only figures whose hash equals the one of the tree it runs in (the ONE definition: bench.py and tools/_prof.py call this).  Comments and white space
    are not part of it (round 6: a documentation change in include/evg.h used to invalidate every counter pass)."""
    import hashlib
    h = hashlib.sha256()
    for f in kernel_source_files():
        h.update(os.path.basename(f).encode())
        h.update(_code_only(open(f, encoding="utf-8", errors="replace").read()).encode())
    return h.hexdigest()[:16]


class EvgTables(C.Structure):
    _fields_ = [
        ("node_dist", (C.c_int32 * 12) * 12), ("node_control_points", C.c_int32 * 12),
        ("node_defense", C.c_double * 12), ("node_resource", C.c_int32 * 12),
        ("node_team_start", C.c_int32 * 12), ("p1_node_map", C.c_int32 * 12),
        ("num_unit_types", C.c_int32), ("unit_health", C.c_int32 * 4), ("unit_damage", C.c_int32 * 4),
        ("unit_speed", C.c_int32 * 4), ("unit_control", C.c_int32 * 4), ("unit_cost", C.c_int32 * 4),
        ("group_type", (C.c_int32 * 12) * 2), ("group_size", (C.c_int32 * 12) * 2), ("max_turns", C.c_int32),
    ]


class EvgConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("num_envs", C.c_int32), ("device_id", C.c_int32),
        ("seed", C.c_uint64), ("env_id_base", C.c_uint64), ("obs_dtype", C.c_int32), ("auto_reset", C.c_int32),
        ("rng_mode", C.c_int32), ("cache_mib", C.c_int32), ("tables", EvgTables),
    ]


class EvgReplay(C.Structure):
    """evg_replay of include/evg.h: the descriptor of a Smart_State replay memory (device pointers the caller owns)."""
    _fields_ = [
        ("slots", C.c_int32), ("num_seats", C.c_int32), ("seat", C.c_int32), ("n_step", C.c_int32), ("shaping", C.c_int32),
        ("shaping_from", C.c_int32), ("shaping_to", C.c_int32), ("transition_episodes", C.c_int32), ("episode_base", C.c_int64),
        ("shared", C.c_void_p), ("swarm", C.c_void_p), ("directions", C.c_void_p), ("reward", C.c_void_p), ("meta", C.c_void_p),
        ("count", C.c_void_p), ("env_state", C.c_void_p), ("gamma_pow", C.c_void_p), ("scan", C.c_void_p), ("ctl", C.c_void_p),
    ]


class EvgDqnReplay(C.Structure):
    """evg_dqn_replay of include/evg_dqn_replay.h: the descriptor of the agents/DQN family's replay memory (device pointers the caller owns)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("slots", C.c_int32), ("seat", C.c_int32), ("shaping", C.c_int32), ("shaping_from", C.c_int32),
        ("shaping_to", C.c_int32), ("transition_episodes", C.c_int32), ("reserved", C.c_int32), ("episode_base", C.c_int64),
        ("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("meta", C.c_void_p), ("valid", C.c_void_p),
        ("env_state", C.c_void_p), ("scan", C.c_void_p), ("ctl", C.c_void_p),
    ]


class EvgDqnReplayPriority(C.Structure):
    """evg_dqn_replay_priority of include/evg_dqn_replay.h: the weights, stamps and work space of prioritized sampling (device pointers)."""
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("weight", C.c_void_p), ("stamp", C.c_void_p), ("pscan", C.c_void_p),
                ("pctl", C.c_void_p)]


class EvgReplayPriority(C.Structure):
    """evg_replay_priority of include/evg.h: the weight plane and work space of prioritized sampling (device pointers the caller owns)."""
    _fields_ = [("alpha", C.c_float), ("plane", C.c_void_p), ("pscan", C.c_void_p), ("pctl", C.c_void_p)]


class EvgQnet(C.Structure):
    """evg_qnet of include/evg.h: the Smart_State Q network's weights (device pointers the caller owns, nn.Linear layout), one or two sets."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("final_relu", C.c_int32), ("num_sets", C.c_int32),
        ("w1", C.c_void_p * 2), ("b1", C.c_void_p * 2), ("w2", C.c_void_p * 2), ("b2", C.c_void_p * 2), ("w3", C.c_void_p * 2), ("b3", C.c_void_p * 2),
    ]


class EvgMiniQnet(C.Structure):
    """evg_mini_qnet of include/evg.h: the Minimized Q network's weights (device pointers the caller owns, nn.Linear layout), one or two sets."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("h1", C.c_int32), ("final_relu", C.c_int32), ("num_sets", C.c_int32),
        ("w1", C.c_void_p * 2), ("b1", C.c_void_p * 2), ("w2", C.c_void_p * 2), ("b2", C.c_void_p * 2),
    ]


class EvgDqnNet(C.Structure):
    """evg_dqn_net of include/evg_dqn.h: the agents/DQN Q network's weights (device pointers the caller owns, nn.Linear layout)."""
    _fields_ = [("struct_size", C.c_uint32), ("h1", C.c_int32), ("final_relu", C.c_int32), ("reserved", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p)]


class EvgDqnGrads(C.Structure):
    """evg_dqn_grads of include/evg_dqn_grad.h: where the agents/DQN network's parameter gradients go (device pointers the caller owns)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p)]


class EvgQnetGrads(C.Structure):
    """evg_qnet_grads of include/evg_qnet_grad.h: where the Smart_State network's parameter gradients go (device pointers the caller owns)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p)]


class EvgMiniQnetGrads(C.Structure):
    """evg_mini_qnet_grads of include/evg_qnet_grad.h: where the Minimized network's parameter gradients go."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p)]


class EvgTdHeadArgs(C.Structure):
    """evg_td_head_args of include/evg_learn.h: one sampled batch's operands and outputs (device pointers the caller owns)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("batch", C.c_int32), ("out", C.c_int32), ("scale", C.c_float),
                ("reserved", C.c_uint32), ("q_pred", C.c_void_p), ("action", C.c_void_p), ("q_next", C.c_void_p), ("q_select", C.c_void_p),
                ("reward", C.c_void_p), ("not_done", C.c_void_p), ("weights", C.c_void_p), ("gq", C.c_void_p), ("loss", C.c_void_p),
                ("priorities", C.c_void_p), ("estimated", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class EvgDqnTdHeadArgs(C.Structure):
    """evg_dqn_td_head_args of include/evg_dqn_learn.h: one batch's operands and outputs of the agents/DQN family's TD head (device pointers)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("batch", C.c_int32), ("gamma", C.c_float), ("q_pred", C.c_void_p),
                ("action", C.c_void_p), ("q_next", C.c_void_p), ("reward", C.c_void_p), ("not_done", C.c_void_p), ("weights", C.c_void_p),
                ("gq", C.c_void_p), ("loss", C.c_void_p), ("priorities", C.c_void_p), ("estimated", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class EvgAdamTensor(C.Structure):
    """evg_adam_tensor of include/evg_learn.h: one parameter tensor, its gradient and its two moments."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("count", C.c_int64)]


class EvgAdamArgs(C.Structure):
    """evg_adam_args of include/evg_learn.h: one Adam step over the n tensors of one network."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("clamp", C.c_float), ("fresh_state", C.c_int32), ("ctl", C.c_void_p), ("t", EvgAdamTensor * 6)]


class EvgPopLists(C.Structure):
    """evg_pop_lists of include/evg_pop_learn.h: the bucket pass's results that name each member's rows."""
    _fields_ = [("index", C.c_void_p), ("first", C.c_void_p), ("count", C.c_void_p), ("num_members", C.c_int32), ("batch", C.c_int32)]


class EvgTdHeadGroupedArgs(C.Structure):
    """evg_td_head_grouped_args of include/evg_pop_learn.h: evg_td_head's operands and the lists."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("td", EvgTdHeadArgs), ("lists", EvgPopLists)]


class EvgPopBackwardArgs(C.Structure):
    """evg_pop_backward_args of include/evg_pop_learn.h: the members' parameters [tensor][member] and where their gradients go."""
    _fields_ = [("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("final_relu", C.c_int32), ("clamp", C.c_float),
                ("reserved", C.c_uint32), ("lists", EvgPopLists), ("x", C.c_void_p), ("gq", C.c_void_p), ("param", (C.c_void_p * 16) * 6),
                ("grad", (C.c_void_p * 16) * 6), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class EvgAdamGroupedArgs(C.Structure):
    """evg_adam_grouped_args of include/evg_pop_learn.h: one Adam step per member over its n tensors, [tensor][member]."""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("clamp", C.c_float), ("fresh_state", C.c_int32), ("num_members", C.c_int32), ("reserved", C.c_uint32), ("count", C.c_void_p),
                ("ctl", C.c_void_p), ("elements", C.c_int64 * 6), ("param", (C.c_void_p * 16) * 6), ("grad", (C.c_void_p * 16) * 6),
                ("m", (C.c_void_p * 16) * 6), ("v", (C.c_void_p * 16) * 6)]


class EvgLeague(C.Structure):
    """evg_league of include/evg.h: the descriptor of an opponent league (device pointers the caller owns)."""
    _fields_ = [
        ("num_members", C.c_int32), ("members", C.c_int32 * 16), ("seat", C.c_int32), ("resample", C.c_int32),
        ("weights", C.c_void_p), ("assign", C.c_void_p), ("objects", C.c_void_p), ("counts", C.c_void_p), ("ctl", C.c_void_p),
    ]


class EvgPopulation(C.Structure):
    """evg_population of include/evg.h: two teams of Minimized Q networks and the per-env assignment (device pointers the caller owns)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("h1", C.c_int32), ("final_relu", C.c_int32), ("num_members", C.c_int32 * 2), ("reserved", C.c_int32),
        ("w1", (C.c_void_p * 16) * 2), ("b1", (C.c_void_p * 16) * 2), ("w2", (C.c_void_p * 16) * 2), ("b2", (C.c_void_p * 16) * 2),
        ("member", C.c_void_p), ("counts", C.c_void_p), ("ctl", C.c_void_p),
        ("index", C.c_void_p), ("first", C.c_void_p), ("count", C.c_void_p), ("hist", C.c_void_p), ("scratch_rows", C.c_int64),
    ]


class EvgSmartPopulation(C.Structure):
    """evg_smart_population of include/evg.h: two teams of Smart_State Q networks and the per-env assignment (device pointers the caller owns)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("final_relu", C.c_int32), ("num_members", C.c_int32 * 2),
        ("w1", (C.c_void_p * 16) * 2), ("b1", (C.c_void_p * 16) * 2), ("w2", (C.c_void_p * 16) * 2), ("b2", (C.c_void_p * 16) * 2),
        ("w3", (C.c_void_p * 16) * 2), ("b3", (C.c_void_p * 16) * 2),
        ("member", C.c_void_p), ("counts", C.c_void_p), ("ctl", C.c_void_p),
        ("index", C.c_void_p), ("first", C.c_void_p), ("count", C.c_void_p), ("hist", C.c_void_p), ("scratch_rows", C.c_int64),
    ]


POP_MAX_MEMBERS, POP_MAX_ROWS = 16, 1 << 24                   # EVG_POP_MAX_MEMBERS, EVG_POP_MAX_ROWS
POP_S_BAD_MEMBER = 1                                          # EVG_POP_S_*
POP_BINS, POP_BLOCK = 17, 256                                 # the bucket pass: 16 members + the bin of ids >= K; rows per workgroup
LEAGUE_MAX_MEMBERS = 16
LEAGUE_S_BAD_WEIGHTS, LEAGUE_S_BAD_ASSIGN = 1, 2              # EVG_LEAGUE_S_*
ERR_ARG = -1          # EVG_ERR_ARG (= EVG_ERR_INVALID): a bad argument, e.g. a league descriptor out of range
QNET_COMPACT, QNET_COMPACT_SEATS, QNET_EXPANDED = 0, 1, 2     # EVG_QNET_*
QNET_MAX_HIDDEN, QNET_MAX_ROWS = 64, 1 << 30
MINI_QNET_MAX_HIDDEN, MINI_QNET_OUT = 128, 11                  # EVG_MINI_QNET_MAX_HIDDEN; the Minimized head: one Q per node


SHAPE_NAMES = ["normalized_score", "basic_reward", "penalize_long_games", "reward_short_games", "transition", "custom"]   # index = EVG_SHAPE_*
REPLAY_F_NOT_DONE, REPLAY_F_FINAL = 1, 2
REPLAY_S_EMPTY, REPLAY_S_BAD_HANDLE, REPLAY_S_BAD_PRIORITY = 1, 2, 4


class EvgError(RuntimeError):
    pass


class EvgFault(EvgError):
    """EVG_ERR_FAULT: a chunked rollout launch of the handle failed to hand a set of envs on; its state and results are not valid."""


_libs = {}


def _hip_runtimes_mapped():
    """Paths of the libamdhip64 images mapped into this process."""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if "libamdhip64" in os.path.basename(path):
                    found.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(found)


def load(path=None):
    """Load libevg.so (or, for diagnostics, the library at `path`: an explicit argument, never an environment variable);
    fail loudly when it has not been built (there is no fallback path)."""
    path = os.path.abspath(path or LIB_PATH)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise EvgError("%s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "or `make -C everglades-ai-wargame_amd/csrc`; this package has no CPU fallback" % path)
    # libevg.so shares streams and device pointers with PyTorch, so both must run on ONE HIP runtime
    # instance: import torch first, so that its libamdhip64.so.7 is the one already in the process when
    # the loader resolves libevg's NEEDED entry of the same SONAME.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    rts = _hip_runtimes_mapped()
    if len(rts) > 1:
        raise EvgError("two HIP runtimes are mapped into this process (%s): torch's stream handles and device pointers would be "
                       "invalid inside libevg.so -- rebuild libevg.so against the libamdhip64 that torch loads" % ", ".join(rts))
    vp = C.c_void_p
    if hasattr(L, "evg_abi_version"):
        L.evg_abi_version.restype = C.c_int
        if L.evg_abi_version() != ABI_VERSION:
            raise EvgError("%s: ABI version %d, binding expects %d (an older build of the library? rebuild it)" % (path, L.evg_abi_version(), ABI_VERSION))
    missing = [n for n in EXPORTS if not hasattr(L, n)]
    if missing:       # an older build of the library (e.g. a baseline kept for tools/ab.sh): say what it lacks instead of an AttributeError
        raise EvgError("%s does not export %s -- it was built from older sources than this binding (ABI %d); rebuild it" % (path, ", ".join(missing),
                                                                                                                            ABI_VERSION))
    L.evg_last_error.restype = C.c_char_p
    L.evg_abi_version.restype = C.c_int
    L.evg_default_tables.argtypes = [C.POINTER(EvgTables)]
    L.evg_default_tables.restype = None
    L.evg_create.argtypes = [C.POINTER(EvgConfig), C.POINTER(vp)]
    L.evg_destroy.argtypes = [vp]
    L.evg_destroy.restype = None
    L.evg_reset.argtypes = [vp, vp, vp, vp]
    L.evg_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_observe.argtypes = [vp, vp, vp]
    L.evg_step_vs_policy.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.evg_get_run_state.argtypes = [vp] * 7
    L.evg_set_run_state.argtypes = [vp] * 7
    L.evg_step_vs_policy_smart.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_step_vs_policy_smart_q.argtypes = [vp, C.c_int, vp, C.c_float, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_step_smart_q.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_observe_seat.argtypes = [vp, C.c_int, vp, vp]
    rp = C.POINTER(EvgReplay)
    L.evg_replay_clear.argtypes = [vp, rp, vp]
    L.evg_replay_record.argtypes = [vp, rp, C.c_int64, vp, vp, vp, vp]
    L.evg_replay_size.argtypes = [vp, rp, vp]
    L.evg_replay_sample.argtypes = [vp, rp, C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    L.evg_replay_gather.argtypes = [vp, rp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "evg_replay_priority_clear"):      # libevg_priority.so only
        pr = C.POINTER(EvgReplayPriority)
        L.evg_replay_priority_clear.argtypes = [vp, rp, pr, vp]
        L.evg_replay_update_priorities.argtypes = [vp, rp, pr, C.c_int, vp, vp, vp]
        L.evg_replay_sample_prioritized.argtypes = [vp, rp, C.c_int, C.c_uint64, vp, vp, vp, vp, vp, vp, pr, C.c_float, vp, vp]
    L.evg_smart_qnet.argtypes = [vp, C.POINTER(EvgQnet), C.c_int, C.c_int64, vp, vp, vp, vp]
    if hasattr(L, "evg_smart_qnet_bf16"):            # libevg_bf16.so only
        L.evg_smart_qnet_bf16.argtypes = [vp, C.POINTER(EvgQnet), C.c_int, C.c_int64, vp, vp, vp, vp]
        L.evg_minimized_qnet_bf16.argtypes = [vp, C.POINTER(EvgMiniQnet), C.c_int, C.c_int64, vp, vp, vp, vp]
    if hasattr(L, "evg_smart_qnet_backward"):        # libevg_grad.so only
        L.evg_smart_qnet_backward.argtypes = [vp, C.POINTER(EvgQnet), C.c_int64, vp, vp, C.POINTER(EvgQnetGrads), vp, C.c_int64, C.c_float, vp]
        L.evg_minimized_qnet_backward.argtypes = [vp, C.POINTER(EvgMiniQnet), C.c_int64, vp, vp, C.POINTER(EvgMiniQnetGrads), vp, C.c_int64, C.c_float, vp]
    if hasattr(L, "evg_td_head"):                    # libevg_learn.so only
        L.evg_td_head.argtypes = [vp, C.POINTER(EvgTdHeadArgs), vp]
        L.evg_adam_step.argtypes = [vp, C.POINTER(EvgAdamArgs), vp]
    if hasattr(L, "evg_td_head_grouped"):            # libevg_poplearn.so only
        L.evg_pop_learn_expand_ids.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp]
        L.evg_pop_learn_take_rows.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, vp, vp]
        L.evg_td_head_grouped.argtypes = [vp, C.POINTER(EvgTdHeadGroupedArgs), vp]
        L.evg_smart_population_backward.argtypes = [vp, C.POINTER(EvgPopBackwardArgs), vp]
        L.evg_population_backward.argtypes = [vp, C.POINTER(EvgPopBackwardArgs), vp]
        L.evg_adam_step_grouped.argtypes = [vp, C.POINTER(EvgAdamGroupedArgs), vp]
    if hasattr(L, "evg_dqn_qnet"):                   # libevg_dqn.so only
        L.evg_dqn_qnet.argtypes = [vp, C.POINTER(EvgDqnNet), C.c_int, C.c_int, C.c_int64, vp, vp, vp]
        L.evg_dqn_actions.argtypes = [vp, vp, vp, vp]
        L.evg_dqn_get_action.argtypes = [vp, vp, C.c_float, vp, C.c_int, vp, vp, vp]
    if hasattr(L, "evg_dqn_qnet_backward"):          # libevg_dqngrad.so only
        L.evg_dqn_qnet_backward.argtypes = [vp, C.POINTER(EvgDqnNet), C.c_int64, vp, vp, vp, C.POINTER(EvgDqnGrads), vp, C.c_int64, C.c_float, vp]
    if hasattr(L, "evg_dqn_td_head"):                # libevg_dqnlearn.so only
        L.evg_dqn_td_head.argtypes = [vp, C.POINTER(EvgDqnTdHeadArgs), vp]
        L.evg_adam_step_wide.argtypes = [vp, C.POINTER(EvgAdamArgs), vp]
    if hasattr(L, "evg_dqn_replay_clear"):           # libevg_dqnreplay.so only
        dr = C.POINTER(EvgDqnReplay)
        L.evg_dqn_replay_clear.argtypes = [vp, dr, vp]
        L.evg_dqn_replay_record.argtypes = [vp, dr, C.c_int64, vp, vp, vp, vp]
        L.evg_dqn_replay_size.argtypes = [vp, dr, vp]
        L.evg_dqn_replay_sample.argtypes = [vp, dr, C.c_int, C.c_uint64, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.evg_dqn_replay_gather.argtypes = [vp, dr, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        dp = C.POINTER(EvgDqnReplayPriority)
        L.evg_dqn_replay_priority_clear.argtypes = [vp, dr, dp, vp]
        L.evg_dqn_replay_update_priorities.argtypes = [vp, dr, dp, C.c_int, vp, vp, vp]
        L.evg_dqn_replay_sample_prioritized.argtypes = [vp, dr, dp, C.c_int, C.c_uint64, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp]
    lp = C.POINTER(EvgLeague)
    L.evg_league_clear.argtypes = [vp, lp, vp]
    L.evg_league_assign.argtypes = [vp, lp, vp, vp]
    L.evg_league_importance.argtypes = [vp, lp, vp, vp]
    L.evg_step_vs_league.argtypes = [vp, vp, C.c_int, lp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_step_vs_league_q.argtypes = [vp, vp, C.c_float, vp, lp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_minimized_get_action.argtypes = [vp, vp, C.c_float, vp, C.c_int, vp, vp, vp]
    L.evg_step_vs_policy_minimized_q.argtypes = [vp, C.c_int, vp, C.c_float, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_step_vs_league_minimized_q.argtypes = [vp, vp, C.c_float, vp, lp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_step_minimized_q.argtypes = [vp, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_step_league_minimized_q.argtypes = [vp, vp, C.c_float, C.c_float, vp, lp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.evg_minimized_qnet.argtypes = [vp, C.POINTER(EvgMiniQnet), C.c_int, C.c_int64, vp, vp, vp, vp]
    pp = C.POINTER(EvgPopulation)
    L.evg_population_clear.argtypes = [vp, pp, vp]
    L.evg_population_assign.argtypes = [vp, pp, vp, vp, vp, vp]
    L.evg_population_qnet.argtypes = [vp, pp, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
    sp = C.POINTER(EvgSmartPopulation)
    L.evg_smart_population_clear.argtypes = [vp, sp, vp]
    L.evg_smart_population_assign.argtypes = [vp, sp, vp, vp, vp, vp]
    L.evg_smart_population_qnet.argtypes = [vp, sp, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
    if hasattr(L, "evg_population_qnet_bf16"):       # libevg_popbf16.so only
        L.evg_population_qnet_bf16.argtypes = [vp, pp, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
        L.evg_smart_population_qnet_bf16.argtypes = [vp, sp, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
    L.evg_random_actions_seat.argtypes = [vp, C.c_int, vp, vp]
    L.evg_smart_state_seat.argtypes = [vp, vp, vp, vp]
    L.evg_smart_state_compact.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.evg_check_fault.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.evg_rollout_vs_policy.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.evg_fog_of_war.argtypes = [vp, vp, vp, vp]
    L.evg_sightings.argtypes = [vp, vp, vp]
    L.evg_smart_state.argtypes = [vp, C.c_int, vp, vp, vp]
    L.evg_smart_actions.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.evg_smart_get_action.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_float, vp, vp, vp, vp, vp]
    L.evg_move_table.argtypes = [vp]
    L.evg_move_table.restype = None
    L.evg_random_actions.argtypes = [vp, vp, vp]
    L.evg_rollout_random.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.evg_rollout_policies.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.evg_scripted_actions.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
    L.evg_scripted_reset.argtypes = [vp, vp]
    L.evg_get_state.argtypes = [vp, vp, vp, vp, vp]
    L.evg_set_state.argtypes = [vp, vp, vp, vp, vp]
    L.evg_seed_stock_entropy.argtypes = [vp, vp, vp]
    L.evg_get_stock_entropy.argtypes = [vp, vp]
    L.evg_set_stock_entropy.argtypes = [vp, vp]
    L.evg_episode_stats.argtypes = [vp, vp, vp, vp, vp]
    L.evg_episode_stats_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.evg_pack_episode_results.argtypes = [vp, vp, vp]
    L.evg_pack_episode_results_counted.argtypes = [vp, vp, vp, vp]
    L.evg_comm_unique_id.argtypes = [vp]
    L.evg_comm_init.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.evg_gather_returns.argtypes = [vp, C.c_int, vp, vp]
    L.evg_comm_destroy.argtypes = [vp]
    L.evg_launch_plan.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    L.evg_num_envs.argtypes = [vp]
    L.evg_state_bytes_per_env.argtypes = [vp]
    if hasattr(L, "evg_diag_configure"):      # diagnostic libraries only
        L.evg_diag_configure.argtypes = [vp, C.c_uint32, C.c_int, C.c_int]
    _libs[path] = L
    return L


def load_priority():
    """Load libevg_priority.so: libevg.so's sources built with -DEVG_PRIORITY, which exports the entry points of include/evg.h plus PRIORITY_EXPORTS
    (include/evg_replay_priority.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error (check(rc, this library))."""
    L = load(PRIORITY_LIB_PATH)
    missing = [n for n in PRIORITY_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc priority)" % (PRIORITY_LIB_PATH, ", ".join(missing)))
    return L


def load_bf16():
    """Load libevg_bf16.so: libevg.so's sources built with -DEVG_BF16, which exports the entry points of include/evg.h plus BF16_EXPORTS
    (include/evg_qnet_bf16.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error (check(rc, this library))."""
    L = load(BF16_LIB_PATH)
    missing = [n for n in BF16_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc bf16)" % (BF16_LIB_PATH, ", ".join(missing)))
    return L


def load_popbf16():
    """Load libevg_popbf16.so: libevg.so's sources built with -DEVG_BF16 -DEVG_POP_BF16, which exports the entry points of include/evg.h plus
    BF16_EXPORTS plus POPBF16_EXPORTS (include/evg_pop_bf16.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error."""
    L = load(POPBF16_LIB_PATH)
    missing = [n for n in BF16_EXPORTS + POPBF16_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc popbf16)" % (POPBF16_LIB_PATH, ", ".join(missing)))
    return L


def load_dqn():
    """Load libevg_dqn.so: libevg.so's sources built with -DEVG_DQN, which exports the entry points of include/evg.h plus DQN_EXPORTS
    (include/evg_dqn.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error (check(rc, this library))."""
    L = load(DQN_LIB_PATH)
    missing = [n for n in DQN_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc dqn)" % (DQN_LIB_PATH, ", ".join(missing)))
    return L


def load_dqn_grad():
    """Load libevg_dqngrad.so: libevg.so's sources built with -DEVG_DQN -DEVG_DQN_GRAD, which exports the entry points of include/evg.h plus DQN_EXPORTS
    plus DQN_GRAD_EXPORTS (include/evg_dqn_grad.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error."""
    L = load(DQN_GRAD_LIB_PATH)
    missing = [n for n in DQN_EXPORTS + DQN_GRAD_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc dqngrad)" % (DQN_GRAD_LIB_PATH, ", ".join(missing)))
    return L


def load_dqn_learn():
    """Load libevg_dqnlearn.so: libevg.so's sources built with -DEVG_DQN -DEVG_DQN_GRAD -DEVG_DQN_LEARN, which exports what libevg_dqngrad.so does plus
    DQN_LEARN_EXPORTS (include/evg_dqn_learn.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error."""
    L = load(DQN_LEARN_LIB_PATH)
    missing = [n for n in DQN_EXPORTS + DQN_GRAD_EXPORTS + DQN_LEARN_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc dqnlearn)" % (DQN_LEARN_LIB_PATH, ", ".join(missing)))
    return L


def load_dqn_replay():
    """Load libevg_dqnreplay.so: libevg.so's sources built with -DEVG_DQN -DEVG_DQN_GRAD -DEVG_DQN_LEARN -DEVG_DQN_REPLAY, which exports what
    libevg_dqnlearn.so does plus DQN_REPLAY_EXPORTS (include/evg_dqn_replay.h).  A handle of libevg.so is valid in it; a failed call's text is its own
    evg_last_error."""
    L = load(DQN_REPLAY_LIB_PATH)
    missing = [n for n in DQN_EXPORTS + DQN_GRAD_EXPORTS + DQN_LEARN_EXPORTS + DQN_REPLAY_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc dqnreplay)" % (DQN_REPLAY_LIB_PATH, ", ".join(missing)))
    return L


def load_grad():
    """Load libevg_grad.so: libevg.so's sources built with -DEVG_GRAD, which exports the entry points of include/evg.h plus GRAD_EXPORTS
    (include/evg_qnet_grad.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error (check(rc, this library))."""
    L = load(GRAD_LIB_PATH)
    missing = [n for n in GRAD_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc grad)" % (GRAD_LIB_PATH, ", ".join(missing)))
    return L


def load_learn():
    """Load libevg_learn.so: libevg.so's sources built with -DEVG_GRAD -DEVG_LEARN, which exports the entry points of include/evg.h plus GRAD_EXPORTS
    plus LEARN_EXPORTS (include/evg_learn.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error."""
    L = load(LEARN_LIB_PATH)
    missing = [n for n in GRAD_EXPORTS + LEARN_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc learn)" % (LEARN_LIB_PATH, ", ".join(missing)))
    return L


def load_poplearn():
    """Load libevg_poplearn.so: libevg.so's sources built with -DEVG_GRAD -DEVG_LEARN -DEVG_POP_LEARN, which exports what libevg_learn.so does plus
    POPLEARN_EXPORTS (include/evg_pop_learn.h).  A handle of libevg.so is valid in it; a failed call's text is its own evg_last_error."""
    L = load(POPLEARN_LIB_PATH)
    missing = [n for n in GRAD_EXPORTS + LEARN_EXPORTS + POPLEARN_EXPORTS if not hasattr(L, n)]
    if missing:
        raise EvgError("%s does not export %s; rebuild it (make -C everglades-ai-wargame_amd/csrc poplearn)" % (POPLEARN_LIB_PATH, ", ".join(missing)))
    return L


def check(rc, lib=None):
    if rc != 0:
        raise (EvgFault if rc == ERR_FAULT else EvgError)("libevg error %d: %s" % (rc, (lib or load()).evg_last_error().decode("utf-8", "replace")))
