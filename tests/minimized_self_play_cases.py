"""What the CPU and the GPU tests of the Minimized self-play turn share (tests/test_minimized_self_play_abi.py, tests/test_gpu_minimized_self_play.py): the
league the GPU test of evg_step_league_minimized_q plays, and what the host model (tests/league_model.py) says it does."""
import numpy as np

import league_model as lm

SEED = 20261018
SIZES = (37, 70)            # envs: a full wavefront (32 envs) + 5, the last decode pass (4 envs) partial; two wavefronts + 6
# four members: the caller's second network, a cycling bot (its object has state: the swaps are visible), a member of weight zero that is never drawn, and
# the cycling bot's id again (a member of its own, with its own objects and counters)
MEMBERS = ["q", "cycle_rush_turn25", "swarm_agent", "cycle_rush_turn25"]
WEIGHTS = [2.0, 1.0, 0.0, 1.5]
# the league of the run without auto-reset (one episode, the assignment of league.clear()): three different bots around the network
MEMBERS_FROZEN = ["random_actions_delay", "q", "swarm_agent", "dfs_attack"]
# A game lasts at most 150 turns (the default tables' turn limit), so TURNS turns start at least EPISODES episodes in every env: 0 .. EPISODES - 1
EPISODES, TURNS = 4, 3 * 150 + 5


def model_histories(n, seat, episodes=EPISODES):
    """the members every env plays in its first `episodes` episodes, from the host model alone"""
    m = lm.League(SEED, 0, n, len(MEMBERS), seat, True, WEIGHTS)
    m.clear(np.zeros(n, np.int64))
    for k in range(1, episodes):
        for e in range(n):
            m.start_episode(e, k, np.asarray(lm.FRESH, np.uint32))
    return m.history
