"""What the CPU and the GPU tests of the step forms off their defaults share (tests/test_off_default_cases.py, tests/test_gpu_off_defaults.py): a seed whose
high word is in use, env ids at the top of the 32-bit range, the two leagues the GPU tests play and what the host model (tests/league_model.py) says they do."""
import numpy as np

import league_model as lm

SEED = 0x9E3779B97F4A7C15   # both words of the Philox key non-zero and different
SIZES = (37, 70)            # envs: a full wavefront (32 envs) + 5, the last decode pass (4 envs) partial; two wavefronts + 6
# a league of bots only (step_vs, step_vs_q): an RNG bot, a member of weight zero that is never drawn, a delay-coin bot, a cycling bot whose object has state
MEMBERS_BOTS = ["swarm_agent", "cycle_rush_turn25", "random_actions_delay", "cycle_rush_turn25"]
WEIGHTS_BOTS = [1.0, 0.0, 2.0, 1.5]
# a league around the caller's second network (step_q): the network, a cycling bot, a member of weight zero, the cycling bot's id again
MEMBERS_Q = ["q", "cycle_rush_turn25", "swarm_agent", "cycle_rush_turn25"]
WEIGHTS_Q = [2.0, 1.0, 0.0, 1.5]
LEAGUES = {"bots": (MEMBERS_BOTS, WEIGHTS_BOTS), "q": (MEMBERS_Q, WEIGHTS_Q)}
# A game lasts at most 150 turns (the default tables' turn limit), so TURNS turns start at least EPISODES episodes in every env: 0 .. EPISODES - 1
# (three episodes are the fewest in which an env can leave a member and return to it)
EPISODES = 3
TURNS = (EPISODES - 1) * 150 + 5


def base_for(n):
    """env_id_base of an n-env handle whose last env has the id 0xFFFFFFFF"""
    return 2 ** 32 - n


def model_histories(n, seat, league, episodes=EPISODES, seed=SEED):
    """the members every env plays in its first `episodes` episodes, from the host model alone"""
    members, weights = LEAGUES[league]
    m = lm.League(seed, base_for(n), n, len(members), seat, True, weights)
    m.clear(np.zeros(n, np.int64))
    for k in range(1, episodes):
        for e in range(n):
            m.start_episode(e, k, np.asarray(lm.FRESH, np.uint32))
    return m.history
