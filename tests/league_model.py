"""Host model of the opponent league (everglades_amd.OpponentLeague, include/evg.h evg_league): our own numpy restatement of what
agents/Smart_State/training_scripts/dqn_smart_state_cycled_training_with_importance.py does around its episodes -- random.choices over the bots (:210), the
per-bot tally (:281-289), updateAgentWeights (:166-173), one bot object per list entry (:68-160) -- per env, with the choice's random() served from the
keyed stream.  This file is also the statement of RNG domain 5 (the league draw), next to oracle/rng_spec.py's domains 0..4:

  league (domain 5): the member an env plays in episode k: word 0 of block 0 with turn 0, node 0, group 0, player = the LEAGUE's seat, episode k, as a
                     fraction of 2^32, stands in for the random.random() inside random.choices (a 32-bit uniform for its 53 bits, as the delay coin).
"""
import numpy as np

import rng_spec

DOMAIN_LEAGUE = 5
FRESH = (0x112, 0xBA875421, 0)          # a new agent object: first_turn | group 1 | node 2, SwarmAgent's ATTACK_LIST, dfs_attack's call counter
S_BAD_WEIGHTS, S_BAD_ASSIGN = 1, 2
# the script's opposing_agents (:68-160) in its order, as EVG_POLICY_* names
SCRIPT_MEMBERS = ["random_actions_delay", "random_actions", "bull_rush", "all_cycle", "base_rush_v1", "cycle_rush_turn25", "cycle_rush_turn50",
                  "cycle_target_node", "cycle_target_node1", "cycle_target_node11", "cycle_target_node11P2", "random_actions_2", "same_commands_2",
                  "same_commands", "swarm_agent"]


def league_word(seed, env_id, episode, player):
    """the 32-bit word of the draw"""
    return rng_spec.philox4x32_10(rng_spec._ctr(DOMAIN_LEAGUE, 0, 0, 0, player, episode, env_id), rng_spec._key(seed))[0]


def league_u(seed, env_id, episode, player):
    return league_word(seed, env_id, episode, player) / 4294967296.0


def choose(u, weights):
    """random.choices(range(M), weights)[0] with random() = u: the member, or None where the reference raises ValueError (total <= 0 or not finite)."""
    w = [float(x) for x in weights]
    cum = []
    acc = None
    for x in w:                              # itertools.accumulate: float64 sums, left to right
        acc = x if acc is None else acc + x
        cum.append(acc)
    total = cum[-1] + 0.0
    if not (total > 0.0) or total == float("inf"):
        return None
    x = u * total
    return sum(1 for j in range(len(w) - 1) if cum[j] <= x)


def importance(counts):
    """updateAgentWeights (:166-173) over counts [M][4] = games, wins, ties, losses"""
    out = np.ones(len(counts), np.float64)
    for m, (games, wins) in enumerate(np.asarray(counts)[:, :2].tolist()):
        if games:
            out[m] = 1.0 - wins / games + 0.05
    return out


class League(object):
    """assignment, object store and counters of N envs; the caller moves the live object in and out of its handle as swap() says"""

    def __init__(self, seed, env_id_base, N, M, seat, resample, weights=None):
        self.seed, self.base, self.N, self.M, self.seat, self.resample = seed, env_id_base, N, M, seat, resample
        self.weights = np.ones(M, np.float64) if weights is None else np.asarray(weights, np.float64).copy()
        self.assign = np.zeros(N, np.uint8)
        self.objects = np.tile(np.asarray(FRESH, np.uint32)[None, :, None], (M, 1, N))
        self.counts = np.zeros((M, 4), np.int64)
        self.status = 0
        self.history = [[] for _ in range(N)]        # members played, per env, in order

    def member(self, e):
        m = int(self.assign[e])
        if m >= self.M:
            self.status |= S_BAD_ASSIGN
            return 0
        return m

    def draw(self, e, episode):
        """the member of env e for `episode` (the current one is kept where the reference would raise)"""
        m = choose(league_u(self.seed, self.base + e, episode, 1 - self.seat), self.weights)
        if m is None:
            self.status |= S_BAD_WEIGHTS
            return self.member(e)
        return m

    def clear(self, episodes):
        self.objects[:] = np.asarray(FRESH, np.uint32)[None, :, None]
        self.counts[:] = 0
        self.status = 0
        if self.resample:
            for e in range(self.N):
                if self.assign[e] >= self.M:
                    self.assign[e] = 0
                self.assign[e] = self.draw(e, int(episodes[e]))
        self.history = [[int(self.assign[e])] for e in range(self.N)]

    def tally(self, e, winner):
        """a step ended env e's episode with `winner` (EVG_WINNER_*: 0, 1, 2 = tie)"""
        m = self.member(e)
        self.counts[m, 0] += 1
        self.counts[m, 1 if winner == self.seat else (2 if winner == 2 else 3)] += 1

    def start_episode(self, e, episode, live):
        """env e starts `episode`: (new member, the live object to continue with); `live` = the three words of the handle's object"""
        old = self.member(e)
        if not self.resample:
            return old, live
        new = self.draw(e, episode)
        if new != old:
            self.objects[old, :, e] = live
            live = self.objects[new, :, e].copy()
            self.assign[e] = new
        self.history[e].append(new)
        return new, live
