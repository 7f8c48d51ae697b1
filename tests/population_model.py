"""Host model of self-royale (everglades_amd.QPopulation, include/evg.h evg_population): our own numpy restatement of what
agents/Minimized/training_scripts/dqn_self_royale.py does around its episodes -- random.choice(team) per seat (:95-98) and the per-member record of the
games played -- per env, with the choice served from the keyed stream.  This file is also the statement of RNG domain 6 (the population draw), next to
oracle/rng_spec.py's domains 0..4 and league_model.py's domain 5:

  population (domain 6): the member of team p that plays env e in episode k: word 0 of block 0 with turn 0, node 0, group 0, player = p, episode k --
                     member = (word * K) >> 32, the multiply-high form of the combat draw.  A team of one draws nothing: member 0.

It also holds the assignments the GPU tests of the grouped forward use (assignment()), so that a CPU test can check what they cover.
"""
import numpy as np

import rng_spec

DOMAIN_POPULATION = 6
S_BAD_MEMBER = 1
MAX_MEMBERS = 16
WINNER_NONE, WINNER_P0, WINNER_P1, WINNER_TIE = -1, 0, 1, 2


def population_word(seed, env_id, episode, player):
    """the 32-bit word of the draw"""
    return rng_spec.philox4x32_10(rng_spec._ctr(DOMAIN_POPULATION, 0, 0, 0, player, episode, env_id), rng_spec._key(seed))[0]


def population_words(seed, env_ids, episodes, player):
    """population_word for arrays of env ids and episodes (numpy, uint64 arithmetic)"""
    k0, k1 = rng_spec._key(seed)
    M = np.uint64(rng_spec.MASK)
    env_ids = np.asarray(env_ids, np.uint64) & M
    episodes = np.broadcast_to(np.asarray(episodes, np.uint64) & M, env_ids.shape)
    ctr0 = rng_spec._ctr(DOMAIN_POPULATION, 0, 0, 0, player, 0, 0)
    c0 = np.full(env_ids.shape, ctr0[0], np.uint64)
    c1 = np.full(env_ids.shape, ctr0[1], np.uint64)
    c2, c3 = episodes.copy(), env_ids.copy()
    for r in range(10):
        if r:
            k0 = (k0 + rng_spec.W0) & rng_spec.MASK
            k1 = (k1 + rng_spec.W1) & rng_spec.MASK
        p0 = np.uint64(rng_spec.M0) * c0
        p1 = np.uint64(rng_spec.M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & M, p0 & M
    return c0.astype(np.uint32)


def choose(word, K):
    """random.choice(range(K)) from the draw's word: (word * K) >> 32; a team of one draws nothing"""
    return 0 if K <= 1 else (int(word) * int(K)) >> 32


def members(seed, env_ids, episodes, player, K):
    """choose() for arrays -> uint8"""
    env_ids = np.asarray(env_ids)
    if K <= 1:
        return np.zeros(env_ids.shape, np.uint8)
    return ((population_words(seed, env_ids, episodes, player).astype(np.uint64) * np.uint64(K)) >> np.uint64(32)).astype(np.uint8)


class Population(object):
    """assignment and counters of N envs"""

    def __init__(self, seed, env_id_base, N, K):
        self.seed, self.base, self.N, self.K = seed, env_id_base, N, tuple(K)
        self.member = np.zeros((N, 2), np.uint8)
        self.counts = np.zeros((2, MAX_MEMBERS, 4), np.int64)
        self.status = 0

    def _draw(self, envs, episodes):
        ids = self.base + envs
        for p in range(2):
            self.member[envs, p] = members(self.seed, ids, np.asarray(episodes)[envs], p, self.K[p])

    def clear(self, episodes):
        """episodes: the envs' current episode indices [N]"""
        self.counts[:] = 0
        self.status = 0
        self._draw(np.arange(self.N), episodes)

    def assign(self, mask, winner, episodes):
        """evg_population_assign: -> the members that played (a copy of member as it stood); tally where winner is given; draw for `episodes`"""
        envs = np.arange(self.N) if mask is None else np.nonzero(np.asarray(mask))[0]
        history = self.member.copy()
        if winner is not None:
            for e in envs:
                w = int(winner[e])
                if w not in (WINNER_P0, WINNER_P1, WINNER_TIE):
                    continue
                for p in range(2):
                    m = int(self.member[e, p])
                    if m >= self.K[p]:
                        self.status |= S_BAD_MEMBER
                        continue
                    self.counts[p, m, 0] += 1
                    self.counts[p, m, 1 if w == p else (2 if w == WINNER_TIE else 3)] += 1
        self._draw(envs, episodes)
        return history


# ---- the assignments of the grouped forward's GPU tests: uint8 [N, 2] for teams of K = (K0, K1)
ASSIGNMENTS = ("one", "empty", "boundary", "alternating")


def assignment(kind, N, K):
    a = np.zeros((N, 2), np.uint8)
    e = np.arange(N)
    for p in range(2):
        k = K[p]
        if kind == "one":                    # every env on one member: the last of the team
            a[:, p] = k - 1
        elif kind == "empty":                # member 0 has no env where the team has another
            a[:, p] = 0 if k == 1 else 1 + e % (k - 1)
        elif kind == "boundary":             # a member with exactly 16 envs and one with exactly 17 (the wavefront's group of 16), where there is room
            if k >= 3 and N >= 33:
                a[:, p] = np.where(e < 16, 0, np.where(e < 33, 1, 2 + e % (k - 2)))
            elif k == 2 and N >= 33:         # member 1: exactly 17; member 0 the rest (exactly 16 of 33)
                a[:, p] = np.where(e < 17, 1, 0)
            else:
                a[:, p] = e % k
        elif kind == "alternating":          # neighbours never share a member: no wavefront's 16 rows are contiguous
            a[:, p] = (e + p) % k
        else:
            raise ValueError(kind)
    return a
