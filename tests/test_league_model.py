"""CPU tests of the opponent league's host model (tests/league_model.py): its choice is Python's own random.choices, its weights the cycled training
script's updateAgentWeights."""
import itertools
import random

import numpy as np

import league_model as lm


class _Fixed(random.Random):
    """a generator whose random() is the model's u"""

    def __init__(self, u):
        super().__init__(0)
        self.u = u

    def random(self):
        return self.u


def _update_agent_weights(opposing_agents):
    """dqn_smart_state_cycled_training_with_importance.py:166-173, restated"""
    opposing_agent_weights = []
    for opposing_agent in opposing_agents:
        if opposing_agent["games"] == 0:
            opposing_agent_weights.append(1.0)
        else:
            opposing_agent_weights.append(1.0 - opposing_agent["wins"] / opposing_agent["games"] + 0.05)
    return opposing_agent_weights


def _weight_sets():
    rs = np.random.RandomState(5)
    sets = []
    for M in (1, 2, 3, 15, 16):
        sets.append([1.0] * M)
        sets.append([0.25 * (j + 1) for j in range(M)])                  # dyadic: x can land exactly on a boundary
        for _ in range(6):
            sets.append(rs.random_sample(M).tolist())
        for _ in range(6):                                              # the shape updateAgentWeights produces
            games = rs.randint(0, 60, M)
            wins = (games * rs.random_sample(M)).astype(int)
            sets.append(_update_agent_weights([dict(games=int(g), wins=int(w)) for g, w in zip(games, wins)]))
        if M >= 2:
            z = rs.random_sample(M) + 0.1
            for zero in ([0], [M - 1], [M // 2], list(range(M - 1)), list(range(1, M))) + (([0, M - 1],) if M > 2 else ()):
                w = z.copy()
                w[zero] = 0.0
                sets.append(w.tolist())
    return sets


def test_the_models_choice_is_pythons_random_choices():
    rs = np.random.RandomState(11)
    largest = (2 ** 32 - 1) / 4294967296.0
    cases = 0
    for w in _weight_sets():
        M = len(w)
        cum = list(itertools.accumulate(w))
        total = cum[-1] + 0.0
        us = [0.0, largest, 0.5] + (rs.randint(0, 2 ** 32, 120, dtype=np.uint64) / 4294967296.0).tolist()
        # x exactly on a cumulative boundary, where the division is exact and the quotient is a 32-bit fraction
        for c in (cum[:-1] if total > 0.0 else []):
            u = c / total
            if u < 1.0 and u * 4294967296.0 == int(u * 4294967296.0) and u * total == c:
                us.append(u)
        for u in us:
            want = _Fixed(u).choices(range(M), w)[0]
            assert lm.choose(u, w) == want, (u, w)
            cases += 1
    assert cases >= 10000, cases
    # boundaries were really hit
    assert lm.choose(0.25, [1.0, 1.0, 1.0, 1.0]) == 1 == _Fixed(0.25).choices(range(4), [1.0] * 4)[0]
    # where the reference raises, the model says so
    for w in ([0.0, 0.0], [float("inf"), 1.0], [float("nan"), 1.0], [-1.0, 0.5]):
        assert lm.choose(0.3, w) is None
        try:
            _Fixed(0.3).choices(range(len(w)), w)
        except ValueError:
            pass
        else:
            raise AssertionError(w)
    # the draw itself: a keyed word, distinct per env, episode and seat
    words = {lm.league_word(9, e, k, p) for e in range(8) for k in range(8) for p in range(2)}
    assert len(words) == 128


def test_the_models_weights_are_update_agent_weights():
    rs = np.random.RandomState(3)
    for M in (1, 4, 15, 16):
        for _ in range(50):
            games = rs.randint(0, 200, M)
            games[rs.randint(0, M)] = 0
            wins = (games * rs.random_sample(M)).astype(np.int64)
            wins[rs.randint(0, M)] = games[rs.randint(0, M)] * 0 + wins[0]
            k = rs.randint(0, M)
            wins[k] = games[k]                                           # wins == games
            wins = np.minimum(wins, games)
            counts = np.zeros((M, 4), np.int64)
            counts[:, 0], counts[:, 1] = games, wins
            want = _update_agent_weights([dict(games=int(g), wins=int(w)) for g, w in zip(games, wins)])
            got = lm.importance(counts)
            assert got.tolist() == want
            assert all(got[m] == 1.0 for m in range(M) if games[m] == 0)
            assert got[k] == (1.0 if games[k] == 0 else 1.0 - 1.0 + 0.05)
