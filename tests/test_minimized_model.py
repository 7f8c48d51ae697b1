"""CPU tests (no GPU needed) of the Minimized agents' host model (tests/minimized_model.py) against the reference's own DQNAgent methods, recorded in
tests/golden/minimized_actions.npz (tools/gen_minimized_golden.py), and of the decode rules the fixtures cannot hold: NaN, +-inf and all-equal rows."""
import numpy as np
import pytest

from conftest import load_golden
import minimized_model as mm


@pytest.fixture(scope="module")
def gold():
    return load_golden("minimized_actions.npz")


def test_best_actions_equal_the_reference(gold):
    q, best = gold["q"], gold["best"]
    ties = 0
    for m in range(q.shape[0]):
        for p in range(2):
            assert np.array_equal(mm.best_actions(q[m, p]), best[m, p]), (m, p)
            ties += len(set(q[m, p].max(axis=1).tolist())) < 12
    assert ties > 50                        # the fixture does exercise the stable order of equal keys
    assert best[..., 1].min() >= 1 and best[..., 1].max() <= 11


def test_get_action_equals_the_reference_at_six_epsilon_levels(gold):
    q, eps, seed = gold["q"], gold["eps"], int(gold["seed"][0])
    M = q.shape[0]
    assert sorted(set(eps.ravel().tolist())) == [0.0, np.float32(0.05), np.float32(0.3), 0.5, np.float32(0.95), 1.0]
    for p in range(2):
        rows, explored = mm.get_action(q[:, p], seed, np.arange(M), gold["episode"], gold["obs"][:, p, 0], p, eps[:, p])
        assert np.array_equal(explored, gold["explored"][:, p])
        assert np.array_equal(rows, gold["actions"][:, p])
    x = gold["explored"].astype(bool)
    assert x[eps == 1.0].all() and not x[eps == 0.0].any() and 0 < x.sum() < x.size
    # where the random branch ran: 7 distinct swarms and 7 distinct nodes of 1..11
    for a in gold["actions"][x]:
        assert len(set(a[:, 0])) == 7 and len(set(a[:, 1])) == 7 and a[:, 1].min() >= 1 and a[:, 1].max() <= 11 and a[:, 0].max() <= 11


def test_node_draw_of_one_agent_call_worked_by_hand():
    """(seed 20261018, env 5, episode 2, turn 17, seat 1): block 1's halves are 27445, 29981, 62683, 33894, 44462, 50061, 35450, 4579.  The draw by hand,
    pool 0..10: i = 0: 27445 * 11 >> 16 = 4, j = 4, node 5; i = 1: 29981 * 10 >> 16 = 4, j = 5, node 6; i = 2: 62683 * 9 >> 16 = 8, j = 10, node 11;
    i = 3: 33894 * 8 >> 16 = 4, j = 7, node 8; i = 4: 44462 * 7 >> 16 = 4, j = 8, node 9; i = 5 (pool now 4 5 10 7 8 1 6 3 0 9 2): 50061 * 6 >> 16 = 4,
    j = 9, node 10; i = 6: 35450 * 5 >> 16 = 2, j = 8, node 1.  The coin is half 7 of block 0 (23274) << 16 | half 7 of block 1 (4579)."""
    h1 = mm.rng_spec.halves(mm.rng_spec.philox4x32_10(mm.rng_spec._ctr(4, 1, 17, 0, 1, 2, 5), mm.rng_spec._key(20261018)))
    assert h1 == [27445, 29981, 62683, 33894, 44462, 50061, 35450, 4579]
    coin, swarms, nodes = mm.explore_draws(20261018, 5, 2, 17, 1)
    assert nodes == [5, 6, 11, 8, 9, 10, 1]
    assert coin == (23274 << 16) | 4579 == 1525289443
    assert (coin, swarms) == tuple(mm.rng_spec.explore_draws(20261018, 5, 2, 17, 1)[:2])      # the Smart_State call's coin and swarm draw, unchanged


def test_nan_inf_and_all_equal_rows():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    v = np.zeros(11, np.float32)
    assert mm.swarm_best(v) == (1, 0.0)                                 # all equal: the first
    v[4] = v[9] = 2.0
    assert mm.swarm_best(v) == (5, 2.0)                                 # the FIRST maximum
    v[7] = nan
    node, key = mm.swarm_best(v)
    assert node == 8 and key == inf                                      # a NaN is the maximum; as a key it counts as +inf
    v[2] = nan
    assert mm.swarm_best(v)[0] == 3                                      # the first NaN
    v[:] = -inf
    assert mm.swarm_best(v) == (1, -inf)
    v[10] = inf
    assert mm.swarm_best(v) == (11, inf)
    # rows: a NaN swarm and a +inf swarm tie as keys and keep swarm order, behind every finite swarm; -inf comes first
    q = np.tile(np.arange(11, dtype=np.float32), (12, 1))               # every swarm: best 10 at node 11
    q[3, 0] = nan
    q[1, 5] = inf
    q[8] = -inf
    q[6] = 10.0                                                          # all equal at the common key: node 1
    rows = mm.best_actions(q)
    assert rows.tolist() == [[8, 1], [0, 11], [2, 11], [4, 11], [5, 11], [6, 1], [7, 11]]
    q[[0, 2, 4, 5, 7, 9]] = inf                                          # six +inf swarms around the NaN one and the inf-at-5 one
    assert mm.best_actions(q).tolist() == [[8, 1], [6, 1], [10, 11], [11, 11], [0, 1], [1, 6], [2, 1]]
    q[:] = 0.5
    assert mm.best_actions(q).tolist() == [[s, 1] for s in range(7)]
