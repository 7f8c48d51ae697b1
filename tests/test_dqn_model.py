"""CPU tests (no GPU needed) of the agents/DQN family's host model (tests/dqn_model.py: the contracts of include/evg_dqn.h restated) against the
reference's own methods recorded in tests/golden/dqn_agent.npz (tools/gen_dqn_golden.py): QNetwork.forward, DQNAgent.filter_actions and
DQNAgent.get_action / epsilon_greedy."""
import numpy as np
import pytest

from conftest import load_golden
import dqn_model as dm
from qnet_model import fmaf32

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


def _params(d):
    return d["a_w1"], d["a_b1"], d["a_w2"], d["a_b2"]


def test_filter_actions_equals_the_reference_row_for_row():
    d = load_golden("dqn_agent.npz")
    q, want = d["b_q"], d["b_rows"]
    assert q.shape == (312, 132) and want.shape == (312, 7, 2) and np.isnan(q).any() and np.isinf(q).any()
    got = np.stack([dm.filter_actions(q[m]) for m in range(q.shape[0])])
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert bad.size == 0, (bad[:5], got[bad[:1]], want[bad[:1]])
    # the quirks the rows pin: nodes stay 0..10, an all-zero row is seven {0, 0}, nothing <= 0 and no NaN is taken, equal values keep the first
    assert want[..., 1].min() == 0 and want[..., 1].max() == 10 and want[..., 0].max() == 11
    zero = np.flatnonzero((q == 0).all(axis=1))
    negative = np.flatnonzero((q < 0).all(axis=1))
    assert zero.size >= 4 and negative.size >= 8 and not want[zero].any() and not want[negative].any()
    assert np.array_equal(want[3], np.stack([np.arange(7), np.zeros(7, int)], axis=1))          # everything ties at 0.5: groups 0..6 at node 0
    assert np.array_equal(dm.filter_actions(np.full(132, np.nan, np.float32)), np.zeros((7, 2), np.int32))


def test_get_action_equals_the_reference_rows_and_explored_flags():
    d = load_golden("dqn_agent.npz")
    M = d["c_eps"].shape[0]
    q, seed, ids = d["b_q"][:M], int(d["c_seed"][0]), np.arange(M)
    for p in range(2):
        rows, explored = dm.get_action(q, seed, ids, d["c_episode"], d["c_turn"], p, d["c_eps"][:, p])
        assert np.array_equal(explored, d["c_explored"][:, p]) and np.array_equal(rows, d["c_rows"][:, p]), p
    x = d["c_explored"]
    assert 0 < x.sum() < x.size and x[d["c_eps"] == 1.0].all() and d["c_rows"][x == 1][..., 1].min() == 0
    # `sample > eps` is the greedy branch: row 0's epsilon IS its coin and explores; row 1's is the float32 below its coin and does not
    for m, flag in ((0, 1), (1, 0)):
        coin = dm.explore_draws(seed, m, int(d["c_episode"][m]), int(d["c_turn"][m]), 0)[0] / 4294967296.0
        eps = float(d["c_eps"][m, 0])
        assert (eps == coin if flag else eps < coin and float(np.nextafter(np.float32(eps), np.float32(1))) == coin) and x[m, 0] == flag
    # the draws are the Minimized agents' with the node one lower (a seat runs one family per turn)
    import minimized_model as mm
    a, b = dm.explore_draws(seed, 5, 1, 17, 1), mm.explore_draws(seed, 5, 1, 17, 1)
    assert a[:2] == b[:2] and a[2] == [n - 1 for n in b[2]] and len(set(a[1])) == 7 and len(set(a[2])) == 7 and max(a[2]) <= 10


def test_chain_and_reference_forward_lie_within_the_counted_bound_of_float64():
    """Both fp32 evaluations -- the model's fmaf chain and torch's GEMM recorded in the fixture -- lie within E2 (dqn_model.error_bound: counted from the
    number of roundings, not tuned) of the float64 value, hence within 2 E2 of each other."""
    d = load_golden("dqn_agent.npz")
    params, x, ref = _params(d), d["a_x"], d["a_q"].astype(np.float64)
    assert d["a_w1"].shape == (48, 105) and d["a_w2"].shape == (132, 48) and x.shape == (64, 105)
    q32 = dm.forward(x, params, True).astype(np.float64)
    q64 = dm.forward_f64(x, params, True)
    e2 = dm.error_bound(x, params)
    print("chain - f64: %.3e, torch - f64: %.3e, chain - torch: %.3e; E2 from %.3e to %.3e; |q| up to %.3g" % (
        np.abs(q32 - q64).max(), np.abs(ref - q64).max(), np.abs(q32 - ref).max(), e2.min(), e2.max(), np.abs(q64).max()))
    assert (e2 > 0).all() and e2.max() < 1e-2
    assert (np.abs(q32 - q64) <= e2).all() and (np.abs(ref - q64) <= e2).all() and (np.abs(q32 - ref) <= 2 * e2).all()
    assert (ref >= 0).all() and 0.2 < (ref > 0).mean() < 0.8            # the reference applies the final ReLU, and it clips some and not all
    # the bound sees a dropped term: the chain without x[104] is outside it somewhere
    cut = x.copy()
    cut[:, 104] = 0
    assert (np.abs(dm.forward(cut, params, True).astype(np.float64) - q64) > e2).any()


def _chain(x, params, final_relu):
    """the contract spelled out scalar by scalar, for one row"""
    w1, b1, w2, b2 = params
    h = []
    for j in range(w1.shape[0]):
        acc = np.float32(b1[j])
        for k in range(105):
            acc = fmaf32(w1[j, k], x[k], acc)
        h.append(np.float32(0) if acc < 0 else np.float32(acc))
    q = []
    for o in range(132):
        acc = np.float32(b2[o])
        for j in range(w1.shape[0]):
            acc = fmaf32(w2[o, j], h[j], acc)
        q.append(np.float32(0) if final_relu and acc < 0 else np.float32(acc))
    return np.array(q, np.float32)


def test_forward_follows_the_chain_at_one_hidden_unit_and_with_planted_specials():
    rng = np.random.RandomState(5)
    for h1 in (1, 3):
        params = [rng.standard_normal(s).astype(np.float32) * 0.3 for s in ((h1, 105), (h1,), (132, h1), (132,))]
        x = rng.standard_normal((4, 105)).astype(np.float32)
        x[1, 7], x[2, 50], x[3, 104] = np.nan, np.inf, np.float32(1e-41)           # a NaN, an Inf and a subnormal in x
        for planted in (None, (0, 0, 3, np.nan), (0, 0, 104, np.inf), (0, 0, 9, np.float32(3e-42)), (2, 5, 0, -np.inf), (1, 0, None, np.nan)):
            p = [t.copy() for t in params]
            if planted is not None:
                t, i, j, v = planted
                if j is None:
                    p[t][i] = v
                else:
                    p[t][i, j] = v
            for fr in (True, False):
                got = dm.forward(x, p, fr)
                for r in range(4):
                    want = _chain(x[r], p, fr)
                    assert np.array_equal(np.isnan(got[r]), np.isnan(want)) and np.array_equal(np.nan_to_num(got[r], nan=7.0), np.nan_to_num(want, nan=7.0))
        q = dm.forward(x, params, True)
        assert np.isnan(q[1]).all()                                            # the NaN goes through the ReLU of both layers
        assert np.isfinite(q[0]).all()
