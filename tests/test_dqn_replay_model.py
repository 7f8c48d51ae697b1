"""CPU tests (no GPU needed) of the host model of the agents/DQN family's replay memory (tests/dqn_replay_model.py): against the reference's own
remember_game_state / ReplayMemory / reward_short_games on a recorded game's end (tests/golden/dqn_replay.npz, tools/gen_dqn_replay_golden.py), and the
uniformity of its draw.  The GPU tests then compare the device with the model bit for bit."""
import os

import numpy as np

from conftest import ROOT, load_golden
import dqn_replay_model as dm


def play(fx, H, auto_reset, rows=None):
    """the fixture's turns through the model, one env; the ring of observations as the step would have written it"""
    T = len(fx["turn"])
    m = dm.DqnReplayModel(1, H, shaping="reward_short_games", seat=0, auto_reset=auto_reset, turn0=[fx["turn"][0]])
    ring = np.zeros((m.slots, 1, 105), np.int16)
    ring[0, 0] = fx["obs"][0]
    for t in range(T):
        ring[(t + 1) % m.slots, 0] = fx["obs"][t + 1]
        m.record((fx["rows"] if rows is None else rows)[t][None], fx["reward"][t][None], fx["done"][t][None])
    return m, ring


def test_model_equals_the_reference_memory_in_push_order():
    fx = load_golden("dqn_replay.npz")
    T = len(fx["turn"])
    assert fx["done"][-1] == 1 and not fx["done"][:-1].any()
    for auto_reset in (True, False):
        m, ring = play(fx, T, auto_reset)
        assert m.size() == T and m.status == 0
        r = m.push_order()
        handles = np.stack([r["slot"], r["env"], 0 * r["slot"], 0 * r["slot"]], 1)
        state, action, nxt, reward, nd = m.gather(handles, ring)
        assert np.array_equal(action, fx["ref_action"].astype(np.int64)) and action.dtype == np.int64
        assert np.array_equal(r["reward"], fx["ref_reward"])                                        # float64, bit for bit
        assert np.array_equal(reward, fx["ref_reward"].astype(np.float32))                          # rounded once
        assert np.array_equal(state.astype(np.float64), fx["ref_state"])
        assert np.array_equal(nd, fx["done"] == 0)
        assert np.array_equal(nxt[nd].astype(np.float64), fx["ref_next_state"][nd])
        assert not nxt[~nd].any()                                                                   # the documented difference: zeros, not_done = 0
        if not auto_reset:                                                                          # the terminal observation, unmasked
            nxt2 = m.gather(handles, ring, terminal_next=True)[2]
            assert np.array_equal(nxt2.astype(np.float64), fx["ref_next_state"])
        assert m.ctr[0].tolist() == [0, 1, 0, 0 if auto_reset else 1]
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_replay.npz"))
    assert all(z[k].dtype.kind in "fiu" for k in z.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dqn_replay.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "dqn_learn.npz"))


def test_lifetime_frozen_envs_and_action_validity():
    fx = load_golden("dqn_replay.npz")
    T = len(fx["turn"])
    m, _ = play(fx, 3, True)                                                                        # H = 3: records T - 3 .. T - 1 are live
    assert m.size() == 3 and sorted(m.turn_of[m.records()["slot"]].tolist()) == [T - 3, T - 2, T - 1]
    m, _ = play(fx, 3, False)
    for _ in range(2):                                                                              # frozen: records nothing, and the ring empties
        m.record(fx["rows"][0][None], fx["reward"][0][None], [1])
    assert m.size() == 1 and m.ctr[0, 3] == 1
    for col, bad in ((0, 12), (0, -1), (1, 11), (1, -1)):
        rows = fx["rows"].copy()
        rows[T - 2, 4, col] = bad
        m, _ = play(fx, T, True, rows)
        assert m.size() == T - 1 and m.status == dm.S_BAD_ACTION and m.valid[(T - 2) % m.slots, 0] == 0
    assert dm.actions_valid(np.array([[11, 10]] * 7)) and dm.unravel(np.array([[11, 10]])).tolist() == [131]


def test_gather_of_bad_handles_and_the_empty_draw():
    fx = load_golden("dqn_replay.npz")
    m, ring = play(fx, 3, True)
    h = m.handles()
    bad = np.array([[-1, -1, -1, -1], [m.slots, 0, 0, 0], [0, 1, 0, 0], [h[0][0], 0, 1, 0], [h[0][0], 0, 0, 1]], np.int32)
    out = m.gather(bad[:1], ring)
    assert m.status == 0 and not any(np.asarray(o).any() for o in out)                              # all -1: the empty draw's handle, no bit
    out = m.gather(bad, ring)
    assert m.status == dm.S_BAD_HANDLE and not any(np.asarray(o).any() for o in out)
    empty = dm.DqnReplayModel(2, 2)
    assert (empty.draw(1, 0, 5) == -1).all() and empty.status == dm.S_EMPTY


def test_draw_is_uniform_over_the_valid_records():
    """40 valid records among 60, 120 000 model draws over 3 calls and 2 seeds: chi-square with 39 degrees of freedom.  The 0.999 quantile of
    chi2(39) is 72.05; the draws are fixed by the seeds, so the test is deterministic."""
    N, H = 10, 5
    m = dm.DqnReplayModel(N, H)
    rng = np.random.default_rng(7)
    flat = np.zeros(m.slots * N, np.uint8)
    flat[rng.permutation(m.slots * N)[:40]] = 1
    m.valid[:] = flat.reshape(m.slots, N)
    h = m.handles()
    assert len(h) == 40
    index = {(int(k), int(e)): i for i, (k, e, _, _) in enumerate(h)}
    counts = np.zeros(40, np.int64)
    draws = 0
    for seed, call in ((11, 0), (11, 1), (0xDEADBEEF12345678, 1 << 33)):
        d = m.draw(seed, call, 40000)
        assert (d[:, 2:] == 0).all()
        for k, e in d[:, :2]:
            counts[index[(int(k), int(e))]] += 1                                                     # (a hole would raise KeyError)
        draws += len(d)
    assert draws >= 100000
    expected = draws / 40.0
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("chi-square %.2f over %d draws" % (chi2, draws))
    assert chi2 < 72.05
    # the t-th valid record in (slot, env) order: handles are sorted by slot, then env
    assert np.array_equal(h[:, :2], np.array(sorted(map(tuple, h[:, :2].tolist())), np.int32))


# ---------------------------------------------------------------------- sampling by priority
import dqn_replay_priority_model as pm     # noqa: E402


def priority_case(fx):
    """the fixture's 40 records as slot 0 of a 40-env memory: the reference's index i is env i"""
    base = dm.DqnReplayModel(40, 1)
    base.valid[0, :] = 1
    model = pm.DqnPriorityModel(base, float(fx["prio_alpha"]))
    model.update(base.handles(), fx["prio"])
    return base, model


def test_priority_model_against_the_references_prioritized_memory():
    """the stored weight p ** alpha within 2 float32 ulps of the reference's prios ** prob_alpha, and PrioritizedMemory.sample's importance weights for
    its own indices within rtol 1e-6 (the bounds tests/test_gpu_replay_priority.py uses for these expressions)"""
    fx = load_golden("dqn_replay.npz")
    base, model = priority_case(fx)
    assert model.status == 0 and model.wmax == model.weights.max()
    w, ref = model.weights[0], fx["prio_pow"]
    ulps = np.abs(w.astype(np.float64) - ref.astype(np.float64)) / np.spacing(ref).astype(np.float64)
    print("stored weights: %.2f ulps at most" % ulps.max())
    assert ulps.max() <= 2
    got = model.importance(fx["prio_indices"], float(fx["prio_beta"]))
    dev = np.abs(got / fx["prio_weights"].astype(np.float64) - 1).max()
    print("importance weights: relative deviation %.3g" % dev)
    assert dev <= 1e-6
    assert (model.importance(fx["prio_indices"], 0.0) == 1.0).all()


def test_priority_update_rules_and_the_draw():
    fx = load_golden("dqn_replay.npz")
    base, model = priority_case(fx)
    h = base.handles()
    # duplicates in one update keep the largest, in any order
    model.update(h[[6]], np.array([9.0], np.float32))
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        model.update(h[[5, 5, 5]], np.array([0.5, 7.0, 2.0], np.float32)[order])
        assert model.weights[0, 5] == pm.weight(np.float32(7.0), model.alpha)
    model.update(h[[5]], np.array([0.25], np.float32))                          # a later update replaces it, smaller or not
    assert model.weights[0, 5] == pm.weight(np.float32(0.25), model.alpha) and model.wmax == pm.weight(np.float32(9.0), model.alpha)
    # bad priorities and handles are skipped
    before = model.weights.copy()
    model.update(h[:4], np.array([np.nan, np.inf, 0.0, -1.0], np.float32))
    assert model.status == pm.S_BAD_PRIORITY and np.array_equal(model.weights, before)
    model.update(np.array([[1, 0, 0, 0], [0, 40, 0, 0], [0, 0, 1, 0]]), np.ones(3, np.float32))
    assert model.status == pm.S_BAD_PRIORITY | pm.S_BAD_HANDLE and np.array_equal(model.weights, before)
    # a stale stamp means never updated: the record weighs wmax
    base.meta[0, 7, 0] += 1
    assert model.effective()[7] == model.wmax
    base.meta[0, 7, 0] -= 1
    # the draw follows the probabilities q / Q
    handles, idx = model.draw(3, 0, 40000)
    assert np.array_equal(handles, h[idx])
    counts = np.bincount(idx, minlength=40)
    expected = model.probabilities() * len(idx)
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print("chi-square %.2f" % chi2)
    assert chi2 < 72.05                                                        # the 0.999 quantile of chi2(39)
