"""CPU tests (no GPU needed) of tests/learner_edge_cases.py, on the host models alone: the Q-network families reach the values they name (subnormal
hidden units and Q, NaN / Inf / finite Q, damaged rows next to finite ones) and the replay driver reaches the records it names (episodes shorter than n,
both kinds of finalised record, the transition ratio below and at 1, empty scan blocks at both ends and in a row).  The GPU tests of
tests/test_gpu_learner_edges.py rely on this to tell a kernel that is wrong at these edges from one that is right."""
import numpy as np
import pytest

import learner_edge_cases as cases
from qnet_model import expand
from replay_model import F_FINAL, F_NOT_DONE

NETS = [("smart", h) for h in cases.SMART_HIDDEN] + [("mini", h) for h in cases.MINI_HIDDEN]
WIDE = [(k, h) for k, h in NETS if min(h) >= 16]
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")           # numpy's overflow and invalid-value warnings are the subject here


def _q(kind, hidden, family, layout, final_relu=False):
    params, inputs = cases.case(kind, hidden, family, layout)
    return params, inputs, cases.model_q(kind, layout, params, inputs, final_relu)


@pytest.mark.parametrize("kind,hidden", NETS[:1] + NETS[3:4])
def test_signed_inputs_are_negative_in_every_part_and_q_is_finite(kind, hidden):
    x = cases.expanded_inputs("signed")
    shared, swarm = cases.compact_inputs("signed", seats=2)
    assert (x < 0).mean() > 0.4 and (shared < 0).mean() > 0.4 and (swarm < 0).mean() > 0.4
    for layout in cases.LAYOUTS:
        _, _, q = _q(kind, hidden, "signed", layout)
        assert np.isfinite(q).all() and (q < 0).any() and (q > 0).any()


@pytest.mark.parametrize("layout", ["expanded", "compact"])
@pytest.mark.parametrize("kind,hidden", WIDE)
def test_subnormal_family_has_subnormal_hidden_units_and_q(kind, hidden, layout):
    """at least 10 % of the first hidden layer and 10 % of Q are non-zero subnormals, in the expanded rows and behind the compact layouts' one-hot add"""
    params, inputs, q = _q(kind, hidden, "subnormal", layout)
    x = inputs if layout == "expanded" else expand(*inputs).reshape(-1, 59)
    h = cases.first_hidden(params, x)
    assert cases.is_subnormal(h).mean() >= 0.10 and cases.is_subnormal(q).mean() >= 0.10
    assert (h >= np.finfo(np.float32).tiny).any()                         # ... next to normal ones
    if layout == "compact":
        assert cases.is_subnormal(params[0][:, 47:]).mean() > 0.99        # the one-hot term is a subnormal


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden", WIDE)
def test_overflow_family_has_nan_inf_and_finite_q(kind, hidden, layout):
    _, _, q = _q(kind, hidden, "overflow", layout)
    assert np.isnan(q).mean() >= 0.10 and np.isinf(q).mean() >= 0.10 and np.isfinite(q).mean() >= 0.10
    # with the final ReLU on, the NaNs stay: the output layer keeps them
    _, _, qr = _q(kind, hidden, "overflow", layout, True)
    assert np.array_equal(np.isnan(qr), np.isnan(q)) and not (qr < 0).any()
    assert cases.same_values(qr, np.maximum(q, np.float32(0)))            # the final ReLU is the model's np.maximum on top (the GPU tests apply it so)


@pytest.mark.parametrize("kind,hidden", NETS)
def test_non_finite_inputs_damage_their_rows_and_no_other(kind, hidden):
    for family in ("nonfinite", "zero_column"):                           # (absorbed: test_damaged_weights_...)
        _, x, q = _q(kind, hidden, family, "expanded")
        bad = cases.damaged_rows(family, x.shape[0])
        assert 0.2 < bad.mean() < 0.5
        assert np.isfinite(x[~bad]).all() and (~np.isfinite(x[bad])).sum(1).tolist() == [1] * int(bad.sum())
        assert np.isfinite(q[~bad]).all()
        hurt = (~np.isfinite(q[bad])).any(1)
        assert hurt.mean() > 0.5 if min(hidden) >= 16 else hurt.any()     # (the ReLU of a one-unit network clips a -Inf hidden unit to 0)
        if family == "zero_column":
            assert np.isnan(q[bad]).all()                                 # Inf * 0 in every hidden unit
        _, (shared, swarm), q = _q(kind, hidden, family, "compact")
        bad = cases.damaged_rows(family, shared.shape[0])
        in_shared, in_swarm = ~np.isfinite(shared).all(1), ~np.isfinite(swarm).all((1, 2))
        assert in_shared.any() and in_swarm.any() and np.array_equal(in_shared | in_swarm, bad)
        assert np.isfinite(q[~bad]).all()
        hit = ~np.isfinite(swarm).all(2)                                  # [N, 12]: a damaged swarm feature reaches its own swarm's Q alone
        assert np.isfinite(q[in_swarm & ~in_shared][~hit[in_swarm & ~in_shared]]).all()
        _, (shared, swarm), q = _q(kind, hidden, family, "seats")
        ok = np.isfinite(shared).all(2) & np.isfinite(swarm).all((2, 3))  # [N, 2]
        assert (~ok[:, 1]).any() and np.isfinite(q[ok]).all()
        if family == "nonfinite":
            assert (~ok[:, 0]).any() and not (~ok).all(1).any()           # both seats are damaged somewhere, never both in one env
        else:
            assert ok[:, 0].all()


@pytest.mark.parametrize("family", cases.WEIGHT_DAMAGE)
@pytest.mark.parametrize("kind,hidden", NETS)
def test_damaged_weights_reach_q_and_seat_0_stays_finite(kind, hidden, family):
    params, x, q = _q(kind, hidden, family, "expanded")
    clean = cases.net_params(kind, hidden, family, damaged=False)
    assert sum(int((~np.isfinite(a)).sum()) for a in params) == (0 if family in cases.INF_COLUMNS else 1)
    assert family != "absorbed" or (params[0][:, list(cases.POSITIVE_COLUMNS)] > 0).all()
    assert (params[0][:, list(cases.ZERO_COLUMNS)] == 0).all() == (family == "zero_column")
    assert all(np.isfinite(a).all() and (a != 0).all() for a in clean)
    if family == "nan_weight":
        # Smart: unit 3 of the second hidden layer is NaN in every row, so every Q is; Minimized: the weight sits in the output layer, so Q[:, 3] is
        assert np.isnan(q).all() if kind == "smart" else (np.isnan(q[:, 3]).all() and np.isfinite(np.delete(q, 3, 1)).all())
    elif family == "inf_bias":
        assert (~np.isfinite(q)).any(1).all()
    elif family == "zero_column":
        bad = cases.damaged_rows(family, x.shape[0])
        assert np.isnan(q[bad]).all() and np.isfinite(q[~bad]).all()
    else:
        # absorbed: the damaged rows' hidden layer is all zeros behind the ReLU, their Q finite and one and the same; undamaged weights would give NaN
        bad = cases.damaged_rows(family, x.shape[0])
        assert 0.2 < bad.mean() < 0.5 and np.isneginf(x[bad]).sum(1).tolist() == [1] * int(bad.sum())
        assert (cases.first_hidden(params, x[bad]) == 0).all() and np.isfinite(q).all() and (q[bad] == q[bad][0]).all()
        if min(hidden) >= 16:
            assert not np.isfinite(cases.model_q(kind, "expanded", clean, x, False)[bad]).any()
        for layout in ("compact", "seats"):
            assert np.isfinite(_q(kind, hidden, family, layout)[2]).all()
    _, _, qs = _q(kind, hidden, family, "seats")
    assert np.isfinite(qs[:, 0]).all()
    if family != "absorbed" and (min(hidden) >= 16 or family != "inf_bias"):                         # (Inf times one negative weight, then the ReLU: a one-unit network's Q is finite)
        assert (~np.isfinite(qs[:, 1])).any()


def test_sweep_shape():
    for cus in (256, 304, 8):
        rows = cases.sweep_rows(cus)
        groups = (rows + 15) // 16
        assert groups == 4 * 2 * cus + 2 and rows % 16 == 1                # one full group and a 1-row group past the first sweep
        pick = cases.sweep_checked_rows(rows, cus)
        assert {0, 15, 128 * cus - 1, 128 * cus, rows - 1} <= set(pick.tolist()) and 1024 <= len(pick) <= 16 + 96 + 33 + 1024


# ------------------------------------------------------------------------------------------------------------------ replay memory
def _final_records(case):
    """the flags of the finalised records in the ring after every turn, their number and how many of them hold no transition; the model at the end"""
    seen = dict(flags=set(), no_transitions=0, records=0, episodes=set())

    def on_turn(t, m):
        fl = m.meta[..., 2]
        final = fl != 0
        seen["flags"] |= set(np.unique(fl[final]).tolist())
        seen["records"] += int(final.sum())
        seen["episodes"] |= set(np.unique(m.meta[..., 1][final]).tolist())
        seen["no_transitions"] += int((final & (m.count == 0)).sum())
    m = case.run_model(on_turn=on_turn)
    return seen, m


@pytest.mark.parametrize("case", cases.REPLAY_GRID + cases.REPLAY_FROZEN, ids=repr)
def test_replay_cases_reach_short_episodes_and_both_kinds_of_record(case):
    seen, m = _final_records(case)
    assert seen["flags"] == {F_FINAL, F_FINAL | F_NOT_DONE}
    assert 0 < seen["no_transitions"] < seen["records"]
    # episodes shorter than n: an env whose episode ended with fewer than n records kept
    short, ties = [False], [False]
    lengths = np.zeros(case.N, np.int64)
    frozen = np.zeros(case.N, bool)
    for t in range(case.turns):
        dirs, reward, done, custom = case.turn(t)
        live = ~frozen
        lengths[live] += 1
        ended = live & (done != 0)
        short[0] |= bool((lengths[ended] < case.n).any())
        lengths[ended] = 0
        if not case.auto_reset:
            frozen |= ended
        assert dirs.min() == -1 and dirs[..., 0].max() == 12 and dirs[..., 1].max() == 5
        ties[0] |= bool((reward[:, 0] == reward[:, 1]).any())
    assert short[0] and ties[0]
    assert m.turn == case.turns and case.turns == 3 * (case.H + 1) + 5
    if not case.auto_reset:
        assert (m.ctr[:, 3] == 1).all() and frozen.all()                  # every env is frozen by the last turn ...
        for t in case.checks:                                              # ... and at the checks frozen envs sit next to playing ones
            assert set(case.run_model(upto=t + 1).ctr[:, 3].tolist()) == {0, 1}
    else:
        assert case.checks[0] < case.H + 1 <= case.checks[1] and case.checks[2] >= 2 * (case.H + 1)     # the last check: after two wraps
        if not isinstance(case.shaping, str):
            K = case.shaping[3]                                            # ratio = min(1, (1 + episode) / K): below 1 and clipped at 1
            assert any(1 + ep < K for ep in seen["episodes"]) and any(1 + ep > K for ep in seen["episodes"])
    assert case.checks[2] >= 2 * (case.H + 1)
    for t in case.checks:
        assert case.run_model(upto=t + 1).size() > 0


def test_replay_grid_covers_the_configuration_space():
    grid = cases.REPLAY_GRID
    assert len(grid) == 24 and len({c.name for c in grid}) == 24
    assert {(c.H, c.n, c.gamma) for c in grid} == {(7, 6, 1.0), (5, 3, 0.0), (9, 4, 0.999)}
    assert {c.S for c in grid} == {1, 2} and {c.seat for c in grid if c.S == 1} == {1} and all(c.N == 37 for c in grid)
    assert any(c.n == c.H - 1 for c in grid)
    assert all(c.n == 4 and not c.auto_reset for c in cases.REPLAY_FROZEN)


def test_big_ring_has_empty_blocks_at_both_ends_and_in_a_row():
    case = cases.REPLAY_BIG
    R = (case.H + 1) * case.N * case.S
    nb = (R + cases.SCAN_BLOCK - 1) // cases.SCAN_BLOCK
    assert R == 278834 and nb == 273 and (nb + 255) // 256 == 2 and R % 4 == 2 and R % cases.SCAN_BLOCK != 0
    at = {}
    case.run_model(on_turn=lambda t, m: at.__setitem__(t, (cases.empty_blocks(m), m.size(), m.count[0].any())) if t in case.checks else None)
    assert sorted(at) == sorted(case.checks)
    for t, (empty, size, slot0) in at.items():
        assert size > 4099 and not empty.all()
        assert empty[-1] and cases.longest_run(empty) >= 3
    empty, size, slot0 = at[16]
    assert not slot0 and empty[:16].all() and not empty[16:32].all()      # slot 0 has just been emptied: the first block and 15 more
    inner = at[28][0]
    plane = case.N * case.S
    # inside a written slot: the quiet envs give a run of whole empty blocks between two blocks that are not
    k = 3 * plane // cases.SCAN_BLOCK
    run = inner[k:k + plane // cases.SCAN_BLOCK]
    assert 3 <= cases.longest_run(run) < len(run)
