"""CPU tests (no GPU needed) of the host model of the agents/DQN network's backward pass (tests/dqn_grad_model.py), of the families the GPU tests run
(tests/dqn_grad_cases.py) and of the reference fixture (tests/golden/dqn_grad.npz)."""
import os

import numpy as np
import pytest

from conftest import ROOT
import dqn_grad_cases as cases
import dqn_grad_model as model

NAMES = ("w1", "b1", "w2", "b2")
RANDOM = [(h1, f) for h1 in cases.RANDOM_HIDDEN for f in cases.RANDOM_FAMILIES]


# ---------------------------------------------------------------------- 1. the model against torch.autograd in float64
def _torch_grads(x, params, final_relu, gq):
    """torch.autograd in float64 over the model's own activations and masks: the hidden layer's value is the chain's a1 (so that the outer products
    and the masks are the contract's), its derivative the mask's"""
    import torch
    (_, a1), q = model.chain(x, params, final_relu)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float64))
    ps = [t(p).requires_grad_() for p in params]
    z = t(x) @ ps[0].T + ps[1]
    a = t(a1)
    m = (a > 0).double()
    h = z * m + (a - z * m).detach()
    z = h @ ps[2].T + ps[3]
    out = z * t(q > 0) if final_relu else z
    out.backward(t(gq))
    return [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("h1,family", RANDOM)
def test_model_agrees_with_torch_autograd_in_float64(h1, family, final_relu):
    params, x, gq = cases.case(h1, family, cases.RANDOM_ROWS)
    grads, bounds = model.backward(x, params, final_relu, gq)
    want = _torch_grads(x, params, final_relu, gq)
    c2, c1 = model.roundings(x.shape[0])
    for i, (g, e, w) in enumerate(zip(grads, bounds, want)):
        M = e / ((c1 if i < 2 else c2) * model.U)                       # the sums over absolute values
        assert g.shape == w.shape == tuple(params[i].shape)
        assert (np.abs(g - w) <= 1e-12 * M).all(), (NAMES[i], float(np.abs(g - w).max()))
        assert np.abs(g).max() > 0


def test_the_count_of_roundings_is_the_headers():
    assert model.roundings(64) == (64, 64 + 132) and model.roundings(65536) == (65536, 65536 + 132)
    params, x, gq = cases.case(48, "dense", 17)
    _, bounds = model.backward(x, params, False, gq)
    (_, a1), _ = model.chain(x, params, False)
    assert np.allclose(bounds[3], 17 * model.U * np.abs(gq).sum(0), rtol=1e-12)
    assert np.allclose(bounds[2], 17 * model.U * np.abs(gq.astype(np.float64)).T @ np.abs(a1.astype(np.float64)), rtol=1e-12)
    d1 = (np.abs(gq.astype(np.float64)) @ np.abs(params[2].astype(np.float64))) * (a1 > 0)
    assert np.allclose(bounds[1], (17 + 132) * model.U * d1.sum(0), rtol=1e-12)


# ---------------------------------------------------------------------- 2. the bound can see a dropped row
@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("h1,family", RANDOM)
def test_the_bound_sees_one_dropped_row(h1, family, final_relu):
    """Leaving one row's contribution out moves some gradient element by more than that element's E, whichever row (of 9 spread over the batch) it
    is whose upstream gradient reaches a parameter at all: a skipped row cannot hide inside the tolerance."""
    params, x, gq = cases.case(h1, family, cases.RANDOM_ROWS)
    grads, bounds = model.backward(x, params, final_relu, gq)
    seen = 0
    for row in range(0, cases.RANDOM_ROWS, 31):
        dropped, _ = model.backward(x, params, final_relu, gq, drop_row=row)
        moved = max(float((np.abs(d - g) - e).max()) for d, g, e in zip(dropped, grads, bounds))
        reaches = any((d != g).any() for d, g in zip(dropped, grads))
        assert moved > 0 or not reaches, (row, moved)
        seen += reaches
    assert seen >= 1


# ---------------------------------------------------------------------- 3. the exact tier is exact at the sizes the device runs it
@pytest.mark.parametrize("family", cases.EXACT_FAMILIES)
@pytest.mark.parametrize("h1", cases.HIDDEN)
def test_exact_tier_families_pass_the_models_exact_mode(h1, family):
    some = False
    for final_relu in ([False, True] if h1 in cases.BOTH_RELU_HIDDEN else [False]):
        for rows in cases.ROWS:
            params, x, gq = cases.case(h1, family, rows)
            grads, _ = model.backward(x, params, final_relu, gq, exact=True)
            if family == "pow2dup":                                   # B equal rows: B times the one-row gradient
                one, _ = model.backward(x[:1], params, final_relu, gq[:1], exact=True)
                assert all(np.array_equal(g, rows * o) for g, o in zip(grads, one))
        some = some or all(np.abs(g).max() > 0 for g in grads)
        if family == "integer":
            assert all((g == np.rint(g)).all() for g in grads) and max(np.abs(g).max() for g in grads) > 4
    assert some or (h1 == 1 and family == "pow2dup")                  # (the one unit of that case is dead in its one row: gb2 alone is non-zero)


def test_the_integer_family_is_exact_at_the_large_cases():
    import everglades_amd
    _lib = everglades_amd._lib
    rows = cases.sweep_rows(_lib.DQN_GRAD_MAX_BLOCKS)
    assert rows == 32787 and rows <= _lib.DQN_GRAD_MAX_ROWS and _lib.DQN_GRAD_MAX_BLOCKS * 64 > _lib.DQN_GRAD_TINY_ROWS
    for h1, n in ((cases.SWEEP_HIDDEN, rows), (528, _lib.DQN_GRAD_TINY_ROWS + 64 + 5), (96, _lib.DQN_GRAD_MAX_ROWS)):
        params, x, gq = cases.case(h1, "integer", n)
        for final_relu in (False, True):
            grads, _ = model.backward(x, params, final_relu, gq, exact=True)
            assert max(np.abs(g).max() for g in grads) > 1000


def test_exact_mode_refuses_what_may_round():
    for family in cases.RANDOM_FAMILIES:
        params, x, gq = cases.case(48, family, 17)
        with pytest.raises(AssertionError):
            model.backward(x, params, False, gq, exact=True)
    params, x, gq = cases.case(48, "integer", 17)                     # integers, but one row sum of 2^24 + 1
    gq[:, 0] = 0
    gq[0, 0], gq[1, 0] = 2.0 ** 24, 1.0
    with pytest.raises(AssertionError):
        model.backward(x, params, False, gq, exact=True)


# ---------------------------------------------------------------------- 4. both sides of every mask are exercised
@pytest.mark.parametrize("h1,family", RANDOM)
def test_random_families_exercise_both_sides_of_the_masks(h1, family):
    """Between 20 % and 80 % of the (row, hidden unit) pairs are active, and hidden unit 0 is dead in every row."""
    params, x, gq = cases.case(h1, family, cases.RANDOM_ROWS)
    (_, a1), q = model.chain(x, params, True)
    active = a1 > 0
    assert 0.2 <= active.mean() <= 0.8, active.mean()
    assert cases.has_dead_unit(h1) and not active[:, cases.DEAD_UNIT].any()
    assert 0.1 <= (q > 0).mean() <= 0.9
    if family == "gathered7":                                         # seven entries per row, repeated columns added: some rows have fewer columns
        nz = (gq != 0).sum(1)
        assert nz.max() == 7 and nz.min() < 7


# ---------------------------------------------------------------------- 5. the reference's own optimize_model step
def test_the_fixture_lies_within_twice_the_bound_of_the_model():
    """tests/golden/dqn_grad.npz (tools/gen_dqn_grad_golden.py): torch's CPU gradients of the reference's optimize_model and the model's are sums of
    the same terms -- the fixture's rows keep every pre-activation clear of zero, so its masks are the exact chain's --, torch's in fp32 in its own
    order: within E of the float64 value, plus what the roundings of its own gq (3 per entry) can move; 2 E covers both."""
    import dqn_model
    fx = np.load(os.path.join(ROOT, "tests", "golden", "dqn_grad.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dqn_grad.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "dqn_agent.npz"))
    params = tuple(fx[n] for n in NAMES)
    x, action, expected = fx["x"], fx["action"], fx["expected"].astype(np.float64)
    rows = x.shape[0]
    assert rows == 64 and params[0].shape == (48, 105) and action.shape == (64, 7) and 0 <= action.min() and action.max() < 132
    # the fixture's masks are the exact chain's: every pre-activation is further than 4 x the first-order bound from zero
    w1, b1, w2, b2 = (p.astype(np.float64) for p in params)
    z1 = x.astype(np.float64) @ w1.T + b1
    e1 = 106 * dqn_model.U * (np.abs(b1) + np.abs(x.astype(np.float64)) @ np.abs(w1).T)
    z2 = np.maximum(z1, 0) @ w2.T + b2
    assert (np.abs(z1) > 4 * e1).all() and (np.abs(z2) > 4 * dqn_model.error_bound(x, params)).all()
    q = dqn_model.forward(x, params, True)
    assert np.array_equal(q > 0, fx["q"] > 0) and np.allclose(q, fx["q"], rtol=1e-4, atol=1e-4)
    # optimize_model's arithmetic on the chain's q: smooth_l1_loss (mean over 64 x 7), its gradient scattered back through gather (repeats add)
    diff = np.take_along_axis(q.astype(np.float64), action, 1) - expected
    loss = np.where(np.abs(diff) < 1, 0.5 * diff * diff, np.abs(diff) - 0.5).mean()
    assert abs(loss - float(fx["loss"])) <= 1e-5 * abs(loss)
    gq = np.zeros((rows, 132))
    np.add.at(gq, (np.arange(rows)[:, None], action), np.clip(diff, -1, 1) / (7.0 * rows))
    grads, bounds = model.backward(x, params, True, gq.astype(np.float32))
    for n, g, e in zip(NAMES, grads, bounds):
        ok, ratio = cases.within_bound(fx["g_" + n], g, 2 * e)
        assert ok, (n, ratio)
        assert np.array_equal(fx["c_" + n], np.clip(fx["g_" + n], -1, 1))
    assert (np.abs(fx["g_w1"]) > 1).any()
