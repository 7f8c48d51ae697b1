"""CPU tests of the host model of the agents/DQN family's TD head (tests/dqn_learn_model.py) against a torch CPU restatement of
agents/DQN/DQNAgent.py:220-290 and :294-337: gather, topk(7), smooth_l1_loss or the squared form, autograd for gq."""
import numpy as np
import pytest

import dqn_learn_cases as cases
import dqn_learn_model as model

GAMMA = 0.99


def _torch_restatement(c, mode, weighted, masked, dtype):
    """-> (expected [B, 7], loss, gq [B, 132], priorities [B]) as torch computes them in `dtype`"""
    import torch
    tt = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    q_pred, q_next, reward = tt(c["q_pred"]).requires_grad_(True), tt(c["q_next"]), tt(c["reward"])
    action = torch.from_numpy(c["action"])
    valid = (action >= 0) & (action < cases.OUT)
    gathered = torch.gather(q_pred, 1, action.clamp(0, cases.OUT - 1))
    gamma = float(np.float32(GAMMA))
    nxt = q_next.topk(7, 1)[0] * gamma
    if masked:
        nxt = nxt * torch.from_numpy(c["not_done"]).to(dtype)[:, None]
    expected = nxt + reward[:, None]
    w = tt(c["weights"])[:, None] if weighted else torch.ones((len(reward), 1), dtype=dtype)
    td = torch.where(valid, gathered - expected, torch.zeros((), dtype=dtype))          # an out-of-range action is a pair with td = 0
    if mode == "squared":
        per = td.pow(2) * w
        prio = per.mean(1) + float(np.float32(1e-5))
    else:
        per = torch.nn.functional.smooth_l1_loss(td, torch.zeros_like(td), reduction="none") * w
        prio = td.abs().mean(1) + float(np.float32(1e-5))
    loss = per.mean()
    loss.backward()
    return expected.detach().numpy(), float(loss.detach()), q_pred.grad.numpy(), prio.detach().numpy()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", model.MODES)
def test_float64_model_is_the_reference_formulation(mode, weighted, masked):
    import torch
    for seed, B in enumerate((1, 3, 7, 17, 64, 130, 257)):
        c = cases.td_case(B, seed)
        got = model.td_head(c["q_pred"], c["action"], c["q_next"], c["reward"], c["not_done"] if masked else None, c["weights"] if weighted else None, GAMMA, mode)
        expected, loss, gq, prio = _torch_restatement(c, mode, weighted, masked, torch.float64)
        assert np.array_equal(model.top7(c["q_next"]), torch.from_numpy(c["q_next"]).topk(7, 1)[0].numpy())          # ties with multiplicity
        np.testing.assert_allclose(got["estimated"], expected, rtol=1e-14, atol=0)
        np.testing.assert_allclose(got["loss"], loss, rtol=1e-12)
        np.testing.assert_allclose(got["gq"], gq, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(got["priorities"], prio, rtol=1e-12)


@pytest.mark.parametrize("mode", model.MODES)
def test_fp32_order_stays_close_to_the_float64_model_and_to_torch_fp32(mode):
    """the fp32 order's distance from float64 is a few roundings of the pair's magnitude: 16 u (|q| + |est|) per pair covers the header's operations"""
    import torch
    U = 2.0 ** -24
    for seed, B in enumerate((1, 5, 16, 33, 257)):
        c = cases.td_case(B, seed)
        args = (c["q_pred"], c["action"], c["q_next"], c["reward"], c["not_done"], c["weights"], GAMMA, mode)
        want, got = model.td_head(*args), model.td_head32(*args)
        mag = np.abs(c["q_pred"]).max() + np.abs(want["estimated"]).max() + 1.0
        wmax = max(1.0, float(c["weights"].max()))
        assert np.abs(got["estimated"] - want["estimated"]).max() <= 4 * U * mag
        assert np.abs(got["td"] - want["td"]).max() <= 6 * U * mag
        scale = wmax * mag * mag if mode == "squared" else wmax * mag
        assert np.abs(got["gq"] - want["gq"]).max() <= 7 * 16 * U * 2 * scale / (7 * B)
        assert abs(float(got["loss"]) - want["loss"]) <= (16 + B) * U * scale
        assert np.abs(got["priorities"] - want["priorities"]).max() <= 32 * U * scale
        expected, loss, gq, prio = _torch_restatement(c, mode, True, True, torch.float32)
        assert np.abs(got["estimated"] - expected).max() <= 4 * U * mag and abs(float(got["loss"]) - loss) <= (16 + B) * U * scale


def test_planted_rows_select_with_multiplicity_and_out_of_range_actions_add_nothing():
    c = cases.td_case(7, 0)                                 # row i carries plant i
    n = model.top7(c["q_next"])
    assert (n[0] == 0.75).all()                             # all equal: seven instances of the one value
    assert n[1].tolist() == [2.25, 1.125, 0.5, 0.0, 0.0, 0.0, 0.0]       # three positives: the rest are four of the zeros, not one
    assert n[2].tolist() == [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0]
    assert n[3][0] == 11.0 and n[4][0] == 12.0
    for fn in (model.td_head, model.td_head32):
        out = fn(c["q_pred"], c["action"], c["q_next"], c["reward"], None, None, GAMMA, "huber")
        assert np.count_nonzero(out["gq"][5]) == 4 and np.count_nonzero(out["gq"][6]) == 2          # duplicates add; only columns 3 and 131 are valid
        assert (out["td"][6, [1, 2, 3, 6]] == 0).all()
        both = fn(c["q_pred"], np.where((c["action"] < 0) | (c["action"] >= 132), 5, c["action"]), c["q_next"], c["reward"], None, None, GAMMA, "huber")
        assert np.array_equal(np.asarray(out["estimated"]), np.asarray(both["estimated"]))


def test_loss_order_depends_on_the_batch_size_alone_and_caps_the_grid():
    rng = np.random.RandomState(3)
    B = cases.past_cap_batch(model.MAX_BLOCKS)
    rows = rng.rand(B).astype(np.float32)
    a = model.loss_order32(rows, B)
    assert abs(float(a) - rows.astype(np.float64).sum() / (7 * B)) <= 64 * 2.0 ** -24 * float(a)
    assert model.loss_order32(rows[:5], 5) == np.float32(np.float32(np.float32(np.float32(np.float32(rows[0] + rows[1]) + rows[2]) + rows[3]) + rows[4]) / np.float32(35))
