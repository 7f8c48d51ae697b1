"""GPU tests of evg_dqn_td_head / evg_adam_step_wide (include/evg_dqn_learn.h) and of DqnFamilyLearner against the host model of the contract
(tests/dqn_learn_model.py, tests/learner_model.adam32):

  TD head     bit-equal to the fp32-order model (gq, loss, priorities, estimated) in both modes, with and without weights and not_done, at
              B in 1, 3, 16, 17, 64, 257 and 16 x EVG_DQN_TD_MAX_BLOCKS + 19 (every workgroup's sweep loop runs twice, the first three take a third,
              ragged one), the planted rows of tests/dqn_learn_cases.py in every batch; repeatable; sentinels around every output
  wide Adam   bit-equal to adam32 and to evg_adam_step (libevg_learn.so) on copies of the same tensors over five steps: counts (1), (3, 5, 132), the
              105-528-132 network's own, and 4 x 256 x EVG_ADAM_WIDE_MAX_BLOCKS + 1 027 (the grid's stride loop runs twice, then a ragged pass, and
              the tensor ends in a short unit of three elements); fresh_state and clamp on and off; ctl = {k, beta1^k, beta2^k} after k calls
  whole step  step_on at h1 = 48 and 528, B = 64 and 129 (the backward's slices' reduction): the TD head and Adam stages bit-equal to the model on
              the device's own q_pred, q_next and gradients, the gradients within tests/dqn_grad_model's bound, the parameters against
              DqnQNet.with_grad + torch's gather / topk / loss + the model's Adam; a captured step replayed three times == three eager steps
  fixture     three steps of the reference's own optimize_model with a real optim.Adam (tests/golden/dqn_learn.npz)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import dqn_grad_model
import dqn_learn_cases as cases
import dqn_learn_model as model
import learner_model

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
GAMMA = 0.99
KW = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
SENTINEL = F32(-777.25)


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


@pytest.fixture(scope="module")
def env(evg):
    e = evg.EvergladesVecEnv(64, seed=5)
    yield e
    e.close()


@pytest.fixture(scope="module")
def G(evg):
    return evg._lib.load_dqn_learn()


def _dev(env, a):
    import torch
    if isinstance(a, (tuple, list)):
        return [_dev(env, x) for x in a]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


class Guarded(object):
    """a float32 device tensor of n elements between two runs of 64 sentinels (the view starts 256 bytes in: 16-byte aligned)"""

    def __init__(self, env, shape, init=None):
        import torch
        self.n = int(np.prod(shape))
        self.all = torch.full((self.n + 128,), float(SENTINEL), dtype=torch.float32, device=env.device)
        self.t = self.all[64:64 + self.n].view(*shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, F32)).to(env.device).view(*shape))

    def numpy(self):
        a = self.all.cpu().numpy()
        assert (a[:64] == SENTINEL).all() and (a[64 + self.n:] == SENTINEL).all(), "a sentinel next to the tensor was overwritten"
        return a[64:64 + self.n].reshape(tuple(self.t.shape)).copy()


# ---------------------------------------------------------------------- TD head
def _td(evg, env, G, c, mode, weighted, masked, outs=None):
    """one evg_dqn_td_head call on the case c: the four outputs as numpy (sentinels checked)"""
    import torch
    B = c["q_pred"].shape[0]
    ops = {k: _dev(env, c[k]) for k in ("q_pred", "action", "q_next", "reward", "weights")}
    ops["not_done"] = _dev(env, c["not_done"])
    outs = outs or {"gq": Guarded(env, (B, 132)), "loss": Guarded(env, (1,)), "priorities": Guarded(env, (B,)), "estimated": Guarded(env, (B, 7))}
    ws = torch.empty(evg._lib.DQN_TD_WORKSPACE_BYTES // 4, dtype=torch.float32, device=env.device)
    d = evg._lib.EvgDqnTdHeadArgs()
    d.struct_size, d.mode, d.batch, d.gamma = C.sizeof(d), evg._lib.DQN_TD_MODES[mode], B, GAMMA
    d.q_pred, d.action, d.q_next, d.reward = (ops[k].data_ptr() for k in ("q_pred", "action", "q_next", "reward"))
    d.not_done = ops["not_done"].data_ptr() if masked else None
    d.weights = ops["weights"].data_ptr() if weighted else None
    d.gq, d.loss, d.priorities, d.estimated = (outs[k].t.data_ptr() for k in ("gq", "loss", "priorities", "estimated"))
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    rc = G.evg_dqn_td_head(env._h, C.byref(d), env._stream())
    assert rc == 0, G.evg_last_error()
    return {k: g.numpy() for k, g in outs.items()}, outs


def _td_model(c, mode, weighted, masked):
    return model.td_head32(c["q_pred"], c["action"], c["q_next"], c["reward"], c["not_done"] if masked else None, c["weights"] if weighted else None,
                           GAMMA, mode)


def _assert_td_equal(got, want, what):
    for k in ("estimated", "gq", "priorities"):
        differ = int((np.ascontiguousarray(got[k], F32).view(np.uint32) != np.ascontiguousarray(want[k], F32).view(np.uint32)).sum())
        assert differ == 0, (what, k, differ)
    print("%s: loss device %r model %r" % (what, float(got["loss"][0]), float(want["loss"])))
    assert cases.same_bits(got["loss"], np.array([want["loss"]], F32)), (what, "loss", got["loss"], want["loss"])


TD_CONFIGS = [(mode, weighted, masked) for mode in model.MODES for weighted in (False, True) for masked in (False, True)]


@pytest.mark.parametrize("mode,weighted,masked", TD_CONFIGS, ids=["%s-w%d-m%d" % c for c in TD_CONFIGS])
def test_td_head_is_bit_equal_to_the_fp32_model(evg, env, G, mode, weighted, masked):
    seed = TD_CONFIGS.index((mode, weighted, masked))                   # B = 1 meets plants 0..6 (and 0 again) over the eight configurations
    for B in cases.BATCHES:
        c = cases.td_case(B, seed)
        got, _ = _td(evg, env, G, c, mode, weighted, masked)
        _assert_td_equal(got, _td_model(c, mode, weighted, masked), "B %d %s weighted=%d masked=%d" % (B, mode, weighted, masked))


@pytest.mark.parametrize("mode,weighted,masked", [("huber", False, False), ("squared", True, True)], ids=["huber", "squared-w-m"])
def test_td_head_past_the_grid_cap(evg, env, G, mode, weighted, masked):
    B = cases.past_cap_batch(evg._lib.DQN_TD_MAX_BLOCKS)
    assert B == 16 * 1024 + 19 and model.MAX_BLOCKS == evg._lib.DQN_TD_MAX_BLOCKS
    c = cases.td_case(B, 3)
    got, _ = _td(evg, env, G, c, mode, weighted, masked)
    _assert_td_equal(got, _td_model(c, mode, weighted, masked), "B %d %s" % (B, mode))


def test_td_head_every_plant_at_one_row(evg, env, G):
    for seed in range(cases.PLANTS):
        c = cases.td_case(1, seed)
        for mode in model.MODES:
            got, _ = _td(evg, env, G, c, mode, True, False)
            _assert_td_equal(got, _td_model(c, mode, True, False), "plant %d %s" % (seed, mode))


def test_td_head_two_calls_are_bit_equal_and_optional_outputs_may_be_absent(evg, env, G):
    import torch
    c = cases.td_case(257, 2)
    a, outs = _td(evg, env, G, c, "huber", True, True)
    for o in outs.values():
        o.t.fill_(float("nan"))
    b, _ = _td(evg, env, G, c, "huber", True, True, outs)
    assert all(cases.same_bits(a[k], b[k]) for k in a)
    # without priorities and estimated
    B = 257
    ops = {k: _dev(env, c[k]) for k in ("q_pred", "action", "q_next", "reward")}
    gq, loss = Guarded(env, (B, 132)), Guarded(env, (1,))
    ws = torch.empty(evg._lib.DQN_TD_WORKSPACE_BYTES // 4, dtype=torch.float32, device=env.device)
    d = evg._lib.EvgDqnTdHeadArgs()
    d.struct_size, d.mode, d.batch, d.gamma = C.sizeof(d), 0, B, GAMMA
    d.q_pred, d.action, d.q_next, d.reward = (ops[k].data_ptr() for k in ("q_pred", "action", "q_next", "reward"))
    d.gq, d.loss, d.workspace, d.workspace_bytes = gq.t.data_ptr(), loss.t.data_ptr(), ws.data_ptr(), ws.numel() * 4
    assert G.evg_dqn_td_head(env._h, C.byref(d), env._stream()) == 0
    want = _td_model(c, "huber", False, False)
    assert cases.same_bits(gq.numpy(), want["gq"]) and cases.same_bits(loss.numpy(), np.array([want["loss"]], F32))


def test_td_head_and_wide_adam_refusals_with_a_real_handle(evg, env, G):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=env.device)
    cases.check_td_refusals(evg._lib, G, env._h, buf.data_ptr())
    cases.check_adam_refusals(evg._lib, G, env._h, buf.data_ptr())


# ---------------------------------------------------------------------- wide Adam
class AdamState(object):
    def __init__(self, env, params):
        import torch
        self.env = env
        self.p = [Guarded(env, a.shape, a) for a in params]
        self.m = [Guarded(env, a.shape, np.zeros_like(a)) for a in params]
        self.v = [Guarded(env, a.shape, np.zeros_like(a)) for a in params]
        self.ctl = torch.from_numpy(learner_model.ctl_words(learner_model.new_ctl())).to(env.device)

    def host(self):
        return [g.numpy() for g in self.p], [g.numpy() for g in self.m], [g.numpy() for g in self.v], learner_model.ctl_from_words(self.ctl.cpu().numpy())

    def step(self, evg, entry, lib, grads_dev, clamp, fresh):
        a = evg._lib.EvgAdamArgs()
        a.struct_size = C.sizeof(a)
        a.n, a.lr, a.beta1, a.beta2, a.eps, a.clamp, a.fresh_state = len(self.p), KW["lr"], KW["betas"][0], KW["betas"][1], KW["eps"], clamp, int(fresh)
        a.ctl = self.ctl.data_ptr()
        for i, (p, g, m, v) in enumerate(zip(self.p, grads_dev, self.m, self.v)):
            e = a.t[i]
            e.param, e.grad, e.m, e.v, e.count = p.t.data_ptr(), g.data_ptr(), m.t.data_ptr(), v.t.data_ptr(), p.n
        rc = entry(self.env._h, C.byref(a), self.env._stream())
        assert rc == 0, lib.evg_last_error()


ADAM_COUNTS = [(1,), (3, 5, 132), cases.NET_COUNTS, "past_cap"]


@pytest.mark.parametrize("clamp,fresh", [(0.0, False), (1.0, False), (0.0, True), (1.0, True)], ids=["plain", "clamp", "fresh", "clamp-fresh"])
@pytest.mark.parametrize("counts", ADAM_COUNTS, ids=["1", "3-5-132", "network", "past-cap"])
def test_wide_adam_is_bit_equal_to_the_model_and_to_the_one_workgroup_kernel(evg, env, G, counts, clamp, fresh):
    if counts == "past_cap":
        counts = (cases.past_cap_count(evg._lib.ADAM_WIDE_MAX_BLOCKS),)
        assert counts[0] == 4 * 256 * 512 + 1027 and counts[0] % 4 == 3
    L = evg._lib.load_learn()
    params, grads = cases.adam_case(counts, len(counts))
    wide, narrow = AdamState(env, params), AdamState(env, params)
    p32, m32, v32, c32 = params, [np.zeros_like(a) for a in params], [np.zeros_like(a) for a in params], learner_model.new_ctl()
    for s in range(5):
        gd = _dev(env, grads[s])
        wide.step(evg, G.evg_adam_step_wide, G, gd, clamp, fresh)
        narrow.step(evg, L.evg_adam_step, L, gd, clamp, fresh)
        p32, m32, v32, c32 = learner_model.adam32(p32, grads[s], m32, v32, c32, clamp=clamp, fresh=fresh, **KW)
        w, n = wide.host(), narrow.host()
        k = 1 if fresh else s + 1
        assert w[3] == c32 == n[3] and w[3][0] == k, (s, w[3], c32, n[3])
        if not fresh:
            p1 = p2 = 1.0
            for _ in range(k):
                p1, p2 = p1 * float(F32(KW["betas"][0])), p2 * float(F32(KW["betas"][1]))
            assert w[3] == (k, p1, p2)
        for name, a, b, m in zip("p m v".split(), w[:3], n[:3], (p32, m32, v32)):
            for i in range(len(counts)):
                assert cases.same_bits(a[i], m[i]), (s, name, i, "against adam32", int((a[i] != m[i]).sum()))
                assert cases.same_bits(a[i], b[i]), (s, name, i, "against evg_adam_step")
        assert all(torch_equal(g, h) for g, h in zip(gd, _dev(env, grads[s])))                 # the gradients are read, never written


def torch_equal(a, b):
    import torch
    return torch.equal(a, b)


# ---------------------------------------------------------------------- the whole step
def _network(h1, seed):
    rng = np.random.RandomState(seed)
    return [(rng.standard_normal((h1, 105)) * 0.1).astype(F32), (rng.standard_normal(h1) * 0.3).astype(F32),
            (rng.standard_normal((132, h1)) * (2.0 / np.sqrt(h1))).astype(F32), (rng.standard_normal(132) * 0.3).astype(F32)]


def _batch(B, seed):
    rng = np.random.RandomState(seed)
    c = cases.td_case(B, seed)
    return {"state": rng.standard_normal((B, 105)).astype(F32), "next_state": rng.standard_normal((B, 105)).astype(F32), "action": c["action"],
            "reward": c["reward"], "not_done": c["not_done"], "weights": c["weights"]}


@pytest.mark.parametrize("mode,clamp,masked,weighted", [("huber", 1.0, False, False), ("squared", None, True, True)], ids=["optimize_model", "prioritized"])
@pytest.mark.parametrize("B", [64, 129])
@pytest.mark.parametrize("h1", [48, 528])
def test_whole_step_stage_by_stage(evg, env, h1, B, mode, clamp, masked, weighted):
    import torch
    host_policy, host_target, bt = _network(h1, 1), _network(h1, 2), _batch(B, 5)
    policy, target = _dev(env, host_policy), _dev(env, host_target)
    learner = env.dqn_learner(tuple(policy), tuple(target), gamma=GAMMA, mode=mode, clamp=clamp, final_relu=True, **KW)
    d = {k: _dev(env, v) for k, v in bt.items()}
    batch = (d["state"], d["action"], d["next_state"], d["reward"], d["not_done"] if masked else None)
    out = learner.step_on(batch, weights=d["weights"] if weighted else None)
    loss, prio = out if weighted else (out, None)
    assert loss.dim() == 0 and loss.data_ptr() == learner.loss.data_ptr() and all(p.grad is None for p in policy)
    # the forwards are the evaluators' (tests/test_gpu_dqn.py pins those to the fmaf chain)
    assert torch.equal(learner.q_next, env.dqn_qnet(tuple(target), final_relu=True).rows(d["next_state"]))
    q_pred, q_next = learner.q_pred.cpu().numpy(), learner.q_next.cpu().numpy()
    assert np.array_equal(q_pred, dqn_grad_model.chain(bt["state"], host_policy, True)[1])
    # the TD head on the device's own q_pred and q_next
    want = model.td_head32(q_pred, bt["action"], q_next, bt["reward"], bt["not_done"] if masked else None, bt["weights"] if weighted else None, GAMMA, mode)
    gq = learner.gq.cpu().numpy()
    assert cases.same_bits(gq, want["gq"]) and cases.same_bits(loss.cpu().numpy(), want["loss"]) and cases.same_bits(learner.estimated.cpu().numpy(), want["estimated"])
    if weighted:
        assert prio.data_ptr() == learner.priorities.data_ptr() and cases.same_bits(prio.cpu().numpy(), want["priorities"])
    # the backward within its documented bound, on the device's own gq
    grads = [g.cpu().numpy() for g in learner.grads]
    g64, E = dqn_grad_model.backward(bt["state"], host_policy, True, gq, clamp=0.0 if clamp is None else clamp)
    worst = 0.0
    for g, w, e in zip(grads, g64, E):
        err = np.abs(g.astype(np.float64) - w)
        assert (err <= e).all(), float((err / np.maximum(e, 1e-300)).max())
        worst = max(worst, float((err / np.maximum(e, 1e-300)).max()))
    print("h1 %d B %d %s: worst |gradient - model| / E = %.4f" % (h1, B, mode, worst))
    # Adam on the device's own gradients
    zeros = [np.zeros_like(a) for a in host_policy]
    p32, m32, v32, c32 = learner_model.adam32(host_policy, grads, zeros, zeros, learner_model.new_ctl(), **KW)
    assert all(cases.same_bits(a.cpu().numpy(), b) for a, b in zip(policy + learner.m + learner.v, p32 + m32 + v32))
    assert learner_model.ctl_from_words(learner.ctl.cpu().numpy()) == c32 and learner.state_dict()["step"] == 1
    # ... and against DqnQNet.with_grad + torch's gather / topk / loss + the model's Adam.  Both gradients lie within E of the exact backward of their
    # own gq, and torch's gq is the device's to within one rounding per element (at most E / B more): |dg| <= 3 E.  The first Adam step is
    # p - lr g / (|g| + eps) up to roundings (bias-corrected m / sqrt(v) = g / |g|), whose slope in g is at most lr eps / (|g| + eps)^2 over the
    # interval, |g| taken at its smaller end; the update never exceeds lr, and the fp32 operations round p and the update a few times: 4 u (|p| + lr).
    ref = [torch.nn.Parameter(_dev(env, a)) for a in host_policy]
    q = env.dqn_qnet(tuple(ref), final_relu=True).with_grad(d["state"])
    with torch.no_grad():
        nxt = learner.q_next.topk(7, 1)[0] * GAMMA
        if masked:
            nxt = nxt * d["not_done"].float()[:, None]
        expected = nxt + d["reward"][:, None]
    valid = (d["action"] >= 0) & (d["action"] < 132)
    td = torch.where(valid, torch.gather(q, 1, d["action"].clamp(0, 131)) - expected, torch.zeros((), device=env.device))
    if mode == "squared":
        ref_loss = (td.pow(2) * d["weights"][:, None]).mean()
    else:
        ref_loss = torch.nn.functional.smooth_l1_loss(td, torch.zeros_like(td))
    ref_loss.backward()
    ref_grads = [(p.grad.clamp(-clamp, clamp) if clamp else p.grad).cpu().numpy() for p in ref]
    r32 = learner_model.adam32(host_policy, ref_grads, zeros, zeros, learner_model.new_ctl(), **KW)[0]
    assert abs(float(ref_loss.detach()) - float(loss)) <= (16 + B) * 2.0 ** -24 * max(1.0, abs(float(loss)))
    for got, want_p, g, rg, e in zip(p32, r32, grads, ref_grads, E):
        assert (np.abs(g.astype(np.float64) - rg) <= 3 * e + 1e-45).all()
        small = np.maximum(np.minimum(np.abs(g), np.abs(rg)).astype(np.float64) - 3 * e, 0.0)
        tol = np.minimum(KW["lr"] * KW["eps"] / (small + KW["eps"]) ** 2 * 3 * e, 2 * KW["lr"]) + 4 * 2.0 ** -24 * (np.abs(want_p) + KW["lr"])
        assert (np.abs(got.astype(np.float64) - want_p) <= tol).all()


def test_a_captured_step_replayed_three_times_equals_three_eager_steps(evg, env):
    import torch
    h1, B = 528, 129
    host_policy, host_target, bt = _network(h1, 3), _network(h1, 4), _batch(B, 6)
    d = {k: _dev(env, v) for k, v in bt.items()}
    batch = (d["state"], d["action"], d["next_state"], d["reward"], d["not_done"])
    results = []
    for captured in (False, True):
        policy, target = _dev(env, host_policy), _dev(env, host_target)
        learner = env.dqn_learner(tuple(policy), tuple(target), gamma=GAMMA, final_relu=True, **KW)
        losses = []
        if captured:
            s = torch.cuda.Stream(env.device)
            s.wait_stream(torch.cuda.current_stream(env.device))
            with torch.cuda.stream(s):
                learner.step_on(batch)                              # warm-up outside the capture: the buffers of this batch size
            torch.cuda.current_stream(env.device).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                learner.step_on(batch)
            with torch.no_grad():
                for p, a in zip(policy, host_policy):
                    p.copy_(_dev(env, a))
            learner.load_state_dict({"ctl": _dev(env, learner_model.ctl_words(learner_model.new_ctl())), "m": [torch.zeros_like(t) for t in learner.m],
                                     "v": [torch.zeros_like(t) for t in learner.v]})
            for _ in range(3):
                g.replay()
                losses.append(learner.loss.clone())
        else:
            for _ in range(3):
                learner.step_on(batch)
                losses.append(learner.loss.clone())
        results.append([t.clone() for t in policy + learner.m + learner.v + [learner.ctl] + losses])
    assert all(torch.equal(a, b) for a, b in zip(*results))
    assert int(results[0][12][0]) == 3 and not torch.equal(results[0][13], results[0][15])


def test_sync_target_state_dict_and_host_side_checks(evg, env):
    import torch
    policy, target = _dev(env, _network(48, 1)), _dev(env, _network(48, 2))
    learner = env.dqn_learner(tuple(policy), tuple(target), final_relu=True)
    assert isinstance(learner, evg.DqnFamilyLearner)
    learner.sync_target()
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(policy, target))
    bt = _batch(3, 1)
    d = {k: _dev(env, v) for k, v in bt.items()}
    learner.step_on((d["state"], d["action"], d["next_state"], d["reward"], None))
    sd = learner.state_dict()
    assert sd["step"] == 1
    learner.step_on((d["state"], d["action"], d["next_state"], d["reward"], None))
    learner.load_state_dict(sd)
    assert learner.state_dict()["step"] == 1 and all(torch.equal(a, b) for a, b in zip(sd["m"] + sd["v"], learner.m + learner.v))
    with pytest.raises(ValueError, match="action"):
        learner.step_on((d["state"], d["action"][:, :6].contiguous(), d["next_state"], d["reward"], None))
    with pytest.raises(ValueError, match="not_done"):
        learner.step_on((d["state"], d["action"], d["next_state"], d["reward"], d["reward"]))
    with pytest.raises(ValueError, match="same network shape"):
        env.dqn_learner(tuple(policy), tuple(_dev(env, _network(49, 2))), final_relu=True)


# ---------------------------------------------------------------------- the reference's own optimize_model, three steps with a real optim.Adam
# Measured on the CPU (tests/test_dqn_learn_abi.py::test_fixture_tolerance_is_twice_the_fp32_host_models_deviation asserts these figures against the
# fixture): the fp32 host model of the whole step (the exact chain, td_head32, tests/dqn_grad_model's float64 backward rounded to fp32, adam32)
# deviates from the reference's parameters by at most FIXTURE_PARAM_DEV x lr over the compared elements and from its losses by at most
# FIXTURE_LOSS_DEV ulps of the loss.  The bounds are twice that.
from dqn_learn_fixture import FIXTURE_LOSS_BOUND_ULPS, FIXTURE_PARAM_BOUND_LR, fixture_compare, load_fixture   # noqa: E402


def test_three_steps_of_the_references_optimize_model(evg, env):
    fx = load_fixture()
    policy, target = _dev(env, fx["policy"]), _dev(env, fx["target"])
    learner = env.dqn_learner(tuple(policy), tuple(target), lr=1e-4, gamma=float(fx["gamma"]), mode="huber", clamp=1.0, final_relu=True)
    for s in range(3):
        b = fx["batches"][s]
        loss = learner.step_on((_dev(env, b["state"]), _dev(env, b["action"]), _dev(env, b["next_state"]), _dev(env, b["reward"]), None))
        dev_lr, dev_ulps, left_out = fixture_compare(fx, s, [p.cpu().numpy() for p in policy], float(loss))
        print("step %d: largest parameter deviation %.4f lr (bound %.4f), loss deviation %.2f ulps (bound %.2f), %.3f %% of the elements left out" % (
            s, dev_lr, FIXTURE_PARAM_BOUND_LR, dev_ulps, FIXTURE_LOSS_BOUND_ULPS, 100 * left_out))
        assert left_out <= 0.01
        assert dev_lr <= FIXTURE_PARAM_BOUND_LR and dev_ulps <= FIXTURE_LOSS_BOUND_ULPS


def test_training_example_runs_with_the_device_learner():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dqn_training.py"), "256", "60", "128", "--device-learner"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device learner" in out.stdout and "all finite: True" in out.stdout
