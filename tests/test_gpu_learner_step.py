"""GPU tests of evg_td_head / evg_adam_step (include/evg_learn.h) and of DqnLearner against the host model of the contract (tests/learner_model.py):

  TD head   exact tier bit-equal to the model, loss included, at B in 1, 15, 16, 17, 63, 64, 65, 259, 4 099, OUT 5 and 11, the three modes, weights
            absent and present, done rows none / all / alternating with garbage behind them; random tier within the counted E; out-of-range actions;
            repeatability; a captured call; every refusal.  Every output is a view with sentinels on both sides.
  Adam      per step against the model applied to the device's own previous state: five steps from zero, a preset control block, zero gradients,
            tiny and huge gradients, the clamp, fresh_state, in place, repeatable, captured
  chain     DqnLearner.step_on / step on a played memory: every stage buffer against its model applied to the device's own previous-stage buffer"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import learner_cases as cases
import learner_model as model
import qnet_grad_model

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
SENTINEL = -7.5
F32 = np.float32


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
    return evg._lib.load_learn()


def _dev(env, a):
    import torch
    if a is None:
        return None
    if isinstance(a, (tuple, list)):
        return [_dev(env, x) for x in a]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


class Guarded(object):
    """a float32 tensor of `shape` inside a larger buffer of sentinels, 16 bytes from its start"""

    def __init__(self, env, shape, init=None):
        import torch
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 8 + (-self.n) % 4,), SENTINEL, dtype=torch.float32, device=env.device)
        self.t = self.buf[4:4 + self.n].view(shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, F32)))

    def numpy(self):
        """the tensor's values; asserts the sentinels"""
        b = self.buf.cpu().numpy()
        assert (b[:4] == SENTINEL).all() and (b[4 + self.n:] == SENTINEL).all(), "a sentinel was overwritten"
        return b[4:4 + self.n].reshape(tuple(self.t.shape)).copy()


_WS = {}


def _td_args(evg, env, c, out, dev=None):
    """the descriptor of a TD head call on the case c (numpy) with the Guarded outputs `out`; -> (descriptor, the device operands, kept alive)"""
    import torch
    _lib = evg._lib
    if "td" not in _WS:
        _WS["td"] = torch.empty(_lib.TD_HEAD_WORKSPACE_BYTES // 4, dtype=torch.float32, device=env.device)
    if dev is None:
        dev = {k: _dev(env, c[k]) for k in ("q_pred", "action", "q_next", "q_select", "reward", "not_done", "weights")}
    d = _lib.EvgTdHeadArgs()
    d.struct_size = C.sizeof(d)
    d.mode, d.batch, d.out, d.scale = _lib.TD_MODES[c["mode"]], len(c["action"]), c["q_pred"].shape[1], float(c["scale"])
    for k, t in dev.items():
        setattr(d, k, None if t is None else t.data_ptr())
    for k in ("gq", "loss", "priorities", "estimated"):
        setattr(d, k, out[k].t.data_ptr())
    d.workspace, d.workspace_bytes = _WS["td"].data_ptr(), _WS["td"].numel() * 4
    return d, dev


def _outputs(env, B, OUT):
    return {"gq": Guarded(env, (B, OUT)), "loss": Guarded(env, (1,)), "priorities": Guarded(env, (B,)), "estimated": Guarded(env, (B,))}


def _td(evg, env, G, c):
    """one evg_td_head call on the case c: the four outputs as numpy (sentinels checked)"""
    B, OUT = c["q_pred"].shape
    out = _outputs(env, B, OUT)
    d, keep = _td_args(evg, env, c, out)
    rc = G.evg_td_head(env._h, C.byref(d), env._stream())
    assert rc == 0, G.evg_last_error()
    got = {k: o.numpy() for k, o in out.items()}
    got["loss"] = got["loss"][0]
    return got


KEYS = ("estimated", "gq", "priorities", "loss")


# ---------------------------------------------------------------------- TD head: exact tier
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("mode", model.MODES)
@pytest.mark.parametrize("OUT", cases.OUTS)
def test_td_head_exact_tier_is_bit_equal_to_the_host_model(evg, env, G, OUT, mode, weighted):
    for B in cases.BATCHES:
        for done in ("none", "all", "alternating"):
            c = cases.td_exact(B, OUT, mode, weighted, done)
            want, _ = model.td_head(exact=True, **c)
            got = _td(evg, env, G, c)
            for k in KEYS:
                assert cases.same_bits(got[k], want[k]), (k, B, done, np.asarray(got[k]).ravel()[:8], np.asarray(want[k]).ravel()[:8])
            assert (got["gq"] != 0).sum() <= B


# ---------------------------------------------------------------------- TD head: random tier
WORST = {}


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("mode", model.MODES)
@pytest.mark.parametrize("OUT", cases.OUTS)
def test_td_head_random_tier_stays_within_the_counted_bound(evg, env, G, OUT, mode, weighted):
    worst = 0.0
    for B in cases.BATCHES:
        c = cases.td_random(B, OUT, mode, weighted)
        want, E = model.td_head(**c)
        got = _td(evg, env, G, c)
        for k in KEYS:
            ok, ratio = cases.within(got[k], want[k], E[k])
            print("OUT %d %s weighted=%d B=%d %s: |device - model| / E = %.4f" % (OUT, mode, weighted, B, k, ratio))
            worst = max(worst, ratio)
            assert ok, (k, B, ratio)
    WORST[(OUT, mode, weighted)] = worst
    print("OUT %d %s weighted=%d: worst ratio %.4f (all cases so far: %.4f)" % (OUT, mode, weighted, worst, max(WORST.values())))


def test_td_head_fp32_order_model_is_the_device_bit_for_bit(evg, env, G):
    """the header's operation order, the order of the loss sum included: the random tier's values are the fp32 model's own bits"""
    for OUT, mode, B in ((5, "max_mean", 259), (11, "double_mean", 4099), (5, "max_max", 65)):
        c = cases.td_random(B, OUT, mode, True)
        want = model.td_head32(**c)
        got = _td(evg, env, G, c)
        for k in KEYS:
            assert cases.same_bits(got[k], want[k]), (k, OUT, mode, B)


# ---------------------------------------------------------------------- TD head: properties
@pytest.mark.parametrize("OUT", cases.OUTS)
def test_out_of_range_actions_write_a_zero_row_and_nothing_else(evg, env, G, OUT):
    rows = [3, 17, 64]
    c = cases.td_random(65, OUT, "max_mean", True)
    c["action"][rows] = [-1, OUT, 2 ** 40]
    want, E = model.td_head(**c)
    got = _td(evg, env, G, c)                                   # (the sentinels around gq and the others are checked in _td)
    assert not got["gq"][rows].any() and (got["priorities"][rows] == F32(1e-5)).all()
    for k in KEYS:
        assert cases.within(got[k], want[k], E[k])[0], k
    keep = np.ones(65, bool)
    keep[rows] = False
    assert (got["gq"][keep] != 0).sum() == 62


def test_td_head_two_calls_are_bit_equal_and_a_captured_call_replays(evg, env, G):
    import torch
    c = cases.td_random(4099, 11, "double_mean", True)
    first, second = _td(evg, env, G, c), _td(evg, env, G, c)
    for k in KEYS:
        assert np.array_equal(np.asarray(first[k]).view(np.uint32), np.asarray(second[k]).view(np.uint32)), k
    out = _outputs(env, 4099, 11)
    d, dev = _td_args(evg, env, c, out)
    s = torch.cuda.Stream(env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(s):
        assert G.evg_td_head(env._h, C.byref(d), env._stream()) == 0
    torch.cuda.current_stream(env.device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert G.evg_td_head(env._h, C.byref(d), env._stream()) == 0
    for o in out.values():
        o.t.fill_(3.0)
    g.replay()
    for k in KEYS:
        assert np.array_equal(out[k].numpy().ravel().view(np.uint32), np.asarray(first[k]).ravel().view(np.uint32)), k
    dev["reward"].add_(1.0)                                     # the replay reads the operands as they are now
    g.replay()
    c2 = dict(c, reward=c["reward"] + F32(1.0))
    want = _td(evg, env, G, c2)
    for k in KEYS:
        assert np.array_equal(out[k].numpy().ravel().view(np.uint32), np.asarray(want[k]).ravel().view(np.uint32)), k
    assert want["loss"] != first["loss"]


def test_td_head_refusals_and_their_texts(evg, env, G):
    import torch
    c = cases.td_random(37, 5, "max_mean", True)
    out = _outputs(env, 37, 5)
    for o in out.values():
        o.t.fill_(7.0)
    base, dev = _td_args(evg, env, c, out)

    def refused(text, **kw):
        d = evg._lib.EvgTdHeadArgs.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(d, k, v)
        assert G.evg_td_head(env._h, C.byref(d), env._stream()) == -1, kw
        assert text in G.evg_last_error().decode(), (text, G.evg_last_error())

    assert G.evg_td_head(None, C.byref(base), None) == -1 and "null handle" in G.evg_last_error().decode()
    assert G.evg_td_head(env._h, None, None) == -1 and "null handle" in G.evg_last_error().decode()
    refused("struct_size", struct_size=64)
    for B in (0, -1, (1 << 20) + 1):
        refused("batch must lie in", batch=B)
    for o in (0, 4, 6, 12):
        refused("out must be 5 or 11", out=o)
    for m in (-1, 3):
        refused("unknown mode", mode=m)
    for s in (float("inf"), float("nan")):
        refused("scale must be finite", scale=s)
    for name in ("q_pred", "action", "q_next", "reward", "not_done", "gq", "loss", "workspace"):
        refused("%s is NULL" % name, **{name: None})
    refused("q_select is NULL", mode=2)
    for name in ("q_pred", "action", "q_next", "q_select", "reward", "not_done", "weights", "gq", "loss", "priorities", "estimated", "workspace"):
        refused("%s must be 16-byte aligned" % name, **{name: dev["q_pred"].data_ptr() + 4})
    refused("workspace is too small", workspace_bytes=evg._lib.TD_HEAD_WORKSPACE_BYTES - 4)
    torch.cuda.synchronize()
    assert all(bool((o.t == 7.0).all()) for o in out.values())          # nothing was launched
    # the optional pointers may be absent
    d = evg._lib.EvgTdHeadArgs.from_buffer_copy(base)
    d.weights = d.priorities = d.estimated = None
    assert G.evg_td_head(env._h, C.byref(d), env._stream()) == 0
    want, E = model.td_head(**dict(c, weights=None))
    assert cases.within(out["gq"].numpy(), want["gq"], E["gq"])[0] and cases.within(out["loss"].numpy()[0], want["loss"], E["loss"])[0]
    assert (out["priorities"].numpy() == 7.0).all() and (out["estimated"].numpy() == 7.0).all()


# ---------------------------------------------------------------------- Adam
KW = dict(lr=float(F32(1e-3)), betas=(float(F32(0.9)), float(F32(0.999))), eps=float(F32(1e-8)))


class AdamState(object):
    """a network's parameters, moments and control block on the device, each tensor guarded"""

    def __init__(self, env, params, m=None, v=None, ctl=None):
        import torch
        self.env = env
        self.p = [Guarded(env, a.shape, a) for a in params]
        self.m = [Guarded(env, a.shape, np.zeros_like(a) if m is None else m[i]) for i, a in enumerate(params)]
        self.v = [Guarded(env, a.shape, np.zeros_like(a) if v is None else v[i]) for i, a in enumerate(params)]
        self.ctl = torch.from_numpy(model.ctl_words(model.new_ctl() if ctl is None else ctl)).to(env.device)

    def host(self):
        return [g.numpy() for g in self.p], [g.numpy() for g in self.m], [g.numpy() for g in self.v], model.ctl_from_words(self.ctl.cpu().numpy())

    def descriptor(self, evg, grads_dev, clamp=0.0, fresh=False, kw=KW):
        a = evg._lib.EvgAdamArgs()
        a.struct_size = C.sizeof(a)
        a.n, a.lr, a.beta1, a.beta2, a.eps, a.clamp, a.fresh_state = len(self.p), kw["lr"], kw["betas"][0], kw["betas"][1], kw["eps"], clamp, int(fresh)
        a.ctl = self.ctl.data_ptr()
        for i, (p, g, m, v) in enumerate(zip(self.p, grads_dev, self.m, self.v)):
            e = a.t[i]
            e.param, e.grad, e.m, e.v, e.count = p.t.data_ptr(), g.data_ptr(), m.t.data_ptr(), v.t.data_ptr(), p.n
        return a

    def step(self, evg, G, grads, clamp=0.0, fresh=False, kw=KW):
        gd = _dev(self.env, grads)
        a = self.descriptor(evg, gd, clamp, fresh, kw)
        rc = G.evg_adam_step(self.env._h, C.byref(a), self.env._stream())
        assert rc == 0, G.evg_last_error()
        return gd


def _check_step(before, after, grads, clamp=0.0, fresh=False, kw=KW, what=""):
    """`after` against the model applied to `before` (both AdamState.host()); -> the worst ratio"""
    (wp, wm, wv, wctl), (Ep, Em, Ev) = model.adam(before[0], grads, before[1], before[2], before[3], clamp=clamp, fresh=fresh, **kw)
    assert after[3] == wctl, (what, after[3], wctl)
    worst = 0.0
    for got, want, E in zip(after[0] + after[1] + after[2], wp + wm + wv, Ep + Em + Ev):
        ok, ratio = cases.within(got, want, E)
        worst = max(worst, ratio)
        assert ok and np.isfinite(got).all(), (what, ratio)
    return worst


@pytest.mark.parametrize("kind,hidden", cases.ADAM_NETS, ids=cases.ADAM_IDS)
def test_adam_five_steps_from_zero_state_match_the_model(evg, env, G, kind, hidden):
    """each of the five steps against the model applied to the state the device itself left (elementwise, sentinels around param, m and v), and the
    fp32-order model run on its own from the start bit for bit"""
    params, grads = cases.adam_case(kind, hidden)
    st = AdamState(env, params)
    p32, m32, v32, c32 = params, [np.zeros_like(a) for a in params], [np.zeros_like(a) for a in params], model.new_ctl()
    worst = 0.0
    for s in range(5):
        before = st.host()
        st.step(evg, G, grads(s))
        after = st.host()
        worst = max(worst, _check_step(before, after, grads(s), what="step %d" % s))
        p32, m32, v32, c32 = model.adam32(p32, grads(s), m32, v32, c32, **KW)
        assert after[3] == c32 and after[3][0] == s + 1
        assert all(cases.same_bits(a, b) for a, b in zip(after[0] + after[1] + after[2], p32 + m32 + v32)), s
    print("%s %s: worst |device - model| / E over five steps = %.4f" % (kind, hidden, worst))


@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_adam_preset_control_block_zero_gradients_extreme_gradients_and_clamp(evg, env, G, kind, hidden):
    params, grads = cases.adam_case(kind, hidden)
    r = np.random.default_rng(3)
    # step 1 000 with consistent products and used moments
    ctl = (1000, KW["betas"][0] ** 1000, KW["betas"][1] ** 1000)
    m0 = [(r.standard_normal(a.shape) * 0.1).astype(F32) for a in params]
    v0 = [(r.random(a.shape) * 0.01).astype(F32) for a in params]
    st = AdamState(env, params, m0, v0, ctl)
    before = st.host()
    st.step(evg, G, grads(0))
    after = st.host()
    _check_step(before, after, grads(0), what="step 1001")
    assert after[3][0] == 1001
    # zero gradients and zero state: the parameters keep their bits
    st = AdamState(env, params)
    st.step(evg, G, [np.zeros_like(a) for a in params])
    after = st.host()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(after[0], params)) and after[3][0] == 1
    assert not any(a.any() for a in after[1] + after[2])
    # gradients of 1e-20 and 1e+15
    for scale in (1e-20, 1e15):
        _, gs = cases.adam_case(kind, hidden, grad_scale=scale)
        st = AdamState(env, params)
        for s in range(2):
            before = st.host()
            st.step(evg, G, gs(s))
            _check_step(before, st.host(), gs(s), what="gradients of %g, step %d" % (scale, s))
    # the clamp, on and off: gradients of scale 3 are clamped to [-1, 1] as they are read
    _, gs = cases.adam_case(kind, hidden, grad_scale=3.0)
    assert any((np.abs(g) > 1).any() for g in gs(0))
    results = []
    for clamp in (0.0, 1.0):
        st = AdamState(env, params)
        before = st.host()
        st.step(evg, G, gs(0), clamp=clamp)
        after = st.host()
        _check_step(before, after, gs(0), clamp=clamp, what="clamp %g" % clamp)
        results.append(after)
    assert not np.array_equal(results[0][2][0], results[1][2][0])
    assert all((np.abs(m) <= (1 - KW["betas"][0]) * 1.0000001).all() for m in results[1][1])


@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_adam_fresh_state_is_a_new_optimizer_every_step(evg, env, G, kind, hidden):
    params, grads = cases.adam_case(kind, hidden)
    r = np.random.default_rng(4)
    junk = [r.standard_normal(a.shape).astype(F32) for a in params]
    st = AdamState(env, params, junk, [np.abs(j) for j in junk], (77, 0.5, 0.25))       # stored state a fresh step must ignore
    moved = []
    for s in range(2):
        before = st.host()
        st.step(evg, G, grads(0), fresh=True)
        after = st.host()
        _check_step(before, after, grads(0), fresh=True, what="fresh step %d" % s)
        assert after[3] == (1, KW["betas"][0], KW["betas"][1])
        moved.append([a.astype(np.float64) - b.astype(np.float64) for a, b in zip(after[0], before[0])])
    # equal gradients, fresh state: both steps are -lr * sign(g) up to eps and the rounding of the subtraction
    for a, b, p in zip(moved[0], moved[1], params):
        assert (np.abs(a - b) <= 2 * np.spacing(np.abs(p) + KW["lr"]).astype(np.float64)).all() and np.abs(a).max() > 0.5 * KW["lr"]


def test_adam_updates_in_place_is_repeatable_and_replays_from_a_graph(evg, env, G):
    import torch
    policy = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5)).to(env.device)
    target = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5)).to(env.device)
    mem = env.smart_replay(4)
    learner = env.smart_learner(policy, target, mem, lr=1e-2)
    bound = env.smart_qnet(policy)                              # an evaluator bound before the step
    x = _dev(env, np.random.default_rng(0).standard_normal((17, 59)).astype(F32))
    q0 = bound.expanded(x).clone()
    ptrs = [p.data_ptr() for p in policy.parameters()]
    start = [p.detach().clone() for p in policy.parameters()]
    grads = [torch.from_numpy(np.random.default_rng(i).standard_normal(tuple(p.shape)).astype(F32)).to(env.device) for i, p in enumerate(start)]

    def restart():
        with torch.no_grad():
            for p, s in zip(policy.parameters(), start):
                p.copy_(s)
        learner.load_state_dict(zero)

    zero = learner.state_dict()
    assert zero["step"] == 0
    for _ in range(3):
        learner.adam_step(grads=grads)
    plain = [p.detach().clone() for p in policy.parameters()]
    sd = learner.state_dict()
    assert sd["step"] == 3 and [p.data_ptr() for p in policy.parameters()] == ptrs
    assert all(p.grad is None for p in policy.parameters())    # the learner owns its gradients
    q1 = bound.expanded(x)
    assert not torch.equal(q0, q1)
    host = [t.cpu().numpy() for t in plain]
    assert np.array_equal(q1.cpu().numpy(), __import__("qnet_model").forward(x.cpu().numpy(), host, False))
    # repeatable bit for bit from equal starting state; state_dict round-trips
    restart()
    assert learner.state_dict()["step"] == 0 and not any(bool(t.any()) for t in learner.m + learner.v)
    for _ in range(3):
        learner.adam_step(grads=grads)
    assert all(torch.equal(a, b.detach()) for a, b in zip(plain, policy.parameters()))
    again = learner.state_dict()
    assert again["step"] == 3 and torch.equal(again["ctl"], sd["ctl"]) and all(torch.equal(a, b) for a, b in zip(again["m"] + again["v"], sd["m"] + sd["v"]))
    # captured and replayed three times == three plain calls
    restart()
    s = torch.cuda.Stream(env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(s):
        learner.adam_step(grads=grads)                          # warm-up outside the capture
    torch.cuda.current_stream(env.device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        learner.adam_step(grads=grads)
    restart()
    for _ in range(3):
        g.replay()
    assert all(torch.equal(a, b.detach()) for a, b in zip(plain, policy.parameters()))
    assert learner.state_dict()["step"] == 3 and torch.equal(learner.ctl, sd["ctl"])


def test_adam_refusals_and_their_texts(evg, env, G):
    import torch
    params, grads = cases.adam_case("mini", (80,))
    st = AdamState(env, params)
    gd = _dev(env, grads(0))
    base = st.descriptor(evg, gd)

    def refused(text, tensor=None, **kw):
        a = evg._lib.EvgAdamArgs.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(a, k, v)
        if tensor is not None:
            setattr(a.t[tensor[0]], tensor[1], tensor[2])
        assert G.evg_adam_step(env._h, C.byref(a), env._stream()) == -1, (kw, tensor)
        assert text in G.evg_last_error().decode(), (text, G.evg_last_error())

    assert G.evg_adam_step(None, C.byref(base), None) == -1 and "null handle" in G.evg_last_error().decode()
    assert G.evg_adam_step(env._h, None, None) == -1 and "null handle" in G.evg_last_error().decode()
    refused("struct_size", struct_size=16)
    for n in (0, 7, -1):
        refused("n must lie in 1..6", n=n)
    for lr in (float("inf"), float("nan")):
        refused("lr must be finite", lr=lr)
    for b in (-0.1, 1.0, float("nan")):
        refused("betas must lie in [0, 1)", beta1=b)
        refused("betas must lie in [0, 1)", beta2=b)
    for e in (0.0, -1e-8, float("inf"), float("nan")):
        refused("eps must be finite and > 0", eps=e)
    for c in (-1.0, float("inf"), float("nan")):
        refused("clamp must be finite and >= 0", clamp=c)
    refused("ctl is NULL", ctl=None)
    refused("ctl must be 16-byte aligned", ctl=st.ctl.data_ptr() + 8)
    for i in (0, 3):
        for name in ("param", "grad", "m", "v"):
            refused("tensor %d: %s is NULL" % (i, name), tensor=(i, name, None))
            refused("tensor %d: %s must be 16-byte aligned" % (i, name), tensor=(i, name, gd[0].data_ptr() + 4))
        for count in (0, -5, (1 << 24) + 1):
            refused("tensor %d: count must lie in" % i, tensor=(i, "count", count))
    torch.cuda.synchronize()
    after = st.host()                                           # nothing was launched
    assert all(np.array_equal(a, b) for a, b in zip(after[0], params)) and after[3] == model.new_ctl()


# ---------------------------------------------------------------------- the chain
def _modules(env, kind, seed):
    import torch
    torch.manual_seed(seed)
    if kind == "smart":
        net = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5))
    else:
        net = torch.nn.Sequential(torch.nn.Linear(59, 80), torch.nn.ReLU(), torch.nn.Linear(80, 11), torch.nn.ReLU())
    return net.to(env.device)


def _played(evg, kind, prioritized, turns=12):
    """256 envs, `turns` turns of step_vs_q from the policy's Q with the memory recording: (env, policy, target, mem)"""
    env = evg.EvergladesVecEnv(256, seed=11, auto_reset=True)
    policy, target = _modules(env, kind, 0), _modules(env, kind, 1)
    make = env.prioritized_replay if prioritized else env.smart_replay
    mem = make(8, n_step=1, gamma=0.999, shaping="reward_short_games" if kind == "smart" else "custom", seats=0)
    act = (env.smart_qnet if kind == "smart" else env.minimized_qnet)(policy)
    env.reset()
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    for t in range(turns):
        q = act(*mem.slot_features(t))
        if kind == "smart":
            env.step_vs_q("swarm_agent", q, 0.3, seat=0, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
            mem.record()
        else:
            env.step_vs_q("random_actions", q, 0.3, seat=0, features=mem.slot_features(t + 1), actions_out=mem.slot_directions(t))
            mem.record(shaped=(env.reward[:, 0] / 10000.0).contiguous())
    return env, policy, target, mem


def _np(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
@pytest.mark.parametrize("mode", ["max_mean", "double_mean"])
@pytest.mark.parametrize("kind", ["smart", "minimized"])
def test_every_stage_of_a_step_agrees_with_its_model_on_the_devices_own_operands(evg, kind, mode, prioritized):
    import torch
    env, policy, target, mem = _played(evg, kind, prioritized)
    try:
        make = env.smart_learner if kind == "smart" else env.minimized_learner
        learner = make(policy, target, mem, lr=1e-3, gamma=0.999, n_step=1, mode=mode, clamp=1.0)
        final_relu = learner.policy_net.final_relu
        B = 64
        for call in range(3):
            if prioritized:
                out = mem.sample(B, seed=call + 1, beta=0.4)
                weights, handles = out[5].clone(), out[6].clone()
            else:
                weights, handles = None, mem.sample(B, seed=call + 1, return_handles=True)[5].clone()
            batch = mem.gather(handles)
            x, action, nxt, reward, not_done = (t.cpu().numpy().copy() for t in batch)
            assert not_done.any() and np.abs(x).sum() > 0
            # the state before the step
            params = _np(policy.parameters())
            m0, v0, ctl0 = _np(learner.m), _np(learner.v), model.ctl_from_words(learner.ctl.cpu().numpy())
            want_pred = learner.policy_net.expanded(batch[0]).cpu().numpy()
            want_next = learner.target_net.expanded(batch[2]).cpu().numpy()
            want_sel = learner.select_net.expanded(batch[2]).cpu().numpy() if mode == "double_mean" else None
            ret = learner.step_on(batch, weights=weights)
            loss = (ret[0] if prioritized else ret)
            assert loss.dim() == 0 and loss.data_ptr() == learner.loss.data_ptr()
            if prioritized:
                assert ret[1].data_ptr() == learner.priorities.data_ptr()
            # forwards: bit-equal to expanded
            q_pred, q_next = learner.q_pred.cpu().numpy(), learner.q_next.cpu().numpy()
            assert np.array_equal(q_pred.view(np.uint32), want_pred.view(np.uint32)) and np.array_equal(q_next.view(np.uint32), want_next.view(np.uint32))
            q_sel = None
            if mode == "double_mean":
                q_sel = learner.q_select.cpu().numpy()
                assert np.array_equal(q_sel.view(np.uint32), want_sel.view(np.uint32))
            else:
                assert learner.q_select is None
            # TD head on the device's own Q
            w_np = None if weights is None else weights.cpu().numpy()
            want, E = model.td_head(q_pred, action, q_next, q_sel, reward, not_done, w_np, F32(0.999), mode)
            gq = learner.gq.cpu().numpy()
            for k, got in (("gq", gq), ("loss", float(loss.item())), ("priorities", learner.priorities.cpu().numpy()),
                           ("estimated", learner.estimated.cpu().numpy())):
                ok, ratio = cases.within(got, want[k], E[k])
                assert ok, (call, k, ratio)
            assert (gq != 0).any()
            # backward on the device's own gq
            gwant, gE = qnet_grad_model.backward(x, params, final_relu, gq, clamp=1.0)
            grads = _np(learner.grads)
            for i, (g, w, e) in enumerate(zip(grads, gwant, gE)):
                ok, ratio = cases.within(g, w, e)
                assert ok, (call, "gradient %d" % i, ratio)
            assert any(g.any() for g in grads)
            # Adam on the device's own gradients
            f = lambda v: float(F32(v))
            (wp, wm, wv, wctl), (Ep, Em, Ev) = model.adam(params, grads, m0, v0, ctl0, lr=f(1e-3), betas=(f(0.9), f(0.999)), eps=f(1e-8))
            after = _np(policy.parameters()) + _np(learner.m) + _np(learner.v)
            for i, (got, w, e) in enumerate(zip(after, wp + wm + wv, Ep + Em + Ev)):
                ok, ratio = cases.within(got, w, e)
                assert ok, (call, "parameter / m / v %d" % i, ratio)
            assert model.ctl_from_words(learner.ctl.cpu().numpy()) == wctl and wctl[0] == call + 1
            assert any(not np.array_equal(a, b) for a, b in zip(after, params))
            assert all(p.grad is None for p in policy.parameters())
        mem.check()
    finally:
        env.close()


@pytest.mark.parametrize("kind", ["smart", "minimized"])
def test_step_draws_what_sample_draws_updates_priorities_and_syncs_the_target(evg, kind):
    import torch
    env, policy, target, mem = _played(evg, kind, True)
    try:
        make = env.smart_learner if kind == "smart" else env.minimized_learner
        learner = make(policy, target, mem, lr=1e-3, beta=0.4)
        B = 64
        # what mem.sample draws with this seed at this call index
        calls = mem.sample_calls.clone()
        out = mem.sample(B, seed=9, beta=0.4)
        drawn = [t.cpu().numpy().copy() for t in out]
        mem.sample_calls.copy_(calls)                           # repeat the draw
        plane0 = mem.priorities.cpu().numpy().copy()
        params = _np(policy.parameters())
        loss = learner.step(B, 9)
        assert int(mem.sample_calls.item()) == int(calls.item()) + 1
        batch_now = [t.cpu().numpy() for t in mem._outputs(B)]
        for a, b in zip(drawn[:5] + [drawn[6]], batch_now):
            assert np.array_equal(a, b)
        # the step computed on that batch: the model's TD head on the device's Q gives the priorities now in the memory
        want, E = model.td_head(learner.q_pred.cpu().numpy(), drawn[1], learner.q_next.cpu().numpy(), None, drawn[3], drawn[4], drawn[5], F32(0.999),
                                "max_mean")
        prio = learner.priorities.cpu().numpy()
        assert cases.within(prio, want["priorities"], E["priorities"])[0] and cases.within(float(loss.item()), want["loss"], E["loss"])[0]
        plane1 = mem.priorities.cpu().numpy()
        handles = drawn[6]
        # No priority was stored before this step, and a record keeps its transitions' weights in the order of their rows: the non-zero entries of a
        # record named by the batch are the weights of its drawn rows, ascending.  A transition named several times keeps the largest priority; the
        # weight is priority ** alpha within 2 float32 ulps (tests/test_gpu_replay_priority.py).
        assert not plane0[..., :7].any()
        records = 0
        for rec in np.unique(handles[:, :3], axis=0):
            slot, e, seat = (int(v) for v in rec)
            named = (handles[:, :3] == rec).all(1)
            want_w = [F32(prio[named & (handles[:, 3] == row)].astype(np.float64).max() ** float(F32(0.6))) for row in np.unique(handles[named, 3])]
            stored = plane1[slot, e, seat, :7]
            stored = stored[stored != 0]
            assert len(stored) == len(want_w), (rec, stored, want_w)
            assert all(abs(float(s) - float(w)) <= 2 * float(np.spacing(w)) for s, w in zip(stored, want_w)), (rec, stored, want_w)
            records += 1
        assert records > 0 and np.count_nonzero(plane1[..., :7]) == len(np.unique(handles, axis=0))
        mem.check()
        assert any(not np.array_equal(a, b) for a, b in zip(_np(policy.parameters()), params))
        # sync_target and the state_dict round trip
        assert not all(torch.equal(a, b) for a, b in zip(policy.parameters(), target.parameters()))
        tptr = [p.data_ptr() for p in target.parameters()]
        learner.sync_target()
        assert all(torch.equal(a, b) for a, b in zip(policy.parameters(), target.parameters())) and tptr == [p.data_ptr() for p in target.parameters()]
        sd = learner.state_dict()
        assert sd["step"] == 1
        other = make(policy, target, mem)
        other.load_state_dict(sd)
        assert torch.equal(other.ctl, learner.ctl) and all(torch.equal(a, b) for a, b in zip(other.m + other.v, learner.m + learner.v))
        assert other.state_dict()["step"] == 1
    finally:
        env.close()


def test_step_on_a_plain_memory_draws_what_sample_draws(evg):
    env, policy, target, mem = _played(evg, "smart", False)
    try:
        learner = env.smart_learner(policy, target, mem)
        calls = mem.sample_calls.clone()
        drawn = [t.cpu().numpy().copy() for t in mem.sample(64, seed=9, return_handles=True)]
        mem.sample_calls.copy_(calls)                           # repeat the draw
        want_pred = learner.policy_net.expanded(mem._outputs(64)[0]).cpu().numpy()
        loss = learner.step(64, 9)
        assert int(mem.sample_calls.item()) == int(calls.item()) + 1
        for a, b in zip(drawn, mem._outputs(64)):
            assert np.array_equal(a, b.cpu().numpy())
        q_pred = learner.q_pred.cpu().numpy()
        assert np.array_equal(q_pred.view(np.uint32), want_pred.view(np.uint32))
        want, E = model.td_head(q_pred, drawn[1], learner.q_next.cpu().numpy(), None, drawn[3], drawn[4], None, F32(0.999), "max_mean")
        assert cases.within(float(loss.item()), want["loss"], E["loss"])[0] and cases.within(learner.gq.cpu().numpy(), want["gq"], E["gq"])[0]
        mem.check()
    finally:
        env.close()


def test_bf16_target_and_the_blind_target_run_through_the_chain(evg):
    """target_precision="bf16" with the double mode (selection and evaluation are both inference) and mode="max_max": q_next is the bf16 evaluator's,
    the TD head's outputs agree with the model on it"""
    env, policy, target, mem = _played(evg, "smart", False)
    try:
        for mode, precision in (("double_mean", "bf16"), ("max_max", "fp32")):
            learner = env.smart_learner(policy, target, mem, mode=mode, target_precision=precision)
            handles = mem.sample(64, seed=3, return_handles=True)[5].clone()
            batch = mem.gather(handles)
            x, action, nxt, reward, not_done = (t.cpu().numpy().copy() for t in batch)
            want_next = env.smart_qnet(target, precision=precision).expanded(batch[2]).cpu().numpy()
            loss = learner.step_on(batch)
            q_next = learner.q_next.cpu().numpy()
            assert np.array_equal(q_next.view(np.uint32), want_next.view(np.uint32))
            q_sel = learner.q_select.cpu().numpy() if mode == "double_mean" else None
            want, E = model.td_head(learner.q_pred.cpu().numpy(), action, q_next, q_sel, reward, not_done, None, F32(0.999), mode)
            assert cases.within(learner.gq.cpu().numpy(), want["gq"], E["gq"])[0] and cases.within(float(loss.item()), want["loss"], E["loss"])[0]
    finally:
        env.close()


@pytest.mark.parametrize("example,extra", [("smart_state_training.py", []), ("smart_state_training.py", ["--prioritized", "--acting-precision", "bf16"]),
                                           ("minimized_training.py", [])], ids=["smart", "smart-prioritized-bf16", "minimized"])
def test_training_examples_run_with_the_device_learner(example, extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", example), "256", "12", "64", "--device-learner"] + extra,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "device learner" in out.stdout and "all finite: True" in out.stdout, out.stdout[-2000:]
