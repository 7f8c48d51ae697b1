"""GPU tests of evg_smart_qnet_backward / evg_minimized_qnet_backward and of SmartQNet.with_grad / MinimizedQNet.with_grad (include/evg_qnet_grad.h)
against the host model of the contract (tests/qnet_grad_model.py):

  exact tier    the families of tests/qnet_grad_cases.py (integer, permutation, pow2dup): bit-equal gradients at B in 1, 15, 16, 17, 63, 65, 259, and
                (integer) at two sweeps of the capped grid plus 19 rows
  random tier   dense and gathered: every element within the model's derived E
  properties    rows with gq = 0, a dead unit's row, the clamp, sentinels around the gradient tensors, repeatability, a captured call
  autograd      with_grad's forward is expanded's; gather -> smooth_l1_loss -> backward fills .grad; a second backward accumulates; refusals
  neighbours    the fp32 and bf16 evaluators with the new library loaded; the two training examples with --device-backward"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import qnet_grad_cases as cases
import qnet_grad_model as model
import qnet_model
import minimized_model

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
FINAL_RELU = [False, True]


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


def _dev(env, a):
    import torch
    if isinstance(a, (tuple, list)):
        return tuple(_dev(env, x) for x in a)
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _net(env, kind, dev_params, final_relu, precision="fp32"):
    make = env.smart_qnet if kind == "smart" else env.minimized_qnet
    return make(dev_params, final_relu=final_relu, precision=precision)


def _grads(net, dev_params, x, gq, clamp=0.0):
    """the entry point itself: the gradients of dev_params for (x, gq), as numpy"""
    return [g.cpu().numpy() for g in net._backward(x, dev_params, gq, clamp)]


# ---------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("final_relu", FINAL_RELU)
@pytest.mark.parametrize("family", cases.EXACT_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_exact_tier_is_bit_equal_to_the_host_model(env, kind, hidden, family, final_relu):
    params, x, gq = cases.case(kind, hidden, family, cases.ROWS[-1])
    dp = _dev(env, params)
    net = _net(env, kind, dp, final_relu)
    for rows in cases.ROWS:
        if family == "pow2dup":
            _, x, gq = cases.case(kind, hidden, family, rows)
        want, _ = model.backward(x[:rows], params, final_relu, gq[:rows], exact=True)
        got = _grads(net, dp, _dev(env, x[:rows]), _dev(env, gq[:rows]))
        differ = [int((g != w).sum()) for g, w in zip(got, want)]
        print("%s %s %s final_relu=%d rows=%d: elements that differ %s, largest |gradient| %g" % (
            kind, hidden, family, final_relu, rows, differ, max(np.abs(w).max() for w in want)))
        assert all(cases.same_values(g, w) for g, w in zip(got, want)), (rows, differ)


@pytest.mark.parametrize("final_relu", FINAL_RELU)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_exact_tier_over_two_sweeps_of_the_capped_grid(evg, env, kind, hidden, final_relu):
    """2 x EVG_QNET_GRAD_MAX_BLOCKS x 64 + 19 rows: every wavefront runs its loop twice whatever the device's grid, two take a third group, the last
    group holds 3 rows"""
    rows = cases.sweep_rows(evg._lib.QNET_GRAD_MAX_BLOCKS)
    params, x, gq = cases.case(kind, hidden, "integer", rows)
    want, _ = model.backward(x, params, final_relu, gq, exact=True)
    dp = _dev(env, params)
    got = _grads(_net(env, kind, dp, final_relu), dp, _dev(env, x), _dev(env, gq))
    assert all(cases.same_values(g, w) for g, w in zip(got, want)), [int((g != w).sum()) for g, w in zip(got, want)]


# ---------------------------------------------------------------------- random tier
WORST = {}


@pytest.mark.parametrize("final_relu", FINAL_RELU)
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_random_tier_stays_within_the_derived_bound(env, kind, hidden, family, final_relu):
    dp = None
    worst = 0.0
    for rows in (17, cases.RANDOM_ROWS):
        params, x, gq = cases.case(kind, hidden, family, rows)
        if dp is None:
            dp = _dev(env, params)
            net = _net(env, kind, dp, final_relu)
        want, bound = model.backward(x, params, final_relu, gq)
        got = _grads(net, dp, _dev(env, x), _dev(env, gq))
        for g, w, e in zip(got, want, bound):
            ok, ratio = cases.within_bound(g, w, e)
            worst = max(worst, ratio)
            assert ok, (rows, ratio)
        if cases.has_dead_unit(hidden):                          # a dead unit's gradient row is exactly zero
            assert not got[0][cases.DEAD_UNIT].any() and got[1][cases.DEAD_UNIT] == 0 and not got[2][:, cases.DEAD_UNIT].any()
    WORST[(kind, hidden, family, final_relu)] = worst
    print("%s %s %s final_relu=%d: worst |device - model| / E = %.4f (so far, all cases: %.4f)" % (kind, hidden, family, final_relu, worst, max(WORST.values())))


# ---------------------------------------------------------------------- properties
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("smart", (3, 64)), ("mini", (80,))], ids=["smart", "smart-3x64", "mini"])
def test_rows_without_an_upstream_gradient_add_exactly_nothing(env, kind, hidden):
    """Integer family (every order of the sums gives the same bits): with gq = 0 in all rows but every seventh, the gradients are those of the kept
    rows alone.  Dense family: zero rows at the end of the last group (the same grid, the same order of the sums) change no bit; gq = 0
    everywhere gives zeros."""
    params, x, gq = cases.case(kind, hidden, "integer", 259)
    dp = _dev(env, params)
    net = _net(env, kind, dp, False)
    keep = np.arange(259) % 7 == 3
    g0 = gq.copy()
    g0[~keep] = 0
    got = _grads(net, dp, _dev(env, x), _dev(env, g0))
    alone = _grads(net, dp, _dev(env, x[keep]), _dev(env, gq[keep]))
    assert all(np.array_equal(a, b) for a, b in zip(got, alone)) and any(a.any() for a in alone)
    params, x, gq = cases.case(kind, hidden, "dense", 259)
    dp = _dev(env, params)
    net = _net(env, kind, dp, False)
    g0 = gq.copy()
    g0[257:] = 0
    got = _grads(net, dp, _dev(env, x), _dev(env, g0))
    alone = _grads(net, dp, _dev(env, x[:257]), _dev(env, gq[:257]))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, alone))
    zero = _grads(net, dp, _dev(env, x), _dev(env, np.zeros_like(gq)))
    assert not any(z.any() for z in zero)


@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_clamp_is_numpy_clip_of_the_summed_gradients(env, kind, hidden):
    params, x, gq = cases.case(kind, hidden, "integer", 259)
    dp = _dev(env, params)
    net = _net(env, kind, dp, True)
    for clamp in (1.0, 2.5):
        want, _ = model.backward(x, params, True, gq, exact=True, clamp=clamp)
        raw, _ = model.backward(x, params, True, gq, exact=True)
        assert any((np.abs(r) > clamp).any() for r in raw) and any((np.abs(r) < clamp).any() for r in raw)
        got = _grads(net, dp, _dev(env, x), _dev(env, gq), clamp=clamp)
        assert all(cases.same_values(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("h2", cases.SENTINEL_HIDDEN)
@pytest.mark.parametrize("h1", cases.SENTINEL_HIDDEN)
def test_nothing_outside_the_linear_shapes_is_written(evg, env, h1, h2):
    """every gradient tensor sits inside a larger buffer filled with a sentinel, 16 bytes from its start: the sentinels before and after it are intact"""
    import torch
    _lib = evg._lib
    G = _lib.load_grad()
    for kind, hidden in (("smart", (h1, h2)), ("mini", (h1,))):
        if kind == "mini" and h2 != cases.SENTINEL_HIDDEN[0]:
            continue
        params = cases.params(kind, hidden, "dense")
        x, gq = cases.inputs(kind, hidden, "dense", 65)
        dp = _dev(env, params)
        net = _net(env, kind, dp, False)
        want = _grads(net, dp, _dev(env, x), _dev(env, gq))
        bufs = [torch.full((p.size + 4 + 256,), -7.5, dtype=torch.float32, device=env.device) for p in params]
        d = net._descriptor(1)
        gs = net._GRAD_STRUCT()
        gs.struct_size = C.sizeof(gs)
        for (name, _), b in zip(gs._fields_[2:], bufs):
            setattr(gs, name, b.data_ptr() + 16)
        ws = torch.empty(_lib.QNET_GRAD_MAX_BLOCKS * net._GRAD_PARTIAL, dtype=torch.float32, device=env.device)
        dx, dg = _dev(env, x), _dev(env, gq)
        rc = getattr(G, net._GRAD_ENTRY)(env._h, C.byref(d), 65, C.c_void_p(dx.data_ptr()), C.c_void_p(dg.data_ptr()), C.byref(gs),
                                         C.c_void_p(ws.data_ptr()), ws.numel() * 4, 0.0, env._stream())
        assert rc == 0, G.evg_last_error()
        for b, p, w in zip(bufs, params, want):
            b = b.cpu().numpy()
            assert (b[:4] == -7.5).all() and (b[4 + p.size:] == -7.5).all()
            assert np.array_equal(b[4:4 + p.size].reshape(p.shape).view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_two_calls_are_bit_equal_and_a_captured_call_replays(env, kind, hidden):
    import torch
    rows = 1024 + 3
    params = cases.params(kind, hidden, "dense")
    x, gq = cases.inputs(kind, hidden, "dense", rows)
    dp = _dev(env, params)
    net = _net(env, kind, dp, True)
    dx, dg = _dev(env, x), _dev(env, gq)
    first = _grads(net, dp, dx, dg)
    second = _grads(net, dp, dx, dg)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, second)) and any(a.any() for a in first)
    s = torch.cuda.Stream(env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(s):
        net._backward(dx, dp, dg, 0.0)                         # warm-up outside the capture (the workspace exists from here on)
    torch.cuda.current_stream(env.device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net._backward(dx, dp, dg, 0.0)
    for o in out:
        o.fill_(-7.0)
    g.replay()
    assert all(np.array_equal(o.cpu().numpy().view(np.uint32), a.view(np.uint32)) for o, a in zip(out, first))
    dg.mul_(2.0)                                               # the replay reads the tensors as they are now
    g.replay()
    want = _grads(net, dp, dx, dg)
    assert all(np.array_equal(o.cpu().numpy().view(np.uint32), a.view(np.uint32)) for o, a in zip(out, want))
    assert not np.array_equal(want[0], first[0])


# ---------------------------------------------------------------------- autograd
def _module(kind, hidden, params, final_relu):
    import torch
    sz = cases.sizes(kind, hidden)
    mods = []
    for i in range(len(sz) - 1):
        lin = torch.nn.Linear(sz[i], sz[i + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(params[2 * i]))
            lin.bias.copy_(torch.from_numpy(params[2 * i + 1]))
        mods += [lin, torch.nn.ReLU()]
    return torch.nn.Sequential(*(mods if final_relu else mods[:-1]))


@pytest.mark.parametrize("final_relu", FINAL_RELU)
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("smart", (3, 64)), ("mini", (80,)), ("mini", (1,))], ids=["smart", "smart-3x64", "mini", "mini-1"])
def test_with_grad_is_expanded_forward_and_fills_grad_through_a_loss(env, kind, hidden, final_relu):
    import torch
    import torch.nn.functional as F
    rows = 259
    params, x, _ = cases.case(kind, hidden, "gathered", rows)
    policy = _module(kind, hidden, params, final_relu).to(env.device)
    net = _net(env, kind, policy, None)
    assert net.final_relu == final_relu
    dx = _dev(env, x)
    rng = np.random.default_rng(7)
    action = torch.from_numpy(rng.integers(0, cases.OUT[kind], (rows, 1))).to(env.device)
    target = torch.from_numpy(rng.standard_normal((rows, 1)).astype(np.float32) * 2).to(env.device)
    q = net.with_grad(dx)
    assert q.requires_grad and tuple(q.shape) == (rows, cases.OUT[kind])
    assert np.array_equal(q.detach().cpu().numpy().view(np.uint32), net.expanded(dx).cpu().numpy().view(np.uint32))
    assert np.array_equal(q.detach().cpu().numpy(), (qnet_model if kind == "smart" else minimized_model).forward(x, params, final_relu))
    x3 = dx[:252].reshape(21, 12, 59)                          # leading dimensions are kept
    assert torch.equal(net.with_grad(x3).detach(), net.expanded(x3))
    predicted = q.gather(1, action)
    loss = F.smooth_l1_loss(predicted, target)
    loss.backward()
    # the upstream gradient that autograd sent down, recomputed on the host from the device's own Q: exact arithmetic on fp32 values, rounded once
    qh = q.detach().cpu().numpy().astype(np.float64)
    a, t = action.cpu().numpy()[:, 0], target.cpu().numpy().astype(np.float64)[:, 0]
    diff = qh[np.arange(rows), a] - t
    gq = np.zeros((rows, cases.OUT[kind]), np.float32)
    gq[np.arange(rows), a] = np.clip(diff.astype(np.float32), -1, 1) / np.float32(rows)
    want, bound = model.backward(x, params, final_relu, gq)
    # E for this gq, plus what the roundings of each gq entry in torch's own smooth-L1 backward (a subtraction, a scale by 1 / B: 3 roundings against
    # the host's) can move: 3 u M = E * 3 / c, and c >= B
    got = [p.grad.cpu().numpy() for p in policy.parameters()]
    worst = 0.0
    for g, w, e in zip(got, want, bound):
        ok, ratio = cases.within_bound(g, w, e * (1.0 + 3.0 / rows))
        worst = max(worst, ratio)
        assert ok, ratio
    print("%s %s final_relu=%d: worst |.grad - model| / tolerance = %.4f" % (kind, hidden, final_relu, worst))
    # a second backward accumulates: .grad doubles within 1 ulp
    F.smooth_l1_loss(net.with_grad(dx).gather(1, action), target).backward()
    for p, g in zip(policy.parameters(), got):
        twice = p.grad.cpu().numpy()
        assert (np.abs(twice.astype(np.float64) - 2.0 * g.astype(np.float64)) <= np.spacing(np.abs(twice))).all()
    # clamp= clamps this call's contribution
    for p in policy.parameters():
        p.grad = None
    F.smooth_l1_loss(net.with_grad(dx, clamp=1e-3).gather(1, action), target).backward()
    for p, g in zip(policy.parameters(), got):
        assert np.array_equal(p.grad.cpu().numpy(), np.clip(g, np.float32(-1e-3), np.float32(1e-3)))
    # the module's parameters are read at call time: an in-place update is followed
    with torch.no_grad():
        for p in policy.parameters():
            p.mul_(0.5)
    assert torch.equal(net.with_grad(dx).detach(), net.expanded(dx)) and not torch.equal(net.expanded(dx), q.detach())


def test_refusals_and_their_texts(evg, env):
    import torch
    _lib = evg._lib
    G = _lib.load_grad()
    for kind, hidden in (("smart", (60, 60)), ("mini", (80,))):
        params, x, gq = cases.case(kind, hidden, "dense", 37)
        dp = _dev(env, params)
        net = _net(env, kind, dp, False)
        dx, dg = _dev(env, x), _dev(env, gq)
        with pytest.raises(ValueError, match="not a pair"):
            _net(env, kind, (dp, dp), False).with_grad(dx)
        with pytest.raises(ValueError, match="must not require grad"):
            net.with_grad(dx.clone().requires_grad_())
        with pytest.raises(ValueError, match="fp32 chain"):
            _net(env, kind, dp, False, precision="bf16").with_grad(dx)
        with pytest.raises(ValueError, match=r"\[\.\.\., 59\]"):
            net.with_grad(dx[:, :58])
        for bad in (0, -1.0, float("inf"), float("nan"), "1"):
            with pytest.raises(ValueError, match="clamp"):
                net.with_grad(dx, clamp=bad)
        # the entry point's own refusals: EVG_ERR_INVALID, nothing launched
        outs = [torch.full(p.shape, 7.0, dtype=torch.float32, device=env.device) for p in dp]
        ws = torch.empty(_lib.QNET_GRAD_MAX_BLOCKS * net._GRAD_PARTIAL, dtype=torch.float32, device=env.device)

        def call(d=None, rows=37, xp=None, gp=None, grad=None, wsp=None, wsb=None, clamp=0.0, size=None):
            d = net._descriptor(1) if d is None else d
            gs = net._GRAD_STRUCT()
            gs.struct_size = C.sizeof(gs) if size is None else size
            for (name, _), o in zip(gs._fields_[2:], outs):
                setattr(gs, name, o.data_ptr())
            if grad is not None:
                setattr(gs, grad[0], grad[1])
            return getattr(G, net._GRAD_ENTRY)(env._h, C.byref(d), rows, C.c_void_p(dx.data_ptr() if xp is None else xp),
                                               C.c_void_p(dg.data_ptr() if gp is None else gp), C.byref(gs),
                                               C.c_void_p(ws.data_ptr() if wsp is None else wsp), ws.numel() * 4 if wsb is None else wsb, clamp, None)

        def refused(text, **kw):
            assert call(**kw) == -1, kw
            assert text in G.evg_last_error().decode(), (text, G.evg_last_error())

        d = net._descriptor(1)
        d.num_sets = 2
        refused("one network only", d=d)
        d = net._descriptor(1)
        d.h1 = 0
        refused("hidden size", d=d)
        d = net._descriptor(1)
        d.b1[0] = d.b1[0] + 4
        refused("16-byte aligned", d=d)
        refused("rows must lie in", rows=0)
        refused("16-byte aligned", xp=dx.data_ptr() + 4)
        refused("16-byte aligned", gp=dg.data_ptr() + 8)
        refused("struct_size", size=8)
        for name, _ in net._GRAD_STRUCT._fields_[2:]:
            refused("gradient pointer %s is NULL" % name, grad=(name, None))
            refused("gradient pointer %s must be 16-byte aligned" % name, grad=(name, outs[0].data_ptr() + 4))
        refused("workspace is NULL", wsp=0)
        refused("16-byte aligned", wsp=ws.data_ptr() + 4)
        refused("workspace is too small", wsb=4 * net._GRAD_PARTIAL - 4)
        refused("clamp must be finite", clamp=-1.0)
        refused("clamp must be finite", clamp=float("nan"))
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs)       # nothing was launched
        assert call(wsb=4 * net._GRAD_PARTIAL) == 0            # 37 rows are one workgroup: one partial is enough
        torch.cuda.synchronize()
        assert all(bool((o != 7.0).all()) for o in outs)       # every element was overwritten


def test_fp32_and_bf16_evaluators_are_unchanged_with_the_grad_library_loaded(evg, env):
    import learner_edge_cases as edge
    outs = {}
    for stage in ("before", "after"):
        for kind, hidden, host in (("smart", (60, 60), qnet_model), ("mini", (80,), minimized_model)):
            params, inputs = edge.case(kind, hidden, "signed", "compact")
            dp, di = _dev(env, params), _dev(env, inputs)
            got = _net(env, kind, dp, True)(di[0], di[1]).cpu().numpy()
            outs[(stage, kind, "fp32")] = got
            assert edge.same_values(got, host.forward_compact(inputs[0], inputs[1], params, True))
            outs[(stage, kind, "bf16")] = _net(env, kind, dp, True, precision="bf16")(di[0], di[1]).cpu().numpy()
        evg._lib.load_grad()
        params, x, gq = cases.case("smart", (60, 60), "dense", 65)
        dp = _dev(env, params)
        _grads(_net(env, "smart", dp, True), dp, _dev(env, x), _dev(env, gq))
    for kind in ("smart", "mini"):
        for precision in ("fp32", "bf16"):
            assert np.array_equal(outs[("before", kind, precision)].view(np.uint32), outs[("after", kind, precision)].view(np.uint32))


@pytest.mark.parametrize("example", ["smart_state_training.py", "minimized_training.py"])
def test_training_examples_run_with_the_device_backward(example):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", example), "256", "40", "256", "--device-backward"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "device backward" in out.stdout and "all finite: True" in out.stdout, out.stdout[-2000:]
