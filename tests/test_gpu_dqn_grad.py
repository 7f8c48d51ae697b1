"""GPU tests of evg_dqn_qnet_backward and DqnQNet.with_grad (include/evg_dqn_grad.h) against the host model of the contract (tests/dqn_grad_model.py):

  exact tier    the families of tests/dqn_grad_cases.py (integer, permutation, pow2dup): bit-equal gradients at rows in 1, 2, 3, 5, 15, 16, 17, 63, 65,
                259 and h1 in 1, 17, 47, 48, 49, 96, 527, 528 (every family at every h1 without the final ReLU; both final_relu values at h1 = 48 and
                528), the integer family past the delta kernel's 16-row form (4 165 rows; 65 536, the most a call takes), and over two sweeps of its capped
                grid plus 19 rows
  random tier   dense and gathered7 at 259 rows, h1 = 48 and 528: every element within the model's derived E
  properties    rows with gq = 0, the clamp, sentinels around the gradient tensors and the workspace, repeatability, a captured call
  autograd      with_grad's forward is rows(); the reference's own optimize_model step (tests/golden/dqn_grad.npz); a second backward accumulates
  neighbours    DqnQNet, dqn_get_action and the fp32 Smart_State evaluator with the new library loaded; examples/dqn_training.py --device-backward

Which case makes each loop take a second pass and a ragged last pass:
  delta kernel, chunk loop (48 hidden units)      h1 = 49: a second chunk of one unit; h1 = 96: a full second chunk; h1 = 527 / 528: eleven
  delta kernel, pass loop of the capped grid      the 16-row form's grid is its passes (one pass per workgroup: rows 17, 63, 65, 259 are 2 .. 17
                                                  workgroups, the last one ragged); the 64-row form runs at 4 165 rows (66 workgroups, a last pass
                                                  of 5 rows) and strides at 32 787 rows: 513 passes on 256 workgroups, the first takes a third
                                                  pass of 19 rows (one full wavefront, one of 3 rows, two empty); 65 536 rows are four full sweeps
  weight kernel, k-step loop (blocks of 32 rows)  rows 63, 65: a second and a third block, ragged; rows 259: three slices of 96, 96 and 67 rows
                                                  (the slices' reduction), three blocks each, the last one of 3 rows; 32 787 rows: 54 slices of 608; 65 536: 56 of 1 184
  weight kernel, tile dealing (4 per workgroup)   h1 = 17: two tiles, two idle wavefronts; h1 = 49: four; h1 = 96: six, a second workgroup with two;
                                                  h1 = 527 / 528: 33 tiles, nine workgroups, the last with one"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import dqn_grad_cases as cases
import dqn_grad_model as model
import dqn_model

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


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


def _grads(net, dev_params, x, gq, clamp=0.0):
    """the entry point itself: the gradients of dev_params for (x, gq) and the evaluator's own Q, as numpy"""
    q = net.rows(x).clone()
    return [g.cpu().numpy() for g in net._backward(x, q, dev_params, gq, clamp)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------- exact tier
EXACT = [(h1, f, False) for h1 in cases.HIDDEN for f in cases.EXACT_FAMILIES] + [(h1, f, True) for h1 in cases.BOTH_RELU_HIDDEN for f in cases.EXACT_FAMILIES]


@pytest.mark.parametrize("h1,family,final_relu", EXACT, ids=["%d-%s-%d" % c for c in EXACT])
def test_exact_tier_is_bit_equal_to_the_host_model(env, h1, family, final_relu):
    params, x, gq = cases.case(h1, family, cases.ROWS[-1])
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=final_relu)
    for rows in cases.ROWS:
        if family == "pow2dup":
            _, x, gq = cases.case(h1, family, rows)
        want, _ = model.backward(x[:rows], params, final_relu, gq[:rows], exact=True)
        got = _grads(net, dp, _dev(env, x[:rows]), _dev(env, gq[:rows]))
        differ = [int((g != w).sum()) for g, w in zip(got, want)]
        print("h1 %d %s final_relu=%d rows=%d: elements that differ %s, largest |gradient| %g" % (
            h1, family, final_relu, rows, differ, max(np.abs(w).max() for w in want)))
        assert all(cases.same_values(g, w) for g, w in zip(got, want)), (rows, differ)


@pytest.mark.parametrize("h1,rows,final_relu", [(528, 4096 + 64 + 5, False), (528, 4096 + 64 + 5, True), (96, 1 << 16, True)], ids=["528-4165-0", "528-4165-1", "96-65536-1"])
def test_exact_tier_in_the_64_row_form_of_the_delta_kernel(evg, env, h1, rows, final_relu):
    """EVG_DQN_GRAD_TINY_ROWS + 64 + 5 rows at h1 = 528: 66 workgroups of four 16-row wavefronts, the last pass holds 5 rows; 33 slices.
    EVG_DQN_GRAD_MAX_ROWS rows at h1 = 96: four full sweeps of the capped grid, EVG_DQN_GRAD_MAX_SLICES slices of 1 184 rows (the last of 416), the largest workspace
    offsets a call can have at this h1"""
    assert rows in (evg._lib.DQN_GRAD_TINY_ROWS + 64 + 5, evg._lib.DQN_GRAD_MAX_ROWS)
    params, x, gq = cases.case(h1, "integer", rows)
    want, _ = model.backward(x, params, final_relu, gq, exact=True)
    dp = _dev(env, params)
    got = _grads(env.dqn_qnet(dp, final_relu=final_relu), dp, _dev(env, x), _dev(env, gq))
    assert all(cases.same_values(g, w) for g, w in zip(got, want)), [int((g != w).sum()) for g, w in zip(got, want)]


@pytest.mark.parametrize("final_relu", [False, True])
def test_exact_tier_over_two_sweeps_of_the_capped_grid(evg, env, final_relu):
    """2 x EVG_DQN_GRAD_MAX_BLOCKS x 64 + 19 rows at h1 = 49 (two chunks): every workgroup of the delta kernel runs its pass loop twice, the first
    takes a third pass of 19 rows"""
    rows = cases.sweep_rows(evg._lib.DQN_GRAD_MAX_BLOCKS)
    params, x, gq = cases.case(cases.SWEEP_HIDDEN, "integer", rows)
    want, _ = model.backward(x, params, final_relu, gq, exact=True)
    dp = _dev(env, params)
    got = _grads(env.dqn_qnet(dp, final_relu=final_relu), dp, _dev(env, x), _dev(env, gq))
    assert all(cases.same_values(g, w) for g, w in zip(got, want)), [int((g != w).sum()) for g, w in zip(got, want)]


# ---------------------------------------------------------------------- random tier
WORST = {}


@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("h1", cases.RANDOM_HIDDEN)
def test_random_tier_stays_within_the_derived_bound(env, h1, family, final_relu):
    params, x, gq = cases.case(h1, family, cases.RANDOM_ROWS)
    dp = _dev(env, params)
    want, bound = model.backward(x, params, final_relu, gq)
    got = _grads(env.dqn_qnet(dp, final_relu=final_relu), dp, _dev(env, x), _dev(env, gq))
    worst = 0.0
    for g, w, e in zip(got, want, bound):
        ok, ratio = cases.within_bound(g, w, e)
        worst = max(worst, ratio)
        assert ok, ratio
    # a dead unit's gradient row is exactly zero
    assert not got[0][cases.DEAD_UNIT].any() and got[1][cases.DEAD_UNIT] == 0 and not got[2][:, cases.DEAD_UNIT].any()
    WORST[(h1, family, final_relu)] = worst
    print("h1 %d %s final_relu=%d: worst |device - model| / E = %.4f (so far, all cases: %.4f)" % (h1, family, final_relu, worst, max(WORST.values())))


# ---------------------------------------------------------------------- properties
@pytest.mark.parametrize("h1", [48, 528])
def test_rows_without_an_upstream_gradient_add_exactly_nothing(env, h1):
    """Integer family (every order of the sums gives the same bits): with gq = 0 in all rows but every seventh, the gradients are those of the kept
    rows alone.  Dense family: rows with gq = 0 at the end (the same rows, so the same slices and the same order of the sums) against the same call
    with those rows' x replaced: no bit changes; gq = 0 everywhere gives zeros."""
    params, x, gq = cases.case(h1, "integer", 259)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=False)
    keep = np.arange(259) % 7 == 3
    g0 = gq.copy()
    g0[~keep] = 0
    got = _grads(net, dp, _dev(env, x), _dev(env, g0))
    alone = _grads(net, dp, _dev(env, x[keep]), _dev(env, gq[keep]))
    assert all(np.array_equal(a, b) for a, b in zip(got, alone)) and any(a.any() for a in alone)
    params, x, gq = cases.case(h1, "dense", 259)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=False)
    g0 = gq.copy()
    g0[200:] = 0
    x0 = x.copy()
    x0[200:] = x[:59] * 3.0
    got = _grads(net, dp, _dev(env, x), _dev(env, g0))
    other = _grads(net, dp, _dev(env, x0), _dev(env, g0))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, other)) and any(a.any() for a in got)
    zero = _grads(net, dp, _dev(env, x), _dev(env, np.zeros_like(gq)))
    assert not any(z.any() for z in zero)


@pytest.mark.parametrize("rows", [65, 259])
def test_clamp_is_numpy_clip_of_the_summed_gradients(env, rows):
    """one slice (the weight kernel clamps at its store) and three (the reduction clamps)"""
    params, x, gq = cases.case(48, "integer", rows)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=True)
    raw, _ = model.backward(x, params, True, gq, exact=True)
    for clamp in (1.0, 2.5):
        assert any((np.abs(r) > clamp).any() for r in raw) and any((np.abs(r) < clamp).any() for r in raw)
        got = _grads(net, dp, _dev(env, x), _dev(env, gq), clamp=clamp)
        assert all(cases.same_values(g, np.clip(r, -clamp, clamp)) for g, r in zip(got, raw))
    params, x, gq = cases.case(48, "dense", rows)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=True)
    free = _grads(net, dp, _dev(env, x), _dev(env, gq))
    got = _grads(net, dp, _dev(env, x), _dev(env, gq), clamp=0.75)
    assert any((np.abs(f) > 0.75).any() for f in free)
    assert all(np.array_equal(g, np.clip(f, np.float32(-0.75), np.float32(0.75))) for g, f in zip(got, free))


@pytest.mark.parametrize("rows", [65, 259])
@pytest.mark.parametrize("h1", cases.SENTINEL_HIDDEN)
def test_nothing_outside_the_linear_shapes_and_the_workspace_is_written(evg, env, h1, rows):
    """every gradient tensor sits inside a larger buffer filled with a sentinel, 16 bytes from its start, and the workspace is followed by sentinels:
    the words before and after keep their bits"""
    import torch
    _lib = evg._lib
    G = _lib.load_dqn_grad()
    params = cases.params(h1, "dense")
    x, gq = cases.inputs(h1, "dense", rows)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=True)
    dx, dg = _dev(env, x), _dev(env, gq)
    want = _grads(net, dp, dx, dg)
    q = net.rows(dx).clone()
    bufs = [torch.full((p.size + 4 + 256,), -7.5, dtype=torch.float32, device=env.device) for p in params]
    d = _lib.EvgDqnNet()
    d.struct_size = C.sizeof(d)
    d.w1, d.b1, d.w2, d.b2 = (t.data_ptr() for t in dp)
    d.h1, d.final_relu = h1, 1
    gs = _lib.EvgDqnGrads()
    gs.struct_size = C.sizeof(gs)
    for (name, _), b in zip(gs._fields_[2:], bufs):
        setattr(gs, name, b.data_ptr() + 16)
    need = _lib.dqn_grad_workspace_bytes(rows, h1)
    ws = torch.full((need // 4 + 1024,), -7.5, dtype=torch.float32, device=env.device)
    rc = G.evg_dqn_qnet_backward(env._h, C.byref(d), rows, C.c_void_p(dx.data_ptr()), C.c_void_p(q.data_ptr()), C.c_void_p(dg.data_ptr()), C.byref(gs),
                                 C.c_void_p(ws.data_ptr()), need, 0.0, env._stream())
    assert rc == 0, G.evg_last_error()
    assert bool((ws[need // 4:] == -7.5).all())
    for b, p, w in zip(bufs, params, want):
        b = b.cpu().numpy()
        assert (b[:4] == -7.5).all() and (b[4 + p.size:] == -7.5).all()
        assert np.array_equal(_bits(b[4:4 + p.size].reshape(p.shape)), _bits(w))


def test_two_calls_are_bit_equal_and_a_captured_call_replays(env):
    import torch
    rows, h1 = 1024 + 3, 528
    params = cases.params(h1, "dense")
    x, gq = cases.inputs(h1, "dense", rows)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=True)
    dx, dg = _dev(env, x), _dev(env, gq)
    q = net.rows(dx).clone()
    first = _grads(net, dp, dx, dg)
    second = _grads(net, dp, dx, dg)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, second)) and any(a.any() for a in first)
    s = torch.cuda.Stream(env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(s):
        net._backward(dx, q, dp, dg, 0.0)                      # warm-up outside the capture (the workspace exists from here on)
    torch.cuda.current_stream(env.device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.rows(dx, out=q)
        out = net._backward(dx, q, dp, dg, 0.0)
    for o in out:
        o.fill_(-7.0)
    g.replay()
    assert all(np.array_equal(_bits(o.cpu().numpy()), _bits(a)) for o, a in zip(out, first))
    with torch.no_grad():                                      # a parameter update is followed: the replay reads the tensors as they are now
        for p in dp:
            p.mul_(0.5)
    g.replay()
    want = _grads(net, dp, dx, dg)
    assert all(np.array_equal(_bits(o.cpu().numpy()), _bits(a)) for o, a in zip(out, want))
    assert not np.array_equal(want[0], first[0])


# ---------------------------------------------------------------------- autograd
def _module(params, final_relu):
    import torch
    mods = []
    for i in range(2):
        lin = torch.nn.Linear(params[2 * i].shape[1], params[2 * i].shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(params[2 * i]))
            lin.bias.copy_(torch.from_numpy(params[2 * i + 1]))
        mods += [lin, torch.nn.ReLU()]
    return torch.nn.Sequential(*(mods if final_relu else mods[:-1]))


@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("h1", [47, 528])
def test_with_grad_is_rows_bit_for_bit(env, h1, final_relu):
    import torch
    rows = 259
    params, x, _ = cases.case(h1, "gathered7", rows)
    policy = _module(params, final_relu).to(env.device)
    net = env.dqn_qnet(policy)
    assert net.final_relu == final_relu
    dx = _dev(env, x)
    q = net.with_grad(dx)
    assert q.requires_grad and tuple(q.shape) == (rows, 132)
    assert np.array_equal(_bits(q.detach().cpu().numpy()), _bits(net.rows(dx).cpu().numpy()))
    assert np.array_equal(q.detach().cpu().numpy(), dqn_model.forward(x, params, final_relu))
    x3 = dx[:252].reshape(21, 12, 105)                         # leading dimensions are kept
    q3 = net.with_grad(x3)
    assert tuple(q3.shape) == (21, 12, 132) and torch.equal(q3.detach().reshape(252, 132), net.rows(dx[:252]))
    with torch.no_grad():                                      # the module's parameters are read at call time: an in-place update is followed
        for p in policy.parameters():
            p.mul_(0.5)
    assert torch.equal(net.with_grad(dx).detach(), net.rows(dx)) and not torch.equal(net.rows(dx), q.detach())


def test_the_reference_optimize_model_step_through_with_grad(env):
    """tests/golden/dqn_grad.npz: the reference's own QNetwork(fc1_unit=48) and DQNAgent.optimize_model on 64 rows.  .grad through with_grad and the
    fixture's loss lies within E (1 + 3 / rows) + E of the fixture's: both are fp32 sums of the same terms (each within E of the float64 model, whose
    masks are the fixture's by construction), and the roundings of each gq entry in torch's smooth-L1 backward can move 3 u M = E * 3 / c, c >= rows."""
    import torch
    import torch.nn.functional as F
    fx = np.load(os.path.join(ROOT, "tests", "golden", "dqn_grad.npz"))
    names = ("w1", "b1", "w2", "b2")
    params = tuple(fx[n] for n in names)
    rows = fx["x"].shape[0]
    policy = _module(params, True).to(env.device)
    net = env.dqn_qnet(policy)
    dx, action, expected = _dev(env, fx["x"]), _dev(env, fx["action"]), _dev(env, fx["expected"])

    def step(clamp=None):
        q = net.with_grad(dx, clamp=clamp)
        loss = F.smooth_l1_loss(q.gather(1, action), expected)
        loss.backward()
        return q, loss

    q, loss = step()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-5 * abs(float(fx["loss"]))
    # the upstream gradient that autograd sent down, recomputed on the host from the device's own Q; repeated columns add
    qh = q.detach().cpu().numpy().astype(np.float64)
    diff = np.take_along_axis(qh, fx["action"], 1) - fx["expected"].astype(np.float64)
    gq = np.zeros((rows, 132), np.float64)
    np.add.at(gq, (np.arange(rows)[:, None], fx["action"]), np.clip(diff, -1, 1) / (7.0 * rows))
    _, bound = model.backward(fx["x"], params, True, gq.astype(np.float32))
    got = [p.grad.cpu().numpy() for p in policy.parameters()]
    worst = 0.0
    for g, n, e in zip(got, names, bound):
        ok, ratio = cases.within_bound(g, fx["g_" + n], e * (1.0 + 3.0 / rows) + e)
        worst = max(worst, ratio)
        assert ok, (n, ratio)
    print("worst |.grad - fixture| / tolerance = %.4f" % worst)
    # a second backward accumulates: .grad doubles within 1 ulp
    step()
    for p, g in zip(policy.parameters(), got):
        twice = p.grad.cpu().numpy()
        assert (np.abs(twice.astype(np.float64) - 2.0 * g.astype(np.float64)) <= np.spacing(np.abs(twice))).all()
    # the clamped form is np.clip of this call's contribution, and lies as close to the fixture's clamped gradients
    for p in policy.parameters():
        p.grad = None
    step(clamp=1.0)
    assert any((np.abs(g) > 1).any() for g in got)
    for p, g, n, e in zip(policy.parameters(), got, names, bound):
        assert np.array_equal(p.grad.cpu().numpy(), np.clip(g, np.float32(-1), np.float32(1)))
        assert cases.within_bound(p.grad.cpu().numpy(), fx["c_" + n], e * (1.0 + 3.0 / rows) + e)[0]


def test_refusals_and_their_texts(evg, env):
    import torch
    _lib = evg._lib
    G = _lib.load_dqn_grad()
    h1, rows = 48, 37
    params, x, gq = cases.case(h1, "dense", rows)
    dp = _dev(env, params)
    net = env.dqn_qnet(dp, final_relu=True)
    dx, dg = _dev(env, x), _dev(env, gq)
    q = net.rows(dx).clone()
    with pytest.raises(ValueError, match="must not require grad"):
        net.with_grad(dx.clone().requires_grad_())
    with pytest.raises(ValueError, match=r"\[\.\.\., 105\]"):
        net.with_grad(dx[:, :104])
    with pytest.raises(ValueError, match="float32"):
        net.with_grad(dx.double())
    with pytest.raises(ValueError):
        net.with_grad(dx.cpu())
    with pytest.raises(ValueError, match="rows"):
        net.with_grad(torch.zeros((_lib.DQN_GRAD_MAX_ROWS + 1, 105), device=env.device))
    for bad in (0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="clamp"):
            net.with_grad(dx, clamp=bad)
    outs = [torch.full(p.shape, 7.0, dtype=torch.float32, device=env.device) for p in dp]
    need = _lib.dqn_grad_workspace_bytes(rows, h1)
    ws = torch.empty(need // 4, dtype=torch.float32, device=env.device)

    def descriptor():
        d = _lib.EvgDqnNet()
        d.struct_size = C.sizeof(d)
        d.w1, d.b1, d.w2, d.b2 = (t.data_ptr() for t in dp)
        d.h1, d.final_relu = h1, 1
        return d

    def call(d=None, rows=rows, xp=None, qp=None, gp=None, grad=None, wsp=None, wsb=None, clamp=0.0, size=None, handle=None, nogs=False):
        d = descriptor() if d is None else d
        gs = _lib.EvgDqnGrads()
        gs.struct_size = C.sizeof(gs) if size is None else size
        for (name, _), o in zip(gs._fields_[2:], outs):
            setattr(gs, name, o.data_ptr())
        if grad is not None:
            setattr(gs, grad[0], grad[1])
        return G.evg_dqn_qnet_backward(env._h if handle is None else handle, C.byref(d) if d != 0 else None, rows,
                                       C.c_void_p(dx.data_ptr() if xp is None else xp), C.c_void_p(q.data_ptr() if qp is None else qp),
                                       C.c_void_p(dg.data_ptr() if gp is None else gp), None if nogs else C.byref(gs),
                                       C.c_void_p(ws.data_ptr() if wsp is None else wsp), need if wsb is None else wsb, clamp, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in G.evg_last_error().decode(), (text, G.evg_last_error())

    refused("null handle or network descriptor", handle=0)
    refused("null handle or network descriptor", d=0)
    d = descriptor()
    d.struct_size = 40
    refused("sizeof(evg_dqn_net)", d=d)
    for bad in (0, 529):
        d = descriptor()
        d.h1 = bad
        refused("hidden size", d=d)
    d = descriptor()
    d.final_relu = 2
    refused("final_relu must be 0 or 1", d=d)
    d = descriptor()
    d.b1 = d.b1 + 4
    refused("b1 must be 16-byte aligned", d=d)
    d = descriptor()
    d.w2 = None
    refused("w2 is NULL", d=d)
    refused("rows must lie in", rows=0)
    refused("rows must lie in", rows=_lib.DQN_GRAD_MAX_ROWS + 1)
    refused("x is NULL", xp=0)
    refused("x must be 16-byte aligned", xp=dx.data_ptr() + 4)
    refused("gq is NULL", gp=0)
    refused("gq must be 16-byte aligned", gp=dg.data_ptr() + 8)
    refused("q is required with final_relu", qp=0)
    refused("q must be 16-byte aligned", qp=q.data_ptr() + 4)
    refused("null gradient descriptor", nogs=True)
    refused("sizeof(evg_dqn_grads)", size=8)
    for name, _ in _lib.EvgDqnGrads._fields_[2:]:
        refused("the gradient pointer %s is NULL" % name, grad=(name, None))
        refused("the gradient pointer %s must be 16-byte aligned" % name, grad=(name, outs[0].data_ptr() + 4))
    refused("the workspace is NULL", wsp=0)
    refused("the workspace must be 16-byte aligned", wsp=ws.data_ptr() + 4)
    refused("the workspace is too small", wsb=need - 4)
    refused("clamp must be finite", clamp=-1.0)
    refused("clamp must be finite", clamp=float("nan"))
    refused("clamp must be finite", clamp=float("inf"))
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)           # nothing was launched
    d = descriptor()
    d.final_relu = 0
    assert call(d=d, qp=0) == 0                                # q may be NULL without the final ReLU
    torch.cuda.synchronize()
    want = _grads(env.dqn_qnet(dp, final_relu=False), dp, dx, dg)
    assert all(np.array_equal(_bits(o.cpu().numpy()), _bits(w)) for o, w in zip(outs, want))


def test_neighbours_are_unchanged_with_the_grad_library_loaded(evg, env):
    """DqnQNet, dqn_get_action and the fp32 Smart_State evaluator return the same bits before and after libevg_dqngrad.so is loaded and has run"""
    import torch
    import qnet_grad_cases as small
    outs = {}
    params, x, gq = cases.case(528, "dense", 259)
    dp, dx = _dev(env, params), _dev(env, x)
    sp, sx, _ = small.case("smart", (60, 60), "dense", 65)
    dsp, dsx = _dev(env, sp), _dev(env, sx)
    for stage in ("before", "after"):
        net = env.dqn_qnet(dp, final_relu=True)
        outs[(stage, "q")] = net.rows(dx).cpu().numpy()
        qn = net.rows(_dev(env, x[:64])).clone()
        explored = torch.zeros(64, dtype=torch.uint8, device=env.device)
        outs[(stage, "rows")] = env.dqn_get_action(qn, 0.3, seat=0, explored=explored).cpu().numpy().copy()
        outs[(stage, "explored")] = explored.cpu().numpy()
        outs[(stage, "smart")] = env.smart_qnet(dsp, final_relu=True).expanded(dsx).cpu().numpy()
        evg._lib.load_dqn_grad()
        _grads(net, dp, dx, _dev(env, gq))
    assert np.array_equal(outs[("before", "q")], dqn_model.forward(x, params, True))
    for k in ("q", "smart"):
        assert np.array_equal(_bits(outs[("before", k)]), _bits(outs[("after", k)]))
    for k in ("rows", "explored"):
        assert np.array_equal(outs[("before", k)], outs[("after", k)])


def test_training_example_runs_with_the_device_backward():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dqn_training.py"), "256", "60", "128", "--device-backward"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "device backward" in out.stdout and "all finite: True" in out.stdout, out.stdout[-2000:]
