"""GPU tests of evg_smart_qnet (EvergladesVecEnv.smart_qnet / everglades_amd.SmartQNet): the Smart_State Q network's forward pass in one launch.  The
contract is the host model's fmaf chain (tests/qnet_model.py) bit for bit -- on the reference's networks (tests/golden/smart_qnet.npz), on live games,
in the compact, two-seat and expanded layouts -- and the reference's forward within the CPU test's tolerance."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from qnet_model import expand, forward, forward_compact

pytestmark = pytest.mark.gpu

NETS = ["a", "b", "c"]
RTOL, ATOL = 1e-5, 1e-5            # as tests/test_qnet_host.py: the reference's torch forward does not add in the chain's order


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


def _np(t):
    return t.detach().cpu().numpy()


def _golden_params(d, v):
    return tuple(d[v + "_" + k] for k in ("w1", "b1", "w2", "b2", "w3", "b3"))


def _dev(torch, params, device):
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in params)


def _random_params(h1, h2, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    shapes = [(h1, 59), (h1,), (h2, h1), (h2,), (5, h2), (5,)]
    return tuple((rng.standard_normal(s) * scale).astype(np.float32) for s in shapes)


def _fixture_features():
    x = load_golden("smart_state.npz")["features"].astype(np.float32).reshape(-1, 12, 59)       # [204, 12, 59]
    return x, np.ascontiguousarray(x[:, 0, :34]), np.ascontiguousarray(x[:, :, 34:47])


@pytest.mark.parametrize("v", NETS)
@pytest.mark.parametrize("final_relu", [True, False])
def test_kernel_equals_host_model_on_the_fixture(evg, env, v, final_relu):
    import torch
    d = load_golden("smart_qnet.npz")
    p = _golden_params(d, v)
    x, shared, swarm = _fixture_features()
    qn = env.smart_qnet(_dev(torch, p, env.device), final_relu=final_relu)
    want = forward(x, p, final_relu)
    got_c = _np(qn(torch.from_numpy(shared).to(env.device), torch.from_numpy(swarm).to(env.device)))
    got_x = _np(qn.expanded(torch.from_numpy(x).to(env.device)))
    assert np.array_equal(got_c, want) and np.array_equal(got_x, want)
    assert np.array_equal(forward_compact(shared, swarm, p, final_relu), want)
    if final_relu:
        np.testing.assert_allclose(got_x, d[v + "_q"].reshape(-1, 12, 5), rtol=RTOL, atol=ATOL)


def test_reference_qnetwork_module_is_read_in_place(evg, env):
    """A module with fc1/fc2/fc3 (the reference's QNetwork's attributes) is bound with the final ReLU on."""
    import torch

    class QNetwork(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc3 = torch.nn.Linear(59, 60), torch.nn.Linear(60, 60), torch.nn.Linear(60, 5)

    d = load_golden("smart_qnet.npz")
    net = QNetwork().to(env.device)
    with torch.no_grad():
        for (lin, k) in ((net.fc1, "1"), (net.fc2, "2"), (net.fc3, "3")):
            lin.weight.copy_(torch.from_numpy(d["a_w" + k]))
            lin.bias.copy_(torch.from_numpy(d["a_b" + k]))
    x, _, _ = _fixture_features()
    qn = env.smart_qnet(net)
    assert qn.final_relu is True
    got = _np(qn.expanded(torch.from_numpy(x).to(env.device)))
    assert np.array_equal(got, forward(x, _golden_params(d, "a"), True))
    np.testing.assert_allclose(got, d["a_q"].reshape(-1, 12, 5), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("h1,h2", [(1, 1), (17, 60), (60, 17), (64, 64), (60, 60), (1, 64)])
def test_hidden_sizes(evg, env, h1, h2):
    import torch
    p = _random_params(h1, h2, 100 * h1 + h2)
    x, shared, swarm = _fixture_features()
    for final_relu in (False, True):
        qn = env.smart_qnet(_dev(torch, p, env.device), final_relu=final_relu)
        want = forward(x, p, final_relu)
        assert np.array_equal(_np(qn(torch.from_numpy(shared).to(env.device), torch.from_numpy(swarm).to(env.device))), want), (h1, h2)
        assert np.array_equal(_np(qn.expanded(torch.from_numpy(x).to(env.device))), want), (h1, h2)


def test_two_seat_launch_equals_two_one_set_launches_and_batch_invariance(evg, env):
    import torch
    dev = env.device
    pa, pb = _dev(torch, _random_params(60, 60, 1), dev), _dev(torch, _random_params(60, 60, 2), dev)
    g = torch.Generator(device="cpu").manual_seed(11)
    N = 1000
    shared = torch.rand((N, 2, 34), generator=g).to(dev)
    swarm = torch.rand((N, 2, 12, 13), generator=g).to(dev)
    both = _np(env.smart_qnet((pa, pb), final_relu=False)(shared, swarm))
    assert both.shape == (N, 2, 12, 5)
    for p, pp in enumerate((pa, pb)):
        one = env.smart_qnet(pp, final_relu=False)
        assert np.array_equal(both[:, p], _np(one(shared[:, p].contiguous(), swarm[:, p].contiguous())))
    same = _np(env.smart_qnet(pa, final_relu=False)(shared, swarm))          # one network on both seats
    assert np.array_equal(same[:, 0], both[:, 0])
    # the same rows at other offsets and in other batch sizes give the same bits
    one = env.smart_qnet(pa, final_relu=False)
    s0, w0 = shared[:, 0].contiguous(), swarm[:, 0].contiguous()
    full = _np(one(s0, w0))
    for lo, hi in ((0, 1), (3, 20), (16, 17), (500, 1000), (999, 1000), (4, 1000)):
        assert np.array_equal(_np(one(s0[lo:hi].clone(), w0[lo:hi].clone())), full[lo:hi]), (lo, hi)     # fresh (aligned) copies
    x = env.expand_smart_state(s0, w0).contiguous()
    fx = _np(one.expanded(x.reshape(-1, 59)))
    assert np.array_equal(fx.reshape(N, 12, 5), full)
    for lo, hi in ((0, 1), (5, 77), (11999 - 16, 11999)):
        assert np.array_equal(_np(one.expanded(x.reshape(-1, 59)[lo:hi].clone())), fx[lo:hi]), (lo, hi)


def _live_features(evg, N, turns, seed):
    """The compact features of a step_vs_q loop (random Q) after `turns` turns, and the expanded features of the same observation."""
    import torch
    env = evg.EvergladesVecEnv(N, seed=seed, auto_reset=True)
    env.reset()
    obs = env.observe_seat(0)
    shared, swarm = env.smart_state_compact(-1, obs)
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(turns):
        q = torch.randn((N, 12, 5), generator=g).to(env.device)
        obs, _, _, _ = env.step_vs_q("swarm_agent", q, 0.2, seat=0, features=(shared, swarm))
    x = env.smart_state(0, obs)                                          # the seat observation the step returned
    return env, shared, swarm, x


@pytest.mark.parametrize("N,check", [(4096, None), (65536, 2048)])
def test_live_games_against_host_model_and_torch(evg, N, check):
    import torch
    env, shared, swarm, x = _live_features(evg, N, 5, 17 + N)
    d = load_golden("smart_qnet.npz")
    p = _golden_params(d, "a")
    qn = env.smart_qnet(_dev(torch, p, env.device), final_relu=True)
    q = qn(shared, swarm)
    qx = qn.expanded(x)
    assert torch.equal(q, qx)                                            # compact == expanded on the same observations
    rows = np.arange(N) if check is None else np.sort(np.random.default_rng(3).choice(N, check, replace=False))
    want = forward_compact(_np(shared)[rows], _np(swarm)[rows], p, True)
    assert np.array_equal(_np(q)[rows], want)
    net = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5),
                              torch.nn.ReLU()).to(env.device)
    with torch.no_grad():
        for i, k in ((0, "1"), (2, "2"), (4, "3")):
            net[i].weight.copy_(torch.from_numpy(d["a_w" + k]))
            net[i].bias.copy_(torch.from_numpy(d["a_b" + k]))
        ref = net(x)
    np.testing.assert_allclose(_np(q), _np(ref), rtol=RTOL, atol=ATOL)
    env.close()


def test_in_place_updates_and_replaced_parameters_are_seen(evg, env):
    import torch
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5)).to(env.device)
    qn = env.smart_qnet(net)
    assert qn.final_relu is False
    x, shared, swarm = _fixture_features()
    xd = torch.from_numpy(x).to(env.device)
    params = lambda: tuple(_np(t) for t in (net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias))  # noqa: E731
    before = _np(qn.expanded(xd))
    assert np.array_equal(before, forward(x, params(), False))
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    net(xd).square().mean().backward()
    opt.step()
    after = _np(qn.expanded(xd))
    assert not np.array_equal(after, before) and np.array_equal(after, forward(x, params(), False))
    other = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5)).to(env.device)
    net.load_state_dict(other.state_dict())
    assert np.array_equal(_np(qn.expanded(xd)), forward(x, params(), False))
    net[2].weight = torch.nn.Parameter(torch.randn(60, 60, device=env.device) * 0.1)      # replaced, not updated in place
    assert np.array_equal(_np(qn.expanded(xd)), forward(x, params(), False))


def test_refusals_leave_out_untouched(evg, env):
    import ctypes as C
    import torch
    from everglades_amd import _lib
    dev = env.device
    p = _dev(torch, _random_params(60, 60, 9), dev)
    N = 64
    shared, swarm = torch.rand((N, 34), device=dev), torch.rand((N, 12, 13), device=dev)
    out = torch.full((N, 12, 5), 7.0, device=dev)
    qn = env.smart_qnet(p, final_relu=False)
    big = torch.zeros(N * 34 + 4, device=dev)
    bad_calls = [
        lambda: qn(shared[:, :33].contiguous(), swarm, out=out),
        lambda: qn(shared.double(), swarm, out=out),
        lambda: qn(shared.cpu(), swarm, out=out),
        lambda: qn(shared.t().contiguous().t(), swarm, out=out),
        lambda: qn(big[1:1 + N * 34].view(N, 34), swarm, out=out),
        lambda: qn(shared, swarm, out=out[:, :, :4]),
        lambda: qn(shared[:0], swarm[:0], out=out[:0]),
        lambda: qn.expanded(torch.rand((N, 58), device=dev), out=out[:, 0]),
        lambda: env.smart_qnet((p[0][:, :58].contiguous(),) + p[1:], final_relu=False)(shared, swarm, out=out),
        lambda: env.smart_qnet(_dev(torch, _random_params(65, 60, 1), dev), final_relu=False)(shared, swarm, out=out),
        lambda: env.smart_qnet(p)(shared, swarm, out=out),                                   # a tuple needs final_relu
        lambda: env.smart_qnet((p, p), final_relu=False)(shared, swarm, out=out),             # a pair needs [N, 2, ...]
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises((ValueError, evg.EvgError)):
            call()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), i
    # the C entry point itself: every bad argument is refused and nothing is launched
    L = env.L

    def desc(**kw):
        d = _lib.EvgQnet()
        d.struct_size, d.h1, d.h2, d.final_relu, d.num_sets = C.sizeof(_lib.EvgQnet), 60, 60, 0, 1
        for i, k in enumerate(("w1", "b1", "w2", "b2", "w3", "b3")):
            getattr(d, k)[0] = p[i].data_ptr()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[0] = v[0]
            else:
                setattr(d, k, v)
        return d

    def call(d, layout=_lib.QNET_COMPACT, rows=N, in0=shared.data_ptr(), in1=swarm.data_ptr(), q=out.data_ptr()):
        return L.evg_smart_qnet(env._h, C.byref(d) if d is not None else None, layout, rows, C.c_void_p(in0), C.c_void_p(in1), C.c_void_p(q), None)

    assert call(desc()) == 0
    torch.cuda.synchronize()
    good = out.clone()
    out.fill_(7.0)
    for d, kw in [(desc(struct_size=8), {}), (desc(h1=0), {}), (desc(h2=65), {}), (desc(final_relu=2), {}), (desc(num_sets=2), {}),
                  (desc(w2=(0,)), {}), (desc(b3=(p[5].data_ptr() + 4,)), {}), (None, {}), (desc(), {"layout": 3}),
                  (desc(), {"layout": _lib.QNET_COMPACT_SEATS}), (desc(), {"rows": 0}), (desc(), {"rows": (1 << 30) + 1}),
                  (desc(), {"in0": 0}), (desc(), {"in1": 0}), (desc(), {"q": 0}), (desc(), {"in0": shared.data_ptr() + 4}),
                  (desc(), {"q": out.data_ptr() + 8})]:
        assert call(d, **kw) == -1, kw                   # EVG_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert bool(torch.isfinite(good).all())


def test_captured_turn_equals_eager_turns(evg):
    import torch
    N, turns = 4096, 6
    p = _random_params(60, 60, 21, scale=0.2)

    def run(capture):
        env = evg.EvergladesVecEnv(N, seed=33, auto_reset=True)
        env.reset()
        shared, swarm = env.smart_state_compact(-1, env.observe_seat(0))
        qn = env.smart_qnet(_dev(torch, p, env.device), final_relu=False)
        q = torch.empty((N, 12, 5), device=env.device)
        out = torch.empty((N, 105), dtype=env.obs_dtype, device=env.device)

        def turn():
            qn(shared, swarm, out=q)
            env.step_vs_q("swarm_agent", q, 0.0, seat=0, features=(shared, swarm), out=out)

        qs = []
        if capture:
            s = torch.cuda.Stream(env.device)
            s.wait_stream(torch.cuda.current_stream(env.device))
            with torch.cuda.stream(s):
                turn()                                        # warm-up outside the capture
            torch.cuda.current_stream(env.device).wait_stream(s)
            qs.append(q.clone())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                turn()
            for _ in range(turns - 1):
                g.replay()
                qs.append(q.clone())
        else:
            for _ in range(turns):
                turn()
                qs.append(q.clone())
        torch.cuda.synchronize()
        res = [_np(t) for t in qs] + [_np(shared), _np(swarm), _np(out)]
        env.close()
        return res

    eager, graphed = run(False), run(True)
    for a, b in zip(eager, graphed):
        assert np.array_equal(a, b)


def _example(name):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    return __import__(name)


def test_examples_run_with_device_net(evg):
    import torch
    st = _example("smart_state_loop").main(2048, 20, 0.1, fused=True, device_net=True)
    assert int(st["totals"][0]) >= 0
    _example("smart_state_loop").main(1024, 10, 0.1, fused=False, device_net=True)
    _example("smart_state_self_play").main(2048, 20, fused=True, device_net=True)
    _example("smart_state_self_play").main(1024, 10, fused=False, device_net=True)
    losses = _example("smart_state_training").main(2048, 40, 256, device_net=True)
    assert len(losses) > 30 and bool(torch.isfinite(losses).all())


def test_loop_example_device_net_gives_the_torch_networks_games(evg):
    """The stand-in network through the kernel plays the same games as through torch whenever the two Q tensors decode alike; at least the Q of the
    first turn is within tolerance of the torch forward."""
    import torch
    loop = _example("smart_state_loop")
    env = evg.EvergladesVecEnv(512, seed=3, auto_reset=True)
    env.reset()
    shared, swarm = env.smart_state_compact(-1, env.observe_seat(0))
    net = loop.make_network(env.device)
    qn = env.smart_qnet(net.params, final_relu=False)
    np.testing.assert_allclose(_np(qn(shared, swarm)), _np(net(shared, swarm)), rtol=1e-4, atol=1e-5)
    want = forward_compact(_np(shared), _np(swarm), tuple(_np(t) for t in net.params), False)
    assert np.array_equal(_np(qn(shared, swarm)), want)
    assert np.array_equal(expand(_np(shared), _np(swarm)), _np(env.expand_smart_state(shared, swarm)))
    env.close()
