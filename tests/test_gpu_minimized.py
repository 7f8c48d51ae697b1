"""GPU tests of the Minimized agents' device path: evg_minimized_get_action, the 11-way head of step_vs_q (evg_step_vs_policy_minimized_q /
evg_step_vs_league_minimized_q), evg_minimized_qnet (EvergladesVecEnv.minimized_qnet / everglades_amd.MinimizedQNet) and the replay memory fed with the
agent's rows.  References: the host model (tests/minimized_model.py, pinned to the reference's own methods by tests/golden/minimized_*.npz on the CPU),
the fixtures themselves, and -- for the fused forms -- the two-launch composition minimized_get_action + step_vs."""
import ctypes as C

import numpy as np
import pytest

import minimized_model as mm
from conftest import load_golden
from replay_model import ReplayModel

gpu = pytest.mark.gpu
LEAGUE15 = ["random_actions_delay", "random_actions", "bull_rush", "all_cycle", "base_rush_v1", "cycle_rush_turn25", "cycle_rush_turn50",
            "cycle_target_node", "cycle_target_node1", "cycle_target_node11", "cycle_target_node11P2", "random_actions_2", "same_commands_2",
            "same_commands", "swarm_agent"]


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _q(torch, shape, gen, dev):
    """values on a grid of halves: exact ties within a swarm and between swarms are common"""
    return (torch.randn(shape, generator=gen) * 2.0).round().div(2.0).to(dev)


# ---------------------------------------------------------------------------------------------- evg_minimized_get_action
@gpu
@pytest.mark.parametrize("seat", [0, 1])
def test_get_action_equals_the_model_and_the_fixture(evg, seat):
    """N = 37: one full wavefront of the per-env draws and a 5-env tail, the last decode row group partial.  Rows m of the fixture become envs m of three
    handles (the fixture's agent of row m is env id m, episode m % 3, turn obs[0]: the handles' state is set to that)."""
    import torch
    g = load_golden("minimized_actions.npz")
    N, seed = 37, int(g["seed"][0])
    for lo in (0, 37, 65):
        sl = slice(lo, lo + N)
        env = evg.EvergladesVecEnv(N, seed=seed, env_id_base=lo, auto_reset=False)
        env.reset()
        st = env.get_state()
        st["env"][:, 0] = g["obs"][sl, seat, 0]
        st["env"][:, 2] = g["episode"][sl]
        env.set_state(st["groups"], st["nodes"], st["health"], st["env"])
        q = torch.as_tensor(g["q"][sl, seat]).to(env.device).contiguous()
        eps = g["eps"][sl, seat]
        want, want_x = mm.get_action(g["q"][sl, seat], seed, np.arange(lo, lo + N), g["episode"][sl], g["obs"][sl, seat, 0], seat, eps)
        assert np.array_equal(want, g["actions"][sl, seat]) and np.array_equal(want_x, g["explored"][sl, seat])
        x = torch.full((N,), 7, dtype=torch.uint8, device=env.device)
        out = torch.full((N, 7, 2), -1, dtype=torch.int32, device=env.device)
        rows = env.minimized_get_action(q, torch.as_tensor(eps).to(env.device), seat=seat, out=out, explored=x)      # per-env epsilon
        assert np.array_equal(rows.cpu().numpy(), want) and np.array_equal(x.cpu().numpy(), want_x)
        for level in (0.0, 0.3, 1.0):                                                                                # scalar epsilon
            w, wx = mm.get_action(g["q"][sl, seat], seed, np.arange(lo, lo + N), g["episode"][sl], g["obs"][sl, seat, 0], seat, np.full(N, level, np.float32))
            x.fill_(7)
            rows = env.minimized_get_action(q, level, seat=seat, explored=x)
            assert np.array_equal(rows.cpu().numpy(), w) and np.array_equal(x.cpu().numpy(), wx), level
            if level == 0.0:
                assert np.array_equal(w, g["best"][sl, seat])                                                        # get_best_actions
        env.close()


@gpu
def test_get_action_nan_and_inf_rows_follow_the_model(evg):
    import torch
    N = 37
    rng = np.random.RandomState(5)
    q = (np.round(rng.standard_normal((N, 12, 11)) * 2) / 2).astype(np.float32)
    q[rng.rand(N, 12, 11) < 0.05] = np.nan
    q[rng.rand(N, 12, 11) < 0.05] = np.inf
    q[rng.rand(N, 12, 11) < 0.05] = -np.inf
    q[3] = 0.0
    env = evg.EvergladesVecEnv(N, seed=9)
    env.reset()
    rows = env.minimized_get_action(torch.as_tensor(q).to(env.device), 0.0)
    want = np.stack([mm.best_actions(q[e]) for e in range(N)])
    assert np.array_equal(rows.cpu().numpy(), want)
    env.close()


# ---------------------------------------------------------------------------------------------- the fused forms
def _fused_against_composition(evg, N, seat, league, turns=160):
    import torch
    seed = 4242 + N
    a = evg.EvergladesVecEnv(N, seed=seed, auto_reset=True)
    b = evg.EvergladesVecEnv(N, seed=seed, auto_reset=True)
    a.reset(), b.reset()
    dev = a.device
    if league:
        w = [1.0 + (i % 4) for i in range(15)]
        pa, pb = a.opponent_league(LEAGUE15, weights=w, seat=seat), b.opponent_league(LEAGUE15, weights=w, seat=seat)
    else:
        pa = pb = "swarm"
    fa = (torch.zeros((N, 34), device=dev), torch.zeros((N, 12, 13), device=dev))
    fb = (torch.zeros((N, 34), device=dev), torch.zeros((N, 12, 13), device=dev))
    ra, rb = torch.zeros((N, 7, 2), dtype=torch.int32, device=dev), torch.zeros((N, 7, 2), dtype=torch.int32, device=dev)
    xa, xb = torch.zeros(N, dtype=torch.uint8, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    oa, ob = torch.zeros((N, 105), device=dev), torch.zeros((N, 105), device=dev)
    eps_env = torch.linspace(0.0, 1.0, N, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(N)
    ends = explores = 0
    for t in range(turns):
        q = _q(torch, (N, 12, 11), gen, dev)
        eps = eps_env if t % 2 else 0.3
        got = a.step_vs_q(pa, q, eps, seat=seat, features=fa if t % 3 else None, explored=xa, actions_out=ra, out=oa)
        b.minimized_get_action(q, eps, seat=seat, out=rb, explored=xb)
        want = b.step_vs(pb, rb, seat=seat, out=ob, features=fb if t % 3 else None)
        assert torch.equal(ra, rb) and torch.equal(xa, xb), t
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), t
        for k in ("winner", "scores", "status"):
            assert torch.equal(got[3][k], want[3][k]), (t, k)
        assert torch.equal(fa[0], fb[0]) and torch.equal(fa[1], fb[1]), t
        ends += int(got[2].sum().item())
        explores += int(xa.sum().item())
    assert ends >= N and 0 < explores < N * turns                     # episodes did end (and, in the league, members changed)
    s1, s2 = a.get_state(), b.get_state()
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    r1, r2 = a.get_run_state(), b.get_run_state()
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k
    if league:
        l1, l2 = pa.state(), pb.state()
        for k in ("assign", "objects", "counts", "ctl"):
            assert np.array_equal(l1[k], l2[k]), k
        assert len(set(l1["assign"].tolist())) > 3 and l1["counts"][:, 0].sum() == ends
    a.close(), b.close()


@gpu
@pytest.mark.parametrize("N", [37, 70])
@pytest.mark.parametrize("seat", [0, 1])
def test_step_vs_q_eleven_way_head_equals_get_action_plus_step_vs(evg, N, seat):
    _fused_against_composition(evg, N, seat, league=False)


@gpu
@pytest.mark.parametrize("N", [37, 70])
@pytest.mark.parametrize("seat", [0, 1])
def test_step_vs_q_eleven_way_head_against_a_fifteen_member_league(evg, N, seat):
    _fused_against_composition(evg, N, seat, league=True)


@gpu
def test_eleven_way_head_takes_no_directions(evg):
    import torch
    env = evg.EvergladesVecEnv(37, seed=1)
    env.reset()
    q = torch.zeros((37, 12, 11), device=env.device)
    with pytest.raises(ValueError):
        env.step_vs_q("swarm", q, 0.0, directions=torch.zeros((37, 7, 2), dtype=torch.int32, device=env.device))
    env.close()


# ---------------------------------------------------------------------------------------------- evg_minimized_qnet
def _net(h1, seed):
    rng = np.random.RandomState(seed)
    return tuple((rng.standard_normal(s) * 0.3).astype(np.float32) for s in ((h1, 59), (h1,), (11, h1), (11,)))


def _features(rows, seed, seats=None):
    rng = np.random.RandomState(seed)
    lead = (rows,) if seats is None else (rows, seats)
    shared = rng.rand(*(lead + (34,))).astype(np.float32)
    swarm = np.zeros(lead + (12, 13), np.float32)
    loc = rng.randint(0, 11, lead + (12,))
    np.put_along_axis(swarm[..., :11], loc[..., None], 1.0, axis=-1)
    swarm[..., 11] = rng.rand(*(lead + (12,))).astype(np.float32)
    swarm[..., 12] = rng.randint(0, 2, lead + (12,))
    return shared, swarm


@pytest.fixture(scope="module")
def qnet_env(evg):
    env = evg.EvergladesVecEnv(64, seed=3)
    yield env
    env.close()


@gpu
@pytest.mark.parametrize("h1", [1, 16, 17, 80, 128])
@pytest.mark.parametrize("final_relu", [True, False])
def test_qnet_equals_the_host_model_bit_for_bit(evg, qnet_env, h1, final_relu):
    """rows 1, 15, 16, 17 (around one group of 16) and 1 000 (63 groups: more than one workgroup, a partial last group) in all three layouts, for every
    hidden size and both final_relu values.  The host model's chain is computed once per layout on the 1 000 rows and sliced."""
    import torch
    from qnet_model import expand
    env = qnet_env
    dev = env.device
    params, params1 = _net(h1, 100 + h1), _net(h1, 200 + h1)
    tp = tuple(torch.as_tensor(p).to(dev) for p in params)
    net = env.minimized_qnet(tp, final_relu=final_relu)
    pair = env.minimized_qnet((tp, tuple(torch.as_tensor(p).to(dev) for p in params1)), final_relu=final_relu)       # seat p through set p
    big = 1000
    shared, swarm = _features(big, 7)
    x = expand(shared, swarm).reshape(-1, 59)[:big]
    s2, w2 = _features(big, 11, seats=2)
    want_x = mm.forward(x, params, final_relu)
    want_c = mm.forward_compact(shared, swarm, params, final_relu)
    want_s = np.stack([mm.forward_compact(s2[:, p], w2[:, p], pr, final_relu) for p, pr in enumerate((params, params1))], axis=1)
    for rows in (1, 15, 16, 17, big):
        got = net.expanded(torch.as_tensor(x[:rows]).to(dev))
        assert np.array_equal(got.cpu().numpy(), want_x[:rows]), ("expanded", rows)
        got = net(torch.as_tensor(shared[:rows]).to(dev), torch.as_tensor(swarm[:rows]).to(dev))
        assert np.array_equal(got.cpu().numpy(), want_c[:rows]), ("compact", rows)
        got = pair(torch.as_tensor(s2[:rows]).to(dev), torch.as_tensor(w2[:rows]).to(dev))
        assert np.array_equal(got.cpu().numpy(), want_s[:rows]), ("seats", rows)
    # an in-place update of the weights is seen by the next call
    with torch.no_grad():
        tp[2].mul_(0.5)
        tp[1].add_(0.125)
    upd = (params[0], params[1] + np.float32(0.125), params[2] * np.float32(0.5), params[3])
    got = net.expanded(torch.as_tensor(x[:17]).to(dev))
    assert np.array_equal(got.cpu().numpy(), mm.forward(x[:17], upd, final_relu))


@gpu
def test_qnet_reference_module_shapes_and_the_recorded_forward(evg, qnet_env):
    import torch
    env = qnet_env
    d = load_golden("minimized_qnet.npz")

    class QNetwork(torch.nn.Module):                          # the reference module's shape: fc1, fc2
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2 = torch.nn.Linear(59, 80), torch.nn.Linear(80, 11)

    m = QNetwork().to(env.device)
    with torch.no_grad():
        for t, k in ((m.fc1.weight, "w1"), (m.fc1.bias, "b1"), (m.fc2.weight, "w2"), (m.fc2.bias, "b2")):
            t.copy_(torch.as_tensor(d[k]))
    net = env.minimized_qnet(m)
    assert net.final_relu and net.h1 == 80
    x = torch.as_tensor(d["x"]).to(env.device)
    got = net.expanded(x).cpu().numpy()
    params = (d["w1"], d["b1"], d["w2"], d["b2"])
    assert np.array_equal(got[:4], mm.forward(d["x"][:4], params, True))
    own = np.abs(mm.forward(d["x"].reshape(-1, 59), params, True).astype(np.float64) - mm.forward_f64(d["x"].reshape(-1, 59), params, True)).max()
    assert np.abs(got.astype(np.float64) - d["q"]).max() <= 4 * own
    seq = torch.nn.Sequential(m.fc1, torch.nn.ReLU(), m.fc2)
    net2 = env.minimized_qnet(seq)
    assert not net2.final_relu
    assert np.array_equal(net2.expanded(x[:2]).cpu().numpy(), mm.forward(d["x"][:2], params, False))
    with pytest.raises(ValueError):
        env.minimized_qnet(seq, final_relu=True)


# ---------------------------------------------------------------------------------------------- replay
@gpu
def test_replay_records_the_agent_rows_as_directions(evg):
    import torch
    N, H, n, turns = 37, 45, 2, 40
    env = evg.EvergladesVecEnv(N, seed=77, auto_reset=True)
    env.reset()
    dev = env.device
    mem = env.smart_replay(H, n_step=n, gamma=0.9, shaping="reward_short_games", seats=0)
    st = env.get_state()["env"]
    model = ReplayModel(N, 1, H, n, 0.9, "reward_short_games", seat=0, auto_reset=True, turn0=st[:, 0], episode0=st[:, 2])
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    gen = torch.Generator(device="cpu").manual_seed(1)
    for t in range(turns):
        q = _q(torch, (N, 12, 11), gen, dev)
        env.step_vs_q("swarm", q, 0.3, seat=0, features=mem.slot_features(t + 1), actions_out=mem.slot_directions(t))
        mem.record()
        rows = mem.slot_directions(t).cpu().numpy()
        assert rows[..., 1].min() >= 1 and rows[..., 1].max() <= 11
        model.record(rows, env.reward.cpu().numpy(), env.done.cpu().numpy())
        assert np.array_equal(mem.meta.cpu().numpy(), model.meta), t
        assert np.array_equal(mem.counts.cpu().numpy(), model.count), t
        assert np.array_equal(mem.rewards.cpu().numpy(), model.rew), t
        assert np.array_equal(mem.env_state.cpu().numpy(), model.ctr), t
    tr = model.transitions()
    assert tr["action"].min() >= 0 and tr["action"].max() <= 10
    done_slots = model.count[model.count > 0]
    assert done_slots.size > 0 and (done_slots == 7).all()            # every named swarm is a transition: 7 distinct swarms, no node 0
    assert int(mem.size().item()) == model.size()
    mem.check()
    env.close()


# ---------------------------------------------------------------------------------------------- the example
@gpu
@pytest.mark.parametrize("league", [False, True])
def test_training_example_runs_with_finite_losses(league):
    import os
    import sys
    import torch
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import minimized_training
    losses = minimized_training.main(2048, 60, 256, league=league)
    assert losses.numel() == 60 - 2 and bool(torch.isfinite(losses).all())


# ---------------------------------------------------------------------------------------------- bad input
@gpu
def test_bad_input_is_refused_with_nothing_launched(evg):
    import torch
    from everglades_amd import _lib
    env = evg.EvergladesVecEnv(37, seed=2)
    env.reset()
    dev, L = env.device, env.L
    vp = C.c_void_p
    w = [torch.zeros(s, device=dev) for s in ((80, 59), (80,), (11, 80), (11,))]
    x, out = torch.zeros((16, 59), device=dev), torch.full((16, 11), 7.0, device=dev)

    def desc(h1=80, size=None):
        d = _lib.EvgMiniQnet()
        d.struct_size = C.sizeof(_lib.EvgMiniQnet) if size is None else size
        d.h1, d.final_relu, d.num_sets = h1, 1, 1
        d.w1[0], d.b1[0], d.w2[0], d.b2[0] = (t.data_ptr() for t in w)
        return d

    def run(d, q_out=None):
        return L.evg_minimized_qnet(env._h, C.byref(d), _lib.QNET_EXPANDED, 16, vp(x.data_ptr()), None, vp((out if q_out is None else q_out).data_ptr()),
                                    env._stream())
    assert run(desc()) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    out.fill_(7.0)
    assert run(desc(size=C.sizeof(_lib.EvgMiniQnet) - 8)) == _lib.ERR_ARG
    assert run(desc(h1=0)) == _lib.ERR_ARG and run(desc(h1=129)) == _lib.ERR_ARG
    assert run(desc(), q_out=out.view(-1)[1:]) == _lib.ERR_ARG
    q = torch.zeros((37 * 12 * 11 + 4,), device=dev)
    rows = torch.full((37, 7, 2), -5, dtype=torch.int32, device=dev)
    assert L.evg_minimized_get_action(env._h, vp(q.data_ptr() + 4), 0.5, None, 0, vp(rows.data_ptr()), None, env._stream()) == _lib.ERR_ARG   # misaligned q
    assert L.evg_minimized_get_action(env._h, vp(q.data_ptr()), 1.5, None, 0, vp(rows.data_ptr()), None, env._stream()) == _lib.ERR_ARG
    p = env._p
    env._seat_buffers()
    assert L.evg_step_vs_policy_minimized_q(env._h, 0, vp(q.data_ptr() + 4), 0.5, None, 3, p["obs_seat"], None, None, vp(rows.data_ptr()), None,
                                            p["reward"], p["done"], p["winner"], p["scores"], p["status"], env._stream()) == _lib.ERR_ARG
    stock = evg.EvergladesVecEnv(37, seed=2, rng_mode="mt19937")
    stock.reset()
    stock._seat_buffers()
    sp = stock._p
    assert L.evg_minimized_get_action(stock._h, vp(q.data_ptr()), 0.5, None, 0, vp(rows.data_ptr()), None, stock._stream()) == _lib.ERR_ARG
    assert L.evg_step_vs_policy_minimized_q(stock._h, 0, vp(q.data_ptr()), 0.5, None, 3, sp["obs_seat"], None, None, vp(rows.data_ptr()), None,
                                            sp["reward"], sp["done"], sp["winner"], sp["scores"], sp["status"], stock._stream()) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and int(rows.max()) == -5                  # nothing ran
    stock.close()
    env.close()
