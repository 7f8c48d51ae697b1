"""GPU tests of evg_step_vs_policy_smart_q (EvergladesVecEnv.step_vs_q): the Smart_State learner's turn from its Q values in one launch -- DQNAgent.get_action
decoded inside the learner-seat step kernel.  The contract is the two-call path it replaces, bit for bit: evg_smart_get_action on the previous seat observation,
then evg_step_vs_policy_smart (or evg_step_vs_policy) with those rows -- every output, and the handle's state afterwards."""
import ctypes as C
import importlib.util
import os
import types

import numpy as np
import pytest

from conftest import ROOT, CUSTOM_FILES, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


def _q(torch, n, gen, device):
    """Q values rounded to halves (ties between swarms and between directions), with +-0.0, +-inf and NaN in some rows."""
    q = (torch.randn((n, 12, 5), generator=gen, device=device) * 2.0).round().div(2.0)
    sel = torch.randint(0, 40, (n, 12, 5), generator=gen, device=device)
    q = torch.where(sel == 0, torch.full_like(q, -0.0), q)
    q = torch.where(sel == 1, torch.full_like(q, 0.0), q)
    q = torch.where(sel == 2, torch.full_like(q, float("inf")), q)
    q = torch.where(sel == 3, torch.full_like(q, float("-inf")), q)
    q = torch.where(sel == 4, torch.full_like(q, float("nan")), q)
    return q.contiguous()


def _eps(torch, t, n, gen, device):
    """scalar 0, 0.1, 1 and a per-env tensor, in turn"""
    k = t % 4
    return (0.0, 0.1, 1.0)[k] if k < 3 else torch.rand(n, generator=gen, device=device)


class _Pair:
    """Two handles on the same games: `a` plays step_vs_q, `b` plays smart_get_action + step_vs; every output of a turn is compared on the device."""

    def __init__(self, evg, n, seat, bot, with_features=True, **kw):
        import torch
        self.torch, self.n, self.seat, self.bot = torch, n, seat, bot
        self.a = evg.EvergladesVecEnv(n, **kw)
        self.b = evg.EvergladesVecEnv(n, **kw)
        dev = self.a.device
        self.feat_a = (torch.full((n, 34), -7.0, device=dev), torch.full((n, 12, 13), -7.0, device=dev)) if with_features else None
        self.feat_b = (torch.full((n, 34), -5.0, device=dev), torch.full((n, 12, 13), -5.0, device=dev)) if with_features else None
        self.rows_a = torch.full((n, 7, 2), -3, dtype=torch.int32, device=dev)
        self.dirs_a = torch.full((n, 7, 2), -3, dtype=torch.int32, device=dev)
        self.ex_a = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        self.rows_b = torch.full((n, 7, 2), -4, dtype=torch.int32, device=dev)
        self.dirs_b = torch.full((n, 7, 2), -4, dtype=torch.int32, device=dev)
        self.ex_b = torch.full((n,), 8, dtype=torch.uint8, device=dev)
        self.obs_b = None

    def start(self):
        self.obs_b = self.b.observe_seat(self.seat)

    def turn(self, q, eps, what):
        torch = self.torch
        oa, ra, da, ia = self.a.step_vs_q(self.bot, q, eps, seat=self.seat, features=self.feat_a, directions=self.dirs_a, explored=self.ex_a,
                                          actions_out=self.rows_a)
        rows = self.b.smart_get_action(q, eps, seat=self.seat, obs=self.obs_b, out=self.rows_b, directions=self.dirs_b, explored=self.ex_b)
        self.obs_b, rb, db, ib = self.b.step_vs(self.bot, rows, seat=self.seat, features=self.feat_b)
        assert torch.equal(self.rows_a, self.rows_b), (what, "rows played")
        assert torch.equal(self.dirs_a, self.dirs_b), (what, "directions")
        assert torch.equal(self.ex_a, self.ex_b), (what, "explored")
        assert torch.equal(oa, self.obs_b), (what, "obs")
        assert torch.equal(ra, rb) and torch.equal(da, db), (what, "reward / done")
        for k in ("winner", "scores", "status"):
            assert torch.equal(ia[k], ib[k]), (what, k)
        if self.feat_a is not None:
            assert torch.equal(self.feat_a[0], self.feat_b[0]) and torch.equal(self.feat_a[1], self.feat_b[1]), (what, "features")

    def finish(self, what):
        sa, sb = self.a.get_state(), self.b.get_state()
        for k in ("groups", "nodes", "health", "env"):
            assert np.array_equal(sa[k], sb[k]), (what, "state", k)
        ra, rb = self.a.get_run_state(), self.b.get_run_state()
        assert sorted(ra) == sorted(rb)
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True), (what, "run state", k)
        self.a.close()
        self.b.close()


@pytest.mark.parametrize("n", [2 * 8192 + 77, 65536 + 37])
@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
def test_fused_equals_two_calls(evg, n, dtype):
    """40 turns from a mid-game start (auto-resets inside the loop), both seats, two bots, epsilon scalar 0 / 0.1 / 1 and per env, Q with ties, +-0.0,
    +-inf and NaN: rows, directions, explored flags, observations, features, rewards, done, winner, scores, status, then the state and the run state."""
    import torch
    for seat, bot in ((0, "swarm"), (1, "cycle_rush_turn25")):
        pr = _Pair(evg, n, seat, bot, seed=21 + seat, auto_reset=True, obs_dtype=dtype, env_id_base=300)
        for env in (pr.a, pr.b):
            env.reset()
            env.rollout_policies(85, "cycle_rush_turn25", "swarm", fused=True, turns_per_launch=85)
        pr.start()
        gen = torch.Generator(device=pr.a.device).manual_seed(100 + seat)
        explored_some = False
        for t in range(40):
            eps = _eps(torch, t, n, gen, pr.a.device)
            pr.turn(_q(torch, n, gen, pr.a.device), eps, (n, dtype, seat, t))
            if t % 4 == 1:
                explored_some = explored_some or bool(pr.ex_a.any())
        assert explored_some
        assert int(pr.a.episode_stats()["totals"][0]) > 0                    # episodes ended and restarted inside the loop
        pr.finish((n, dtype, seat))


def test_fused_decode_matches_oracle(evg, oracle_mod):
    """Each turn, the rows / directions / explored flags of the fused call equal the oracle's DQNAgent.get_action (the one pinned by
    tests/golden/smart_explore.npz) on the previous seat observation, with the episodes of the state the launch starts from; about 10 % explore at 0.1."""
    import torch
    N, seed, base = 65536 + 37, 12, 1000
    env = evg.EvergladesVecEnv(N, seed=seed, auto_reset=True, env_id_base=base)
    env.reset()
    env.rollout_policies(90, "cycle_rush_turn25", "swarm", fused=True, turns_per_launch=90)   # BaseCapture around turns 91-95: resets in the loop
    ids = (base + np.arange(N)).astype(np.uint32)
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.zeros((N, 7, 2), dtype=torch.int32, device=env.device)
    dirs = torch.zeros((N, 7, 2), dtype=torch.int32, device=env.device)
    ex = torch.zeros(N, dtype=torch.uint8, device=env.device)
    for seat, bot in ((0, "swarm"), (1, "cycle_rush_turn25")):
        prev = _np(env.observe_seat(seat)).astype(np.float64)
        for t in range(4):
            episodes = env.get_state()["env"][:, 2].astype(np.uint32)
            q = (torch.randn((N, 12, 5), generator=gen) * 2.0).round().div(2.0)
            eps_np = np.full(N, 0.1, np.float32) if t % 2 == 0 else np.random.default_rng(t).random(N).astype(np.float32)
            eps = 0.1 if t % 2 == 0 else torch.as_tensor(eps_np, device=env.device)
            obs, _, _, _ = env.step_vs_q(bot, q.to(env.device), eps, seat=seat, directions=dirs, explored=ex, actions_out=rows)
            want_a, want_d, want_x = oracle_mod.smart_get_action(q.numpy(), prev, seed, ids, episodes, seat, eps_np)
            assert np.array_equal(_np(rows), want_a) and np.array_equal(_np(dirs), want_d) and np.array_equal(_np(ex), want_x), (seat, t)
            if t % 2 == 0:
                assert abs(want_x.mean() - 0.1) < 0.005, want_x.mean()
            prev = _np(obs).astype(np.float64)
    assert int(env.episode_stats()["totals"][0]) > 0
    env.close()


def _custom_tables(evg, fname, tmp_path):
    d = load_golden(fname)
    kw = {}
    for key, arg in (("map_json", "map_file"), ("unit_json", "unit_file")):
        if str(d[key]):
            path = tmp_path / (fname + "_" + arg + ".json")
            path.write_text(str(d[key]))
            kw[arg] = str(path)
    return evg.tables_from_json(p1_node_map=d["p1_node_map"].tolist(), **kw)


@pytest.mark.parametrize("fname", CUSTOM_FILES)
def test_fused_equals_two_calls_on_non_default_tables(evg, fname, tmp_path):
    """custom_varA..C (other maps, unit files and p1_node_maps, a non-involutive one among them): the swarm locations of the decode are the caller's own
    numbering, as the observation shows them."""
    import torch
    tables = _custom_tables(evg, fname, tmp_path)
    N = 4096 + 19
    for seat, bot in ((1, "swarm"), (0, "cycle_rush_turn25")):
        pr = _Pair(evg, N, seat, bot, seed=3 + seat, auto_reset=True, tables=tables)
        for env in (pr.a, pr.b):
            env.reset()
            env.rollout_policies(60, "random", "swarm", fused=True, turns_per_launch=60)
        pr.start()
        gen = torch.Generator(device=pr.a.device).manual_seed(7 + seat)
        for t in range(30):
            pr.turn(_q(torch, N, gen, pr.a.device), _eps(torch, t, N, gen, pr.a.device), (fname, seat, t))
        pr.finish((fname, seat))


def test_fused_equals_two_calls_without_auto_reset(evg):
    """auto_reset=False, envs finishing inside the loop: frozen envs still get their rows, directions and explored flags, as evg_smart_get_action writes
    them, and repeat their terminal outputs; without the feature buffers the reference path is evg_step_vs_policy."""
    import torch
    N = 3000 + 5
    pr = _Pair(evg, N, 0, "cycle_rush_turn25", with_features=False, seed=8, auto_reset=False)
    for env in (pr.a, pr.b):
        env.reset()
        env.rollout_policies(120, "swarm", "cycle_rush_turn25", fused=True, turns_per_launch=120)
    pr.start()
    gen = torch.Generator(device=pr.a.device).manual_seed(11)
    for t in range(40):
        pr.turn(_q(torch, N, gen, pr.a.device), _eps(torch, t, N, gen, pr.a.device), ("no auto_reset", t))
    assert int(pr.a.status.ne(0).sum()) > N // 2                             # most games have ended and stay frozen
    pr.finish("no auto_reset")


def test_refusals(evg):
    """seat outside 0..1, epsilon 1.5, a stock-entropy handle, one of shared / swarm NULL and shared_out at 8 mod 16 are refused (EVG_ERR_INVALID);
    wrong shapes, dtypes or devices raise ValueError in step_vs_q."""
    import torch
    N = 300
    env = evg.EvergladesVecEnv(N, seed=1)
    env.reset()
    dev = env.device
    L = env.L
    q = torch.zeros((N, 12, 5), device=dev)
    obs = torch.zeros((N, 105), device=dev)
    shared_full = torch.zeros((N + 1, 34), device=dev)
    swarm = torch.zeros((N, 12, 13), device=dev)
    reward = torch.zeros((N, 2), device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)

    def call(h, seat=0, eps=0.0, shared=shared_full[:N], sw=swarm):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return L.evg_step_vs_policy_smart_q(h, seat, p(q), eps, None, 3, p(obs), p(shared), p(sw), None, None, None, p(reward), p(done), None, None,
                                            None, None)

    assert call(env._h) == 0
    torch.cuda.synchronize()
    for kw in (dict(seat=2), dict(seat=-1), dict(eps=1.5), dict(eps=float("nan")), dict(shared=None), dict(sw=None), dict(shared=shared_full[1:N + 1])):
        assert call(env._h, **kw) == -1, kw
    with pytest.raises(evg.EvgError):
        env.step_vs_q("swarm", q, 0.1, features=(shared_full[1:N + 1], swarm))
    stock = evg.EvergladesVecEnv(N, seed=1, rng_mode="mt19937")
    stock.reset()
    assert call(stock._h) == -1
    stock.close()
    for bad in (dict(q=q[:-1]), dict(q=q.double()), dict(q=q.cpu()), dict(epsilon=torch.zeros(N - 1, device=dev)),
                dict(features=(shared_full[:N - 1], swarm)), dict(directions=torch.zeros((N, 7), dtype=torch.int32, device=dev)),
                dict(explored=torch.zeros(N, dtype=torch.int32, device=dev)), dict(actions_out=torch.zeros((N, 7, 2), dtype=torch.int64, device=dev)),
                dict(out=torch.zeros((N, 104), device=dev))):
        kw = dict(q=q, epsilon=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            env.step_vs_q("swarm", kw.pop("q"), kw.pop("epsilon"), **kw)
    env.close()


def test_smart_state_loop_example_fused_equals_two_calls(evg):
    """examples/smart_state_loop.py main(fused=True) plays the same games as main(fused=False): episode statistics, final state and run state."""
    spec = importlib.util.spec_from_file_location("evg_example_smart_q", os.path.join(ROOT, "examples", "smart_state_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    finals = []

    class Recording(evg.EvergladesVecEnv):
        def close(self):
            if getattr(self, "_h", None):
                finals.append((self.get_state(), self.get_run_state()))
            super().close()

    ex.evg = types.SimpleNamespace(EvergladesVecEnv=Recording)
    got = [ex.main(num_envs=2053, turns=170, epsilon=0.25, opponent="cycle_rush_turn25", seat=1, seed=4, fused=f) for f in (False, True)]
    assert int(got[0]["totals"][0]) >= 2053
    for k in got[0]:
        assert np.array_equal(np.asarray(got[0][k]), np.asarray(got[1][k])), k
    assert len(finals) == 2
    for k in ("groups", "nodes", "health", "env"):
        assert np.array_equal(finals[0][0][k], finals[1][0][k]), k
    for k in finals[0][1]:
        assert np.array_equal(np.asarray(finals[0][1][k]), np.asarray(finals[1][1][k]), equal_nan=True), k
