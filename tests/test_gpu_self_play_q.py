"""GPU tests of evg_step_smart_q (EvergladesVecEnv.step_q): the self-play turn from both seats' Q values in one launch -- DQNAgent.get_action for each seat
decoded inside the plain step kernel.  The contract is the five-call path it replaces, bit for bit: evg_smart_get_action for seat 0 and for seat 1 on the
previous observation, evg_step with both seats' rows, evg_smart_state_compact for player 0 and for player 1 -- every output, and the handle's state and run
state afterwards."""
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
    """Both seats' Q values rounded to halves (ties between swarms and between directions), with +-0.0, +-inf and NaN in some rows."""
    q = (torch.randn((n, 2, 12, 5), generator=gen, device=device) * 2.0).round().div(2.0)
    sel = torch.randint(0, 40, (n, 2, 12, 5), generator=gen, device=device)
    q = torch.where(sel == 0, torch.full_like(q, -0.0), q)
    q = torch.where(sel == 1, torch.full_like(q, 0.0), q)
    q = torch.where(sel == 2, torch.full_like(q, float("inf")), q)
    q = torch.where(sel == 3, torch.full_like(q, float("-inf")), q)
    q = torch.where(sel == 4, torch.full_like(q, float("nan")), q)
    return q.contiguous()


def _eps(torch, t, n, gen, device):
    """(0, 0), (0.1, 0), (1, 0.3) and a per-env [N, 2] tensor, in turn"""
    k = t % 4
    return ((0.0, 0.0), (0.1, 0.0), (1.0, 0.3))[k] if k < 3 else torch.rand((n, 2), generator=gen, device=device)


class _Pair:
    """Two handles on the same games: `a` plays step_q, `b` plays smart_get_action x 2 + step + smart_state_compact x 2; every output of a turn is
    compared on the device."""

    def __init__(self, evg, n, with_features=True, **kw):
        import torch
        self.torch, self.n = torch, n
        self.a = evg.EvergladesVecEnv(n, **kw)
        self.b = evg.EvergladesVecEnv(n, **kw)
        dev = self.a.device
        self.feat_a = (torch.full((n, 2, 34), -7.0, device=dev), torch.full((n, 2, 12, 13), -7.0, device=dev)) if with_features else None
        self.feat_b = [(torch.full((n, 34), -5.0, device=dev), torch.full((n, 12, 13), -5.0, device=dev)) for _ in range(2)] if with_features else None
        self.rows_a = torch.full((n, 2, 7, 2), -3, dtype=torch.int32, device=dev)
        self.dirs_a = torch.full((n, 2, 7, 2), -3, dtype=torch.int32, device=dev)
        self.ex_a = torch.full((n, 2), 9, dtype=torch.uint8, device=dev)
        self.rows_b = [torch.full((n, 7, 2), -4, dtype=torch.int32, device=dev) for _ in range(2)]
        self.dirs_b = [torch.full((n, 7, 2), -4, dtype=torch.int32, device=dev) for _ in range(2)]
        self.ex_b = [torch.full((n,), 8, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.obs_b = None

    def start(self):
        self.obs_b = self.b.observe()

    def turn(self, q, eps, what):
        torch = self.torch
        oa, ra, da, ia = self.a.step_q(q, eps, features=self.feat_a, directions=self.dirs_a, explored=self.ex_a, actions_out=self.rows_a)
        for p in range(2):
            eps_p = eps[:, p].contiguous() if isinstance(eps, torch.Tensor) else eps[p]
            self.b.smart_get_action(q[:, p].contiguous(), eps_p, seat=p, obs=self.obs_b, out=self.rows_b[p], directions=self.dirs_b[p], explored=self.ex_b[p])
        self.obs_b, rb, db, ib = self.b.step(torch.stack(self.rows_b, dim=1))
        if self.feat_b is not None:
            for p in range(2):
                self.b.smart_state_compact(p, self.obs_b, *self.feat_b[p])
        for p in range(2):
            assert torch.equal(self.rows_a[:, p], self.rows_b[p]), (what, p, "rows played")
            assert torch.equal(self.dirs_a[:, p], self.dirs_b[p]), (what, p, "directions")
            assert torch.equal(self.ex_a[:, p], self.ex_b[p]), (what, p, "explored")
        assert torch.equal(oa, self.obs_b), (what, "obs")
        assert torch.equal(ra, rb) and torch.equal(da, db), (what, "reward / done")
        for k in ("winner", "scores", "status"):
            assert torch.equal(ia[k], ib[k]), (what, k)
        if self.feat_a is not None:
            for p in range(2):
                assert torch.equal(self.feat_a[0][:, p], self.feat_b[p][0]), (what, p, "shared features")
                assert torch.equal(self.feat_a[1][:, p], self.feat_b[p][1]), (what, p, "swarm features")

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
def test_fused_equals_five_calls(evg, n, dtype):
    """40 turns from a mid-game start (auto-resets inside the loop), epsilon (0, 0) / (0.1, 0) / (1, 0.3) and per env, Q with ties, +-0.0, +-inf and NaN:
    both seats' rows, directions and explored flags, observations, both players' features, rewards, done, winner, scores, status, then the state and the
    run state."""
    import torch
    pr = _Pair(evg, n, seed=31, auto_reset=True, obs_dtype=dtype, env_id_base=500)
    for env in (pr.a, pr.b):
        env.reset()
        env.rollout_policies(85, "cycle_rush_turn25", "swarm", fused=True, turns_per_launch=85)
    pr.start()
    gen = torch.Generator(device=pr.a.device).manual_seed(200)
    explored = [False, False]
    for t in range(40):
        pr.turn(_q(torch, n, gen, pr.a.device), _eps(torch, t, n, gen, pr.a.device), (n, dtype, t))
        for p in range(2):
            explored[p] = explored[p] or bool(pr.ex_a[:, p].any())
    assert all(explored)
    assert int(pr.a.episode_stats()["totals"][0]) > 0                    # episodes ended and restarted inside the loop
    pr.finish((n, dtype))


def test_fused_decode_matches_oracle(evg, oracle_mod):
    """Each turn, both seats' rows / directions / explored flags of the fused call equal the oracle's DQNAgent.get_action on the previous observation of
    that seat, and the oracle game stepped with those rows shows the same observation."""
    import torch
    N, seed, base = 300, 17, 2000
    env = evg.EvergladesVecEnv(N, seed=seed, auto_reset=True, env_id_base=base)
    ora = oracle_mod.Oracle(N, seed=seed, auto_reset=True, env_id_base=base)
    prev = _np(env.reset()).astype(np.float64)
    assert np.array_equal(prev, ora.reset())
    ids = (base + np.arange(N)).astype(np.uint32)
    gen = torch.Generator(device="cpu").manual_seed(6)
    rows = torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=env.device)
    dirs = torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=env.device)
    ex = torch.zeros((N, 2), dtype=torch.uint8, device=env.device)
    explored = np.zeros(2, bool)
    for t in range(30):
        episodes = env.get_state()["env"][:, 2].astype(np.uint32)
        q = (torch.randn((N, 2, 12, 5), generator=gen) * 2.0).round().div(2.0)
        if t % 2 == 0:
            eps_np, eps = np.tile(np.array([0.3, 0.0], np.float32), (N, 1)), (0.3, 0.0)
        else:
            eps_np = np.random.default_rng(t).random((N, 2)).astype(np.float32)
            eps = torch.as_tensor(eps_np, device=env.device)
        obs, _, _, _ = env.step_q(q.to(env.device), eps, directions=dirs, explored=ex, actions_out=rows)
        want = [oracle_mod.smart_get_action(np.ascontiguousarray(q[:, p].numpy()), np.ascontiguousarray(prev[:, p]), seed, ids, episodes, p,
                                            np.ascontiguousarray(eps_np[:, p])) for p in range(2)]
        for p in range(2):
            assert np.array_equal(_np(rows[:, p]), want[p][0]), (t, p, "rows")
            assert np.array_equal(_np(dirs[:, p]), want[p][1]), (t, p, "directions")
            assert np.array_equal(_np(ex[:, p]), want[p][2]), (t, p, "explored")
            explored[p] |= bool(want[p][2].any())
        o_obs, _, _, _ = ora.step(np.stack([want[0][0], want[1][0]], axis=1))
        assert np.array_equal(_np(obs).astype(np.float64), o_obs), (t, "obs")
        prev = o_obs
    assert explored.all()
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
def test_fused_equals_five_calls_on_non_default_tables(evg, fname, tmp_path):
    """custom_varA..C (other maps, unit files and p1_node_maps, a non-involutive one among them): each seat's swarm locations are decoded in that seat's
    own numbering, as its observation shows them."""
    import torch
    tables = _custom_tables(evg, fname, tmp_path)
    N = 4096 + 19
    pr = _Pair(evg, N, seed=5, auto_reset=True, tables=tables)
    for env in (pr.a, pr.b):
        env.reset()
        env.rollout_policies(60, "random", "swarm", fused=True, turns_per_launch=60)
    pr.start()
    gen = torch.Generator(device=pr.a.device).manual_seed(9)
    for t in range(30):
        pr.turn(_q(torch, N, gen, pr.a.device), _eps(torch, t, N, gen, pr.a.device), (fname, t))
    pr.finish(fname)


def test_fused_equals_five_calls_without_auto_reset(evg):
    """auto_reset=False, envs finishing inside the loop: frozen envs still get both seats' rows, directions and explored flags and repeat their terminal
    outputs; without the feature buffers the reference path is evg_smart_get_action x 2 + evg_step."""
    import torch
    N = 3000 + 5
    pr = _Pair(evg, N, with_features=False, seed=8, auto_reset=False)
    for env in (pr.a, pr.b):
        env.reset()
        env.rollout_policies(120, "swarm", "cycle_rush_turn25", fused=True, turns_per_launch=120)
    pr.start()
    gen = torch.Generator(device=pr.a.device).manual_seed(13)
    for t in range(40):
        pr.turn(_q(torch, N, gen, pr.a.device), _eps(torch, t, N, gen, pr.a.device), ("no auto_reset", t))
    assert int(pr.a.status.ne(0).sum()) > N // 2                             # most games have ended and stay frozen
    pr.finish("no auto_reset")


def test_refusals(evg):
    """Missing required pointers, either epsilon outside [0, 1], only one of shared / swarm, misaligned q / obs / shared / actions_out and a stock-entropy
    handle are refused (EVG_ERR_INVALID); wrong shapes, dtypes or devices raise ValueError in step_q."""
    import torch
    N = 300
    env = evg.EvergladesVecEnv(N, seed=1)
    env.reset()
    dev = env.device
    L = env.L

    def buf(shape, dtype=torch.float32):           # (contiguous tensor, the same shape 4 bytes further on: misaligned)
        flat = torch.zeros(int(np.prod(shape)) * 2 + 16, dtype=dtype, device=dev)
        k = 4 // flat.element_size()
        return flat[:int(np.prod(shape))].view(shape), flat[k:k + int(np.prod(shape))].view(shape)

    q, q_mis = buf((N, 2, 12, 5))
    obs, obs_mis = buf((N, 2, 105))
    shared, shared_mis = buf((N, 2, 34))
    swarm, _ = buf((N, 2, 12, 13))
    rows, rows_mis = buf((N, 2, 7, 2), torch.int32)
    reward = torch.zeros((N, 2), device=dev)
    done = torch.zeros(N, dtype=torch.uint8, device=dev)

    def call(h, q=q, e0=0.0, e1=0.0, obs=obs, shared=shared, sw=swarm, rows=rows, reward=reward, done=done):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return L.evg_step_smart_q(h, p(q), e0, e1, None, p(obs), p(shared), p(sw), p(rows), None, None, p(reward), p(done), None, None, None, None)

    assert call(env._h) == 0
    torch.cuda.synchronize()
    for kw in (dict(q=None), dict(obs=None), dict(reward=None), dict(done=None), dict(e0=1.5), dict(e1=-0.1), dict(e1=float("nan")),
               dict(shared=None), dict(sw=None), dict(q=q_mis), dict(obs=obs_mis), dict(shared=shared_mis), dict(rows=rows_mis)):
        assert call(env._h, **kw) == -1, kw
    with pytest.raises(evg.EvgError):
        env.step_q(q, 0.1, features=(shared_mis, swarm))
    stock = evg.EvergladesVecEnv(N, seed=1, rng_mode="mt19937")
    stock.reset()
    assert call(stock._h) == -1
    stock.close()
    for bad in (dict(q=q[:, 0].contiguous()), dict(q=q.double()), dict(q=q.cpu()), dict(epsilon=torch.zeros(N, device=dev)),
                dict(epsilon=torch.zeros((N, 2), dtype=torch.float64, device=dev)), dict(epsilon=(0.1, 0.0, 0.0)),
                dict(features=(shared[:, 0].contiguous(), swarm)), dict(directions=torch.zeros((N, 7, 2), dtype=torch.int32, device=dev)),
                dict(explored=torch.zeros(N, dtype=torch.uint8, device=dev)), dict(actions_out=torch.zeros((N, 2, 7, 2), dtype=torch.int64, device=dev)),
                dict(out=torch.zeros((N, 105), device=dev))):
        kw = dict(q=q, epsilon=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            env.step_q(kw.pop("q"), kw.pop("epsilon"), **kw)
    env.close()


def test_self_play_example_fused_equals_five_calls(evg):
    """examples/smart_state_self_play.py main(fused=True) plays the same games as main(fused=False): win / loss / tie counts and the other episode
    statistics, final state and run state."""
    spec = importlib.util.spec_from_file_location("evg_example_self_play", os.path.join(ROOT, "examples", "smart_state_self_play.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    finals = []

    class Recording(evg.EvergladesVecEnv):
        def close(self):
            if getattr(self, "_h", None):
                finals.append((self.get_state(), self.get_run_state()))
            super().close()

    ex.evg = types.SimpleNamespace(EvergladesVecEnv=Recording)
    got = [ex.main(num_envs=2053, turns=170, epsilon=(0.1, 0.0), seed=4, fused=f) for f in (False, True)]
    assert int(got[0]["totals"][0]) >= 2053
    for k in got[0]:
        assert np.array_equal(np.asarray(got[0][k]), np.asarray(got[1][k])), k
    assert len(finals) == 2
    for k in ("groups", "nodes", "health", "env"):
        assert np.array_equal(finals[0][0][k], finals[1][0][k]), k
    for k in finals[0][1]:
        assert np.array_equal(np.asarray(finals[0][1][k]), np.asarray(finals[1][1][k]), equal_nan=True), k
