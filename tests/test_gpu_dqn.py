"""GPU tests of the agents/DQN family's device path (include/evg_dqn.h, libevg_dqn.so): evg_dqn_qnet (EvergladesVecEnv.dqn_qnet / everglades_amd.DqnQNet),
evg_dqn_actions and evg_dqn_get_action.  References are the host model (tests/dqn_model.py, pinned to the reference's own methods by
tests/golden/dqn_agent.npz on the CPU) and the fixture itself, never the device.

The network kernel's paths: a workgroup pass is R = 16 rows (one group shared by the four wavefronts) up to 4 096 rows, R = 64 rows (one 16-row group
per wavefront) up to 16 384 rows and R = 256 rows (four groups) beyond; the hidden layer is streamed in chunks of C = 48 units; the grid is capped at
256 workgroups.  Large row counts repeat a short block of rows (period 509, a prime: every position inside a 16-row group and a pass meets every
row), so the model is evaluated on 509 rows and the whole output is compared."""
import numpy as np
import pytest

import dqn_model as dm
from conftest import load_golden

gpu = pytest.mark.gpu
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
R_TINY, R_SMALL, R_LARGE, TINY_ROWS, SMALL_ROWS, CHUNK, CAP, PERIOD = 16, 64, 256, 4096, 16384, 48, 256, 509


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    L = everglades_amd._lib
    assert (L.DQN_TINY_ROWS, L.DQN_SMALL_ROWS, L.DQN_CHUNK, L.DQN_MAX_BLOCKS) == (TINY_ROWS, SMALL_ROWS, CHUNK, CAP)
    return everglades_amd


@pytest.fixture(scope="module")
def env(evg):
    e = evg.EvergladesVecEnv(37, seed=11)
    e.reset()
    yield e
    e.close()


def _net(h1, seed, coarse=False):
    """seeded parameters; coarse: on a grid of eighths, so that exact zeros and ties occur"""
    rng = np.random.RandomState(seed)
    p = [rng.standard_normal(s).astype(np.float32) * sc for s, sc in (((h1, 105), 0.1), ((h1,), 0.3), ((132, h1), 0.2), ((132,), 0.3))]
    return [np.round(t * 8) / 8 for t in p] if coarse else p


def _x(rows, seed, coarse=False):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((min(rows, PERIOD), 105)).astype(np.float32)
    return np.round(x * 4) / 4 if coarse else x


def _device(env, params):
    import torch
    return tuple(torch.as_tensor(np.ascontiguousarray(t, np.float32)).to(env.device) for t in params)


def _same(got, want):
    """bit-equal up to the sign of a zero: the NaN positions and every other value"""
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0))


def _check_rows(env, params, base, rows, final_relu):
    """the device's Q of `rows` rows that repeat `base` against the model's Q of base"""
    import torch
    want = dm.forward(base, params, final_relu)
    reps = -(-rows // base.shape[0])
    x = torch.as_tensor(base).to(env.device).repeat(reps, 1)[:rows].contiguous()
    qnet = env.dqn_qnet(_device(env, params), final_relu=final_relu)
    got = qnet.rows(x).cpu().numpy()
    assert got.shape == (rows, 132)
    assert _same(got, np.tile(want, (reps, 1))[:rows]), (rows, params[0].shape[0], final_relu)
    return got


# ---------------------------------------------------------------------------------------------- evg_dqn_qnet: shapes
@gpu
@pytest.mark.parametrize("rows", [1, R_TINY - 1, R_TINY, R_TINY + 1, 63, 64, 65, 257])
def test_forward_is_bit_equal_to_the_model_over_row_counts(env, rows):
    """the 16-row form: a ragged group, one group, R - 1, R, R + 1, several workgroups"""
    params = _net(48, 1)
    q = _check_rows(env, params, _x(rows, rows), rows, True)
    assert (q >= 0).all() and 0.1 < (q > 0).mean() < 0.9
    _check_rows(env, params, _x(rows, rows + 1), rows, False)


@gpu
@pytest.mark.parametrize("h1", [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 527, 528])
def test_forward_is_bit_equal_to_the_model_over_hidden_sizes(env, h1):
    """rows = 33 (the 16-row form) and the same 33 rows repeated to 4 129 and 16 417 rows (the 64- and the 256-row form)"""
    for final_relu in (True, False):
        _check_rows(env, _net(h1, h1), _x(33, h1), 33, final_relu)
    _check_rows(env, _net(h1, h1), _x(33, h1), TINY_ROWS + 33, True)
    _check_rows(env, _net(h1, h1), _x(33, h1), SMALL_ROWS + 33, True)


@gpu
@pytest.mark.parametrize("rows", [TINY_ROWS - 1, TINY_ROWS, TINY_ROWS + 1, TINY_ROWS + R_SMALL - 1, TINY_ROWS + R_SMALL, TINY_ROWS + R_SMALL + 1,
                                  SMALL_ROWS, SMALL_ROWS + 1, SMALL_ROWS + R_LARGE - 1, SMALL_ROWS + R_LARGE, SMALL_ROWS + R_LARGE + 1, CAP * R_LARGE + 17])
def test_forward_at_the_thresholds_between_the_kernels_and_past_the_grid_cap(env, rows):
    """4 096 rows are the last the 16-row passes take (256 workgroups); 4 097 rows are 65 passes of 64 rows, the last with one row; 4 159 / 4 160 / 4 161
    are R - 1, R, R + 1 for the 64-row passes.  16 384 rows are the last the 64-row passes take (256 workgroups, one pass each); one row more is 65
    passes of 256 rows, the last with one row; 16 639 / 16 640 / 16 641 are R - 1, R, R + 1 for the 256-row passes; 65 553 rows are 257 passes on 256 workgroups: workgroup 0 runs a second pass
    of 17 rows.  h1 = 16, rows of period 509."""
    _check_rows(env, _net(16, 3), _x(rows, 4), rows, True)


@gpu
@pytest.mark.parametrize("h1,rows", [(48, 65), (97, 33), (49, TINY_ROWS + 5), (16, SMALL_ROWS + 5)])
def test_forward_on_a_coarse_grid_with_exact_zeros_and_ties(env, h1, rows):
    params, x = _net(h1, 7, coarse=True), _x(rows, 8, coarse=True)
    assert (params[0] == 0).any() and (x == 0).any()
    for final_relu in (True, False):
        _check_rows(env, params, x, rows, final_relu)


# ---------------------------------------------------------------------------------------------- evg_dqn_qnet: numeric edges
@gpu
def test_forward_numeric_edges_follow_the_model(env):
    """rows = 33 -- and the same rows repeated through the other two forms --, h1 = 17 (one chunk, its second column tile with one live unit): NaN, +-Inf, subnormals and values that overflow in layer 2, planted in x,
    the weights and the biases, one class at a time and all together.  NaN positions and all other bits equal the model's."""
    base_p, base_x = _net(17, 21), _x(33, 22)
    big = np.float32(3e38)

    def plant_x(x, p):
        x[1, 0], x[2, 104], x[3, 50], x[32, 104] = np.nan, np.inf, -np.inf, np.nan
        x[4, 7], x[5, 104] = np.float32(1e-41), np.float32(-3e-45)

    def plant_w(x, p):
        p[0][0, 5], p[0][16, 104], p[0][3, 0] = np.nan, np.inf, np.float32(2e-42)
        p[2][0, 16], p[2][131, 0], p[2][7, 3] = -np.inf, np.nan, np.float32(1e-40)

    def plant_b(x, p):
        p[1][2], p[1][16], p[3][5], p[3][131], p[3][9] = np.inf, np.nan, -np.inf, np.nan, np.float32(1e-39)

    def plant_overflow(x, p):
        p[1][4] = big                       # a hidden activation of 3e38 ...
        p[0][4] = 0
        p[2][10, 4], p[2][11, 4], p[2][12, 4] = 2.0, -2.0, 1.0       # ... overflows to +Inf and -Inf in layer 2, and stays finite
        p[3][12] = -big

    def plant_all(x, p):
        for f in (plant_x, plant_w, plant_b, plant_overflow):
            f(x, p)

    for plant in (plant_x, plant_w, plant_b, plant_overflow, plant_all):
        p, x = [t.copy() for t in base_p], base_x.copy()
        plant(x, p)
        for rows in (TINY_ROWS + 33, SMALL_ROWS + 33):          # the same 33 rows, repeated, through the 64- and the 256-row form
            _check_rows(env, p, x, rows, True)
        for final_relu in (True, False):
            q = _check_rows(env, p, x, 33, final_relu)
        if plant is plant_overflow:
            assert np.isposinf(q[:, 10]).all() and np.isneginf(q[:, 11]).all() and np.isfinite(q[:, 12]).all()
        if plant is plant_x:
            assert np.isnan(q[1]).all() and np.isnan(q[32]).all() and np.isfinite(q[0]).all()


# ---------------------------------------------------------------------------------------------- evg_dqn_qnet: nothing outside [rows, 132]
@gpu
@pytest.mark.parametrize("rows,h1", [(33, 17), (1, 48), (TINY_ROWS + 1, 16), (SMALL_ROWS + 1, 16)])
def test_forward_writes_nothing_outside_its_rows_and_reads_nothing_behind_them(env, rows, h1):
    """4 KB behind q and the bytes after the last input row hold a pattern: nothing outside [rows, 132] changes, the last row's result does not depend
    on the pattern, and a NaN pattern does not reach Q."""
    import torch
    params, base = _net(h1, 31), _x(rows, 32)
    want = dm.forward(base, params, True)
    reps = -(-rows // base.shape[0])
    want = np.tile(want, (reps, 1))[:rows]
    qnet = env.dqn_qnet(_device(env, params), final_relu=True)
    for pattern in (12345.0, float("nan")):
        xbuf = torch.full((rows * 105 + 1024,), pattern, dtype=torch.float32, device=env.device)
        qbuf = torch.full((rows * 132 + 1024,), pattern, dtype=torch.float32, device=env.device)
        x, out = xbuf[:rows * 105].view(rows, 105), qbuf[:rows * 132].view(rows, 132)
        x.copy_(torch.as_tensor(base).to(env.device).repeat(reps, 1)[:rows])
        guard = qbuf[rows * 132:].clone().view(torch.int32)
        got = qnet.rows(x, out=out)
        assert got is out and _same(out.cpu().numpy(), want), pattern
        assert torch.equal(qbuf[rows * 132:].view(torch.int32), guard), pattern
        assert torch.equal(xbuf[rows * 105:].view(torch.int32), torch.full((1024,), pattern, dtype=torch.float32, device=env.device).view(torch.int32))


# ---------------------------------------------------------------------------------------------- evg_dqn_qnet: the handle's observation buffers
@gpu
@pytest.mark.parametrize("obs_dtype", ["float32", "float64", "int16"])
def test_observation_forms_equal_the_float_rows_and_the_model(evg, obs_dtype):
    import torch
    e = evg.EvergladesVecEnv(37, seed=5, obs_dtype=obs_dtype)
    e.reset()
    for _ in range(6):
        e.step(e.random_actions())
    params = _net(48, 41)
    qnet = e.dqn_qnet(_device(e, params), final_relu=True)
    obs = e.obs
    assert obs.dtype == getattr(torch, obs_dtype) and tuple(obs.shape) == (37, 2, 105) and (obs.cpu().numpy()[:, :, 1:] != 0).any()
    for p in (0, 1):
        want = dm.forward(obs[:, p].cpu().numpy().astype(np.float32), params, True)
        rows = qnet.rows(obs[:, p].float().contiguous()).cpu().numpy()
        two = qnet(obs, seat=p).cpu().numpy()
        one = qnet(e.observe_seat(p).clone()).cpu().numpy()
        assert np.array_equal(rows, want) and np.array_equal(two, rows) and np.array_equal(one, rows), (obs_dtype, p)
    with pytest.raises(ValueError):
        qnet(obs)                                   # a two-seat buffer needs its seat
    with pytest.raises(ValueError):
        qnet(obs.float() if obs_dtype != "float32" else obs.double(), seat=0)
    e.close()


# ---------------------------------------------------------------------------------------------- the fixture: QNetwork.forward
@gpu
def test_fixture_forward_is_the_model_bit_for_bit_and_within_the_counted_bound(env):
    import torch
    d = load_golden("dqn_agent.npz")
    params, x = (d["a_w1"], d["a_b1"], d["a_w2"], d["a_b2"]), d["a_x"]
    net = torch.nn.Sequential(torch.nn.Linear(105, 48), torch.nn.ReLU(), torch.nn.Linear(48, 132), torch.nn.ReLU()).to(env.device)
    with torch.no_grad():
        for t, v in zip((net[0].weight, net[0].bias, net[2].weight, net[2].bias), params):
            t.copy_(torch.as_tensor(v))
    qnet = env.dqn_qnet(net)
    assert qnet.final_relu is True and qnet.h1 == 48
    got = qnet.rows(torch.as_tensor(x).to(env.device)).cpu().numpy()
    assert np.array_equal(got, dm.forward(x, params, True))
    q64, e2 = dm.forward_f64(x, params, True), dm.error_bound(x, params)
    assert (np.abs(got.astype(np.float64) - q64) <= e2).all() and (np.abs(got.astype(np.float64) - d["a_q"]) <= 2 * e2).all()


# ---------------------------------------------------------------------------------------------- evg_dqn_actions
@gpu
def test_dqn_actions_equals_the_fixture(evg, env):
    import torch
    d = load_golden("dqn_agent.npz")
    q, want = d["b_q"], d["b_rows"]
    M, N = q.shape[0], 37
    covered = np.zeros(M, bool)
    for lo in list(range(0, M - N, N)) + [M - N]:
        out = torch.full((N, 7, 2), -1, dtype=torch.int32, device=env.device)
        rows = env.dqn_actions(torch.as_tensor(q[lo:lo + N]).to(env.device), out=out)
        assert rows is out and np.array_equal(rows.cpu().numpy(), want[lo:lo + N]), lo
        covered[lo:lo + N] = True
    assert covered.all()
    for n, lo in ((1, 100), (65, 240)):             # one env; a full wavefront and one env of a second workgroup
        e = evg.EvergladesVecEnv(n, seed=1)
        e.reset()
        rows = e.dqn_actions(torch.as_tensor(q[lo:lo + n]).to(e.device))
        assert np.array_equal(rows.cpu().numpy(), want[lo:lo + n]) and np.array_equal(want[lo:lo + n], np.stack([dm.filter_actions(r) for r in q[lo:lo + n]]))
        e.close()


# ---------------------------------------------------------------------------------------------- evg_dqn_get_action
@gpu
@pytest.mark.parametrize("seat", [0, 1])
def test_dqn_get_action_equals_the_model_and_the_fixture(evg, seat):
    """Rows m of the fixture become envs m of three handles of N = 37 (the fixture's agent of row m is env id m, episode c_episode[m], turn c_turn[m]:
    the handles' state is set to that).  Per-env epsilon -- with the row whose epsilon equals its coin --, then scalar epsilon 0, 0.3 and 1."""
    import torch
    g = load_golden("dqn_agent.npz")
    N, seed, M = 37, int(g["c_seed"][0]), g["c_eps"].shape[0]
    for lo in (0, 37, M - N):
        sl = slice(lo, lo + N)
        e = evg.EvergladesVecEnv(N, seed=seed, env_id_base=lo, auto_reset=False)
        e.reset()
        st = e.get_state()
        st["env"][:, 0] = g["c_turn"][sl]
        st["env"][:, 2] = g["c_episode"][sl]
        e.set_state(st["groups"], st["nodes"], st["health"], st["env"])
        qh = g["b_q"][sl]
        q = torch.as_tensor(qh).to(e.device).contiguous()
        eps = g["c_eps"][sl, seat]
        ids = np.arange(lo, lo + N)
        want, want_x = dm.get_action(qh, seed, ids, g["c_episode"][sl], g["c_turn"][sl], seat, eps)
        assert np.array_equal(want, g["c_rows"][sl, seat]) and np.array_equal(want_x, g["c_explored"][sl, seat])
        x = torch.full((N,), 7, dtype=torch.uint8, device=e.device)
        out = torch.full((N, 7, 2), -1, dtype=torch.int32, device=e.device)
        rows = e.dqn_get_action(q, torch.as_tensor(eps).to(e.device), seat=seat, out=out, explored=x)            # per-env epsilon
        assert rows is out and np.array_equal(rows.cpu().numpy(), want) and np.array_equal(x.cpu().numpy(), want_x)
        for level in (0.0, 0.3, 1.0):                                                                             # scalar epsilon
            w, wx = dm.get_action(qh, seed, ids, g["c_episode"][sl], g["c_turn"][sl], seat, np.full(N, level, np.float32))
            x.fill_(7)
            rows = e.dqn_get_action(q, level, seat=seat, explored=x)
            assert np.array_equal(rows.cpu().numpy(), w) and np.array_equal(x.cpu().numpy(), wx), level
            assert wx.all() if level == 1.0 else not wx.all()
        e.close()


# ---------------------------------------------------------------------------------------------- determinism, parameters read in place
@gpu
def test_two_calls_are_bit_equal_and_parameters_are_read_in_place(env):
    import torch
    params = _net(528, 51)
    dev = _device(env, params)
    qnet = env.dqn_qnet(dev, final_relu=False)
    x = torch.as_tensor(_x(300, 52)).to(env.device)
    a = qnet.rows(x).clone()
    b = qnet.rows(x)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert qnet.rows(x).data_ptr() == b.data_ptr()                  # nothing is allocated after the first call of a shape
    dev[3].add_(1.0)                                                # b2 += 1: with no final ReLU every Q moves by the last addend's change
    dev[0][5].zero_()
    params[3] = params[3] + np.float32(1.0)
    params[0][5] = 0
    assert np.array_equal(qnet.rows(x).cpu().numpy(), dm.forward(x.cpu().numpy(), params, False))
    assert not torch.equal(a, qnet.rows(x))


# ---------------------------------------------------------------------------------------------- end to end
@gpu
def test_acting_loop_equals_the_model_fed_loop_turn_for_turn(evg):
    """40 turns at N = 37, h1 = 32, auto_reset: obs -> dqn_qnet -> dqn_get_action(0.3) -> step_vs("random_actions") on one handle; on a second handle the
    MODEL's rows, computed from that handle's own observations, are fed to the same step_vs.  Observations, rewards and dones are equal at every turn.
    Both start at turn 128 of their first episode, so every env ends it (turn 150) inside the run and plays the start of its next one."""
    import torch
    N, seed, h1 = 37, 77, 32
    params = _net(h1, 61)
    envs = []
    for _ in range(2):
        e = evg.EvergladesVecEnv(N, seed=seed, auto_reset=True)
        e.reset()
        st = e.get_state()
        st["env"][:, 0] = 128
        e.set_state(st["groups"], st["nodes"], st["health"], st["env"])
        envs.append(e)
    dev_env, ref_env = envs
    qnet = dev_env.dqn_qnet(_device(dev_env, params), final_relu=True)
    obs_d, obs_r = dev_env.observe_seat(0), ref_env.observe_seat(0)
    ids, ended = np.arange(N), 0
    for t in range(40):
        assert torch.equal(obs_d, obs_r), t
        rows_d = dev_env.dqn_get_action(qnet(obs_d), 0.3, seat=0)
        o = obs_r.cpu().numpy()
        episodes = ref_env.get_state()["env"][:, 2]
        rows_m, _ = dm.get_action(dm.forward(o.astype(np.float32), params, True), seed, ids, episodes, o[:, 0].astype(np.int64), 0, np.full(N, 0.3, np.float32))
        assert np.array_equal(rows_d.cpu().numpy(), rows_m), t
        obs_d, rew_d, done_d, _ = dev_env.step_vs("random_actions", rows_d, seat=0)
        obs_r, rew_r, done_r, _ = ref_env.step_vs("random_actions", torch.as_tensor(rows_m).to(ref_env.device), seat=0)
        assert torch.equal(rew_d, rew_r) and torch.equal(done_d, done_r), t
        ended += int(done_d.sum())
    assert torch.equal(obs_d, obs_r) and ended >= N
    for e in envs:
        e.close()
