"""GPU tests of Minimized self-play in one launch: env.step_q with the 11-way head (evg_step_minimized_q) and its league form with a network member
(evg_step_league_minimized_q).  The reference side of every comparison uses none of the two: a second handle plays minimized_get_action for both seats,
step and smart_state_compact for both players; in the league tests the members' bots are consulted through scripted_actions with their objects moved in
and out (get_run_state / set_run_state) and the host model (tests/league_model.py) decides assignment, tally and swap.

Sizes: 32 envs per wavefront and 4 envs per decode pass, so N = 37 is a full wave plus a 5-env tail whose last pass is partial, N = 70 two waves plus 6."""
import ctypes as C

import numpy as np
import pytest

import league_model as lm
import minimized_model as mm
import minimized_self_play_cases as cases

gpu = pytest.mark.gpu
MEMBERS4 = ["swarm_agent", "cycle_rush_turn25", "random_actions_delay", "cycle_rush_turn25"]      # a league without a network member
WEIGHTS4 = [1.0, 0.0, 2.0, 1.5]


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


def _q(torch, n, gen, dev):
    """both seats' values on a grid of halves: exact ties within a swarm and between swarms are common"""
    return (torch.randn((n, 2, 12, 11), generator=gen) * 2.0).round().div(2.0).to(dev)


def _eps_of(torch, eps, p):
    return eps[:, p].contiguous() if isinstance(eps, torch.Tensor) else eps[p]


class _Buffers(object):
    """the outputs of one side, sentinel-filled"""

    def __init__(self, torch, n, dev, fill):
        self.feat = (torch.full((n, 2, 34), float(fill), device=dev), torch.full((n, 2, 12, 13), float(fill), device=dev))
        self.rows = torch.full((n, 2, 7, 2), fill, dtype=torch.int32, device=dev)
        self.ex = torch.full((n, 2), 9, dtype=torch.uint8, device=dev)


def _same_turn(torch, got, want, ga, gb, features, what):
    (o1, r1, d1, i1), (o2, r2, d2, i2) = got, want
    assert torch.equal(ga.rows, gb.rows), (what, "rows played")
    assert torch.equal(ga.ex, gb.ex), (what, "explored")
    assert torch.equal(o1, o2), (what, "obs")
    assert torch.equal(r1, r2) and torch.equal(d1, d2), (what, "reward / done")
    for k in ("winner", "scores", "status"):
        assert torch.equal(i1[k], i2[k]), (what, k)
    if features:
        assert torch.equal(ga.feat[0], gb.feat[0]) and torch.equal(ga.feat[1], gb.feat[1]), (what, "features")


def _same_handles(a, b, agents_b=None):
    s1, s2 = a.get_state(), b.get_state()
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), ("state", k)
    r1, r2 = a.get_run_state(), b.get_run_state()
    if agents_b is not None:
        r2["agents"] = agents_b
    assert sorted(r1) == sorted(r2)
    for k in r1:
        assert np.array_equal(np.asarray(r1[k]), np.asarray(r2[k]), equal_nan=True), ("run state", k)


# ---------------------------------------------------------------------------------------------- A: evg_step_minimized_q
def _five_calls(torch, env, q, eps, buf, features):
    """minimized_get_action for seat 0 and seat 1, step with both seats' rows, smart_state_compact for both players"""
    n = env.num_envs
    rows = [torch.zeros((n, 7, 2), dtype=torch.int32, device=env.device) for _ in range(2)]
    ex = [torch.zeros(n, dtype=torch.uint8, device=env.device) for _ in range(2)]
    for p in range(2):
        env.minimized_get_action(q[:, p].contiguous(), _eps_of(torch, eps, p), seat=p, out=rows[p], explored=ex[p])
    buf.rows.copy_(torch.stack(rows, dim=1))
    buf.ex.copy_(torch.stack(ex, dim=1))
    out = env.step(buf.rows)
    if features:
        for p in range(2):
            s, w = env.smart_state_compact(p, out[0])
            buf.feat[0][:, p].copy_(s)
            buf.feat[1][:, p].copy_(w)
    return out


@gpu
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("N", cases.SIZES)
def test_step_q_eleven_way_head_equals_its_five_call_composition(evg, N, dtype):
    import torch
    seed, turns = 4242 + N, 160
    a = evg.EvergladesVecEnv(N, seed=seed, obs_dtype=dtype, auto_reset=True)
    b = evg.EvergladesVecEnv(N, seed=seed, obs_dtype=dtype, auto_reset=True)
    a.reset(), b.reset()
    dev = a.device
    ga, gb = _Buffers(torch, N, dev, -7), _Buffers(torch, N, dev, -5)
    eps_env = torch.stack([torch.linspace(0.0, 1.0, N), torch.linspace(1.0, 0.0, N)], dim=1).contiguous().to(dev)
    gen = torch.Generator(device="cpu").manual_seed(N)
    ends = 0
    seen = np.zeros((2, 2), bool)                     # [seat][explored] met on some turn
    for t in range(turns):
        q = _q(torch, N, gen, dev)
        eps = eps_env if t % 2 else (0.3, 0.0)
        features = t % 3 != 0
        got = a.step_q(q, eps, features=ga.feat if features else None, explored=ga.ex, actions_out=ga.rows)
        want = _five_calls(torch, b, q, eps, gb, features)
        _same_turn(torch, got, want, ga, gb, features, (N, dtype, t))
        ends += int(got[2].sum().item())
        x = _np(ga.ex)
        for p in range(2):
            seen[p, 0] |= bool((x[:, p] == 0).any())
            seen[p, 1] |= bool((x[:, p] == 1).any())
    assert ends >= N and seen.all()                   # episodes ended; both seats explored on some turns and did not on others
    _same_handles(a, b)
    a.close(), b.close()


@gpu
def test_step_q_eleven_way_head_nan_and_inf_rows_follow_the_model(evg):
    import torch
    N = 37
    rng = np.random.RandomState(5)
    q = (np.round(rng.standard_normal((N, 2, 12, 11)) * 2) / 2).astype(np.float32)
    q[rng.rand(N, 2, 12, 11) < 0.05] = np.nan
    q[rng.rand(N, 2, 12, 11) < 0.05] = np.inf
    q[rng.rand(N, 2, 12, 11) < 0.05] = -np.inf
    q[3] = 0.0
    q[4, 1] = np.nan
    env = evg.EvergladesVecEnv(N, seed=9)
    env.reset()
    rows = torch.full((N, 2, 7, 2), -1, dtype=torch.int32, device=env.device)
    ex = torch.full((N, 2), 9, dtype=torch.uint8, device=env.device)
    for _ in range(3):
        env.step_q(torch.as_tensor(q).to(env.device), 0.0, actions_out=rows, explored=ex)
        want = np.stack([np.stack([mm.best_actions(q[e, p]) for p in range(2)]) for e in range(N)])
        assert np.array_equal(_np(rows), want) and not _np(ex).any()
    env.close()


# ---------------------------------------------------------------------------------------------- B: evg_step_league_minimized_q
class _LeagueComposition(object):
    """The league turn with a network member without a league entry point (the method of tests/test_gpu_league.py's _Composition): the caller's seat and
    the network member's envs take minimized_get_action rows; per bot member in use, the member's objects are moved in (set_run_state), its bot consulted
    (scripted_actions), the advanced objects moved out (get_run_state); step() plays; the host model tallies, draws and swaps at the episode boundaries.
    The network member's objects do not advance."""

    def __init__(self, evg, n, seat, dtype, members, weights, auto_reset=True, seed=cases.SEED, env_id_base=0):
        import torch
        self.torch, self.n, self.seat = torch, n, seat
        self.env = evg.EvergladesVecEnv(n, seed=seed, env_id_base=env_id_base, obs_dtype=dtype, auto_reset=auto_reset)
        self.qm = members.index("q") if "q" in members else -1
        self.ids = [self.env.POLICIES["no_action" if m == "q" else m] for m in members]
        self.env.reset()
        self.model = lm.League(seed, env_id_base, n, len(members), seat, True, weights)
        self.model.clear(np.zeros(n, np.int64))
        self.live = np.tile(np.asarray(lm.FRESH, np.uint32), (n, 1))
        self.episode = np.zeros(n, np.int64)
        self.frozen = np.zeros(n, bool)
        self.bot = torch.zeros((n, 2, 7, 2), dtype=torch.int32, device=self.env.device)
        self.bot_played = 0

    def agents(self):
        a = self.env.get_run_state()["agents"]
        a[:, 1 - self.seat] = self.live
        return a

    def step(self, q, eps, buf, features):
        torch, env, p = self.torch, self.env, 1 - self.seat
        dev = env.device
        member = np.array([self.model.member(e) for e in range(self.n)])
        base = env.get_run_state()["agents"]
        rows = [torch.zeros((self.n, 7, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        ex = [torch.zeros(self.n, dtype=torch.uint8, device=dev) for _ in range(2)]
        for s in range(2):
            env.minimized_get_action(q[:, s].contiguous(), _eps_of(torch, eps, s), seat=s, out=rows[s], explored=ex[s])
        by_net = torch.as_tensor(member == self.qm, device=dev)
        for m in sorted(set(member.tolist()) - {self.qm}):
            a = base.copy()
            a[:, p] = self.live
            env.set_run_state(agents=a)
            env.scripted_actions(self.ids[m], p, out=self.bot)
            sel = torch.as_tensor(member == m, device=dev)
            rows[p] = torch.where(sel[:, None, None], self.bot[:, p], rows[p])
            after = env.get_run_state()["agents"][:, p]
            mine = (member == m) & ~self.frozen
            self.live[mine] = after[mine]
        # a frozen env's bot is not consulted: zero rows
        idle = torch.as_tensor((member != self.qm) & self.frozen, device=dev)
        rows[p] = torch.where(idle[:, None, None], torch.zeros_like(rows[p]), rows[p])
        ex[p] = torch.where(by_net, ex[p], torch.full_like(ex[p], 2))
        self.bot_played += int((member != self.qm).sum())
        a = base.copy()
        a[:, p] = self.live
        env.set_run_state(agents=a)
        buf.rows.copy_(torch.stack(rows, dim=1))
        buf.ex.copy_(torch.stack(ex, dim=1))
        out = env.step(buf.rows)
        if features:
            for s in range(2):
                sh, sw = env.smart_state_compact(s, out[0])
                buf.feat[0][:, s].copy_(sh)
                buf.feat[1][:, s].copy_(sw)
        d, w = _np(out[2]).astype(bool), _np(out[3]["winner"])
        for e in np.nonzero(d & ~self.frozen)[0]:
            self.model.tally(e, int(w[e]))
            if env.auto_reset:
                self.episode[e] += 1
                _, self.live[e] = self.model.start_episode(e, int(self.episode[e]), self.live[e].copy())
            else:
                self.frozen[e] = True
        return out


def _same_league(league, comp):
    st = league.state()
    assert np.array_equal(st["assign"], comp.model.assign)
    assert np.array_equal(st["objects"], comp.model.objects)
    assert np.array_equal(st["counts"], comp.model.counts)
    assert league.status() == comp.model.status


@gpu
@pytest.mark.parametrize("seat", [0, 1])
@pytest.mark.parametrize("N", cases.SIZES)
def test_league_with_a_network_member_equals_the_composition(evg, N, seat):
    """cases.TURNS turns with auto-reset: at least four episodes per env, over which (tests/test_minimized_self_play_abi.py, on the host model) every member
    of non-zero weight is played and some env leaves the network member and returns to it.  float32 observations at N = 37, int16 at N = 70."""
    import torch
    dtype = "float32" if N == 37 else "int16"
    env = evg.EvergladesVecEnv(N, seed=cases.SEED, obs_dtype=dtype, auto_reset=True)
    env.reset()
    league = env.opponent_league(cases.MEMBERS, weights=cases.WEIGHTS, seat=seat)
    assert league.q_member == 0 and league.members[0] == env.POLICIES["no_action"]
    comp = _LeagueComposition(evg, N, seat, dtype, cases.MEMBERS, cases.WEIGHTS)
    dev = env.device
    ga, gb = _Buffers(torch, N, dev, -7), _Buffers(torch, N, dev, -5)
    eps_env = torch.stack([torch.linspace(0.0, 1.0, N), torch.linspace(1.0, 0.0, N)], dim=1).contiguous().to(dev)
    gen = torch.Generator(device="cpu").manual_seed(N + seat)
    assert np.array_equal(_np(league.assign), comp.model.assign)
    twos = 0
    for t in range(cases.TURNS):
        q = _q(torch, N, gen, dev)
        eps = eps_env if t % 2 else (0.3, 0.1)
        features = t % 3 != 0
        got = env.step_q(q, eps, features=ga.feat if features else None, explored=ga.ex, actions_out=ga.rows, league=league)
        want = comp.step(q, eps, gb, features)
        _same_turn(torch, got, want, ga, gb, features, (N, seat, t))
        twos += int((ga.ex[:, 1 - seat] == 2).sum().item())
        assert int(ga.ex[:, seat].max().item()) <= 1
        if t % 10 == 9 or bool(got[2].any()):
            assert np.array_equal(_np(league.assign), comp.model.assign), t
    h = comp.model.history
    assert min(len(a) for a in h) >= cases.EPISODES
    assert [a[:cases.EPISODES] for a in h] == cases.model_histories(N, seat)
    assert 0 < twos == comp.bot_played < N * cases.TURNS
    _same_handles(env, comp.env, comp.agents())
    _same_league(league, comp)
    assert int(league.counts[:, 0].sum()) == int(env.episode_stats()["totals"][0]) >= 3 * N
    env.close(), comp.env.close()


@gpu
def test_league_without_auto_reset_marks_bot_turns_and_zeroes_frozen_bot_rows(evg):
    """one episode without auto-reset, then ten turns on the frozen games: explored is 2 exactly where a bot holds the league seat; a frozen bot-played env
    shows seven {0, 0} rows, a frozen network-played env still shows the network's rows"""
    import torch
    N, seat = 37, 0
    env = evg.EvergladesVecEnv(N, seed=cases.SEED, auto_reset=False)
    env.reset()
    league = env.opponent_league(cases.MEMBERS_FROZEN, seat=seat)
    comp = _LeagueComposition(evg, N, seat, "float32", cases.MEMBERS_FROZEN, None, auto_reset=False)
    dev = env.device
    ga, gb = _Buffers(torch, N, dev, -7), _Buffers(torch, N, dev, -5)
    gen = torch.Generator(device="cpu").manual_seed(77)
    assign = comp.model.assign.copy()
    by_net = assign == cases.MEMBERS_FROZEN.index("q")
    assert by_net.any() and len(set(assign.tolist())) == 4            # every member holds some env
    for t in range(160):
        q = _q(torch, N, gen, dev)
        got = env.step_q(q, (0.2, 0.2), features=ga.feat, explored=ga.ex, actions_out=ga.rows, league=league)
        want = comp.step(q, (0.2, 0.2), gb, True)
        _same_turn(torch, got, want, ga, gb, True, t)
        assert np.array_equal(_np(ga.ex[:, 1]) == 2, ~by_net), t
    assert comp.frozen.all()
    rows = _np(ga.rows)
    assert not rows[~by_net, 1].any()                                    # frozen, bot-played: zero rows
    assert (rows[by_net, 1, :, 1] >= 1).all() and (rows[:, 0, :, 1] >= 1).all()     # the network's rows name nodes 1..11
    assert np.array_equal(_np(league.assign), assign)
    _same_handles(env, comp.env, comp.agents())
    _same_league(league, comp)
    env.close(), comp.env.close()


@gpu
@pytest.mark.parametrize("seat", [0, 1])
def test_league_without_a_network_member_equals_the_one_seat_league_turn(evg, seat):
    """q_member = -1: every league env is bot-played.  The caller's seat sees what step_vs_q(league, q[:, seat]) shows on a second handle with a league of
    its own (evg_step_vs_league_minimized_q); the league seat's explored flags are all 2."""
    import torch
    N, turns, p = 70, 170, 1 - seat
    envs, leagues = [], []
    for _ in range(2):
        env = evg.EvergladesVecEnv(N, seed=cases.SEED, auto_reset=True)
        env.reset()
        envs.append(env)
        leagues.append(env.opponent_league(MEMBERS4, weights=WEIGHTS4, seat=seat))
    a, b = envs
    assert leagues[0].q_member == -1
    dev = a.device
    ga = _Buffers(torch, N, dev, -7)
    fb = (torch.zeros((N, 34), device=dev), torch.zeros((N, 12, 13), device=dev))
    rb, xb = torch.zeros((N, 7, 2), dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    eps_env = torch.stack([torch.linspace(0.0, 1.0, N), torch.linspace(1.0, 0.0, N)], dim=1).contiguous().to(dev)
    gen = torch.Generator(device="cpu").manual_seed(5 + seat)
    ends = 0
    for t in range(turns):
        q = _q(torch, N, gen, dev)
        eps = eps_env if t % 2 else (0.3, 0.1)
        got = a.step_q(q, eps, features=ga.feat, explored=ga.ex, actions_out=ga.rows, league=leagues[0])
        want = b.step_vs_q(leagues[1], q[:, seat].contiguous(), _eps_of(torch, eps, seat), seat=seat, features=fb, explored=xb, actions_out=rb)
        assert torch.equal(ga.rows[:, seat], rb) and torch.equal(ga.ex[:, seat], xb), t
        assert bool((ga.ex[:, p] == 2).all()), t
        assert torch.equal(got[0][:, seat], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), t
        for k in ("winner", "scores", "status"):
            assert torch.equal(got[3][k], want[3][k]), (t, k)
        assert torch.equal(ga.feat[0][:, seat], fb[0]) and torch.equal(ga.feat[1][:, seat], fb[1]), t
        if t % 20 == 19:                                               # the league seat's observation and features: those of the state
            assert torch.equal(got[0], b.observe()), t
            sh, sw = b.smart_state_compact(p, b.obs)
            assert torch.equal(ga.feat[0][:, p], sh) and torch.equal(ga.feat[1][:, p], sw), t
        ends += int(got[2].sum().item())
    assert ends >= N
    _same_handles(a, b)
    l1, l2 = leagues[0].state(), leagues[1].state()
    for k in ("assign", "objects", "counts", "ctl"):
        assert np.array_equal(l1[k], l2[k]), k
    a.close(), b.close()


@gpu
def test_league_run_resumes_from_a_checkpoint_bit_for_bit(evg):
    import torch
    N, seat = 37, 1
    a = evg.EvergladesVecEnv(N, seed=cases.SEED, auto_reset=True)
    a.reset()
    la = a.opponent_league(cases.MEMBERS, weights=cases.WEIGHTS, seat=seat)
    dev = a.device
    ga, gc = _Buffers(torch, N, dev, -7), _Buffers(torch, N, dev, -5)
    gen = torch.Generator(device="cpu").manual_seed(11)
    for t in range(165):                                               # past the first episode boundary: members were redrawn, objects swapped
        a.step_q(_q(torch, N, gen, dev), (0.3, 0.1), features=ga.feat, explored=ga.ex, actions_out=ga.rows, league=la)
    assert int(a.episode_stats()["totals"][0]) >= N
    ck, lst = a.checkpoint(), la.state()
    c = evg.EvergladesVecEnv(N, seed=cases.SEED, auto_reset=True)
    c.reset()
    lc = c.opponent_league(cases.MEMBERS, weights=cases.WEIGHTS, seat=seat)
    c.restore(ck)
    lc.load_state(lst)
    for t in range(150):
        q = _q(torch, N, gen, dev)
        got = a.step_q(q, (0.3, 0.1), features=ga.feat, explored=ga.ex, actions_out=ga.rows, league=la)
        want = c.step_q(q, (0.3, 0.1), features=gc.feat, explored=gc.ex, actions_out=gc.rows, league=lc)
        _same_turn(torch, got, want, ga, gc, True, t)
    _same_handles(a, c)
    l1, l2 = la.state(), lc.state()
    for k in ("assign", "objects", "counts", "ctl"):
        assert np.array_equal(l1[k], l2[k]), k
    assert int(l1["counts"][:, 0].sum()) >= 2 * N
    a.close(), c.close()


# ---------------------------------------------------------------------------------------------- bad input
@gpu
def test_bad_input_is_refused_with_nothing_launched(evg):
    import torch
    from everglades_amd import _lib
    N = 37
    env = evg.EvergladesVecEnv(N, seed=2)
    env.reset()
    dev, L, vp = env.device, env.L, C.c_void_p
    league = env.opponent_league(cases.MEMBERS, weights=cases.WEIGHTS, seat=0)
    q = torch.zeros((N * 2 * 12 * 11 + 4,), device=dev)
    q4 = q[:N * 2 * 12 * 11].view(N, 2, 12, 11)
    obs = torch.full((N, 2, 105), 7.0, device=dev)
    rows = torch.full((N, 2, 7, 2), -5, dtype=torch.int32, device=dev)
    ex = torch.full((N, 2), 9, dtype=torch.uint8, device=dev)
    shared = torch.full((N, 2, 34), 7.0, device=dev)
    p = env._p
    before = env.get_state()

    def plain(h=None, qptr=None, e0=0.5, e1=0.5, sh=None, sw=None, pp=None):
        pp = p if pp is None else pp
        return L.evg_step_minimized_q(env._h if h is None else h, vp(q.data_ptr() if qptr is None else qptr), e0, e1, None, vp(obs.data_ptr()), sh, sw,
                                      vp(rows.data_ptr()), vp(ex.data_ptr()), pp["reward"], pp["done"], pp["winner"], pp["scores"], pp["status"],
                                      env._stream())

    def with_league(h=None, qptr=None, e0=0.5, e1=0.5, sh=None, sw=None, qm=0, ref=None):
        return L.evg_step_league_minimized_q(env._h if h is None else h, vp(q.data_ptr() if qptr is None else qptr), e0, e1, None,
                                             league._ref if ref is None else ref, qm, vp(obs.data_ptr()), sh, sw, vp(rows.data_ptr()), vp(ex.data_ptr()),
                                             p["reward"], p["done"], p["winner"], p["scores"], p["status"], env._stream())
    for call in (plain, with_league):
        assert call(qptr=q.data_ptr() + 4) == _lib.ERR_ARG                 # misaligned q
        assert call(e0=1.5) == _lib.ERR_ARG and call(e1=-0.25) == _lib.ERR_ARG and call(e1=float("nan")) == _lib.ERR_ARG
        assert call(sh=vp(shared.data_ptr())) == _lib.ERR_ARG              # shared_out without swarm_out
    assert with_league(qm=len(cases.MEMBERS)) == _lib.ERR_ARG and with_league(qm=-2) == _lib.ERR_ARG
    stock = evg.EvergladesVecEnv(N, seed=2, rng_mode="mt19937")
    stock.reset()
    assert plain(h=stock._h, pp=stock._p) == _lib.ERR_ARG
    assert with_league(h=stock._h) == _lib.ERR_ARG
    with pytest.raises(ValueError):
        env.step_q(q4, 0.5, directions=torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        env.step_q(q4, 0.5, directions=torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=dev), league=league)
    with pytest.raises(ValueError):
        env.step_vs_q(league, q4[:, 0].contiguous(), 0.5)                   # a league with a network member has no one-seat form
    with pytest.raises(ValueError):
        env.step_vs(league, torch.zeros((N, 7, 2), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        env.step_q(torch.zeros((N, 2, 12, 5), device=dev), 0.5, league=league)
    with pytest.raises(ValueError):
        env.opponent_league(["q", "q", "swarm_agent"])
    torch.cuda.synchronize()
    assert float(obs.min()) == 7.0 and int(rows.max()) == -5 and int(ex.min()) == 9 and float(shared.min()) == 7.0       # nothing ran
    after = env.get_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert not league.counts.any().item()
    stock.close()
    env.close()


# ---------------------------------------------------------------------------------------------- the example
@gpu
@pytest.mark.parametrize("staggered", [False, True])
def test_self_play_example_runs_with_finite_losses(staggered):
    import os
    import sys
    import torch
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import minimized_self_play
    losses = minimized_self_play.main(2048, 60, 256, staggered=staggered)
    assert tuple(losses.shape) == (60 - 2, 2) and bool(torch.isfinite(losses).all())
