"""GPU tests of the opponent league (everglades_amd.OpponentLeague; evg_league_* and evg_step_vs_league(_q)): a per-env scripted opponent, redrawn by weight each
episode.  The contract is a composition of entry points that are pinned to the reference already: the reference side of every comparison uses NO league entry
point -- a second handle driven through scripted_actions(member, 1 - seat) + step (or a plain step_vs(member) handle), get_run_state / set_run_state moving a
member's object in and out, and the host model (tests/league_model.py) deciding the assignment and the tally."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import league_model as lm
from conftest import ROOT

gpu = pytest.mark.gpu

N_SMALL, SEED = 333, 20260917
MEMBERS4 = ["swarm_agent", "cycle_rush_turn25", "random_actions_delay", "cycle_rush_turn25"]     # an RNG bot, a cycling bot, a delay-coin bot, one id repeated
WEIGHTS4 = [1.0, 0.0, 2.0, 1.5]


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


def _rows(torch, n, gen, device):
    """a caller's 7 order rows per env: any group, any node of its own numbering"""
    g = torch.randint(0, 12, (n, 7, 1), generator=gen, device=device, dtype=torch.int32)
    d = torch.randint(1, 12, (n, 7, 1), generator=gen, device=device, dtype=torch.int32)
    return torch.cat([g, d], dim=2).contiguous()


def _model_histories(n, seat, episodes=4):
    """the members every env plays in its first `episodes` episodes, from the host model alone"""
    m = lm.League(SEED, 0, n, len(MEMBERS4), seat, True, WEIGHTS4)
    m.clear(np.zeros(n, np.int64))
    for k in range(1, episodes):
        for e in range(n):
            m.start_episode(e, k, np.asarray(lm.FRESH, np.uint32))
    return m.history


@pytest.mark.parametrize("seat", [0, 1])
def test_the_chosen_seed_changes_members_and_returns_to_earlier_ones(seat):
    """(CPU) what the bit-for-bit test below relies on: with SEED some env changes its member and some env returns to a member it played before, and the
    zero-weight member is never drawn"""
    h = _model_histories(N_SMALL, seat)
    assert any(a[0] != a[1] for a in h)
    assert any(a[2] != a[1] and a[2] in a[:1] for a in h) or any(a[3] != a[2] and a[3] in a[:2] for a in h)
    assert all(1 not in a for a in h)
    assert {x for a in h for x in a} == {0, 2, 3}


class _Composition(object):
    """The league's turn without a league entry point: per member in use, the member's objects moved into a second handle (set_run_state), its bot consulted
    (scripted_actions), the advanced objects moved out (get_run_state); then step() on the caller's rows and each env's member's rows; the host model tallies,
    draws and swaps at the episode boundaries."""

    def __init__(self, evg, n, seat, dtype, members, weights, resample, auto_reset=True, assign=None, seed=SEED, env_id_base=0):
        import torch
        self.torch, self.n, self.seat = torch, n, seat
        self.env = evg.EvergladesVecEnv(n, seed=seed, env_id_base=env_id_base, obs_dtype=dtype, auto_reset=auto_reset)
        self.ids = [self.env.POLICIES[m] for m in members]
        self.env.reset()
        self.model = lm.League(seed, env_id_base, n, len(members), seat, resample, weights)
        if assign is not None:
            self.model.assign[:] = assign
        self.model.clear(np.zeros(n, np.int64))
        self.live = np.tile(np.asarray(lm.FRESH, np.uint32), (n, 1))
        self.episode = np.zeros(n, np.int64)
        self.frozen = np.zeros(n, bool)
        self.actions = torch.zeros((n, 2, 7, 2), dtype=torch.int32, device=self.env.device)
        self.bot = torch.zeros((n, 2, 7, 2), dtype=torch.int32, device=self.env.device)

    def agents(self):
        a = self.env.get_run_state()["agents"]
        a[:, 1 - self.seat] = self.live
        return a

    def step(self, rows):
        torch, env, p = self.torch, self.env, 1 - self.seat
        member = np.array([self.model.member(e) for e in range(self.n)])
        base = env.get_run_state()["agents"]
        self.actions[:, self.seat] = rows
        for m in sorted(set(member.tolist())):
            a = base.copy()
            a[:, p] = self.live
            env.set_run_state(agents=a)
            env.scripted_actions(self.ids[m], p, out=self.bot)
            sel = torch.as_tensor(member == m, device=env.device)
            self.actions[:, p] = torch.where(sel[:, None, None], self.bot[:, p], self.actions[:, p])
            after = env.get_run_state()["agents"][:, p]
            mine = (member == m) & ~self.frozen
            self.live[mine] = after[mine]
        a = base.copy()
        a[:, p] = self.live
        env.set_run_state(agents=a)
        obs, reward, done, info = env.step(self.actions)
        d, w = _np(done).astype(bool), _np(info["winner"])
        for e in np.nonzero(d & ~self.frozen)[0]:
            self.model.tally(e, int(w[e]))
            if env.auto_reset:
                self.episode[e] += 1
                _, self.live[e] = self.model.start_episode(e, int(self.episode[e]), self.live[e].copy())
            else:
                self.frozen[e] = True
        return obs[:, self.seat], reward, done, info

    def reset(self, mask):
        self.env.reset(mask)
        for e in np.nonzero(mask)[0]:
            self.episode[e] += 1
            self.frozen[e] = False
            _, self.live[e] = self.model.start_episode(e, int(self.episode[e]), self.live[e].copy())


def _same_outputs(torch, got, want, turn):
    (o1, r1, d1, i1), (o2, r2, d2, i2) = got, want
    assert torch.equal(o1, o2), turn
    assert torch.equal(r1, r2) and torch.equal(d1, d2), turn
    for k in ("winner", "scores", "status"):
        assert torch.equal(i1[k], i2[k]), (turn, k)


def _same_end_state(env, league, comp):
    s1, s2 = env.get_state(), comp.env.get_state()
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    r1, r2 = env.get_run_state(), comp.env.get_run_state()
    r2["agents"] = comp.agents()
    for k in r1:
        assert np.array_equal(r1[k], r2[k]), k
    st = league.state()
    assert np.array_equal(st["assign"], comp.model.assign)
    assert np.array_equal(st["objects"], comp.model.objects)
    assert np.array_equal(st["counts"], comp.model.counts)
    assert league.status() == comp.model.status


@gpu
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("seat", [0, 1])
def test_league_step_equals_the_composition_over_member_changes(evg, seat, dtype):
    import torch
    n, turns = N_SMALL, 470
    env = evg.EvergladesVecEnv(n, seed=SEED, obs_dtype=dtype, auto_reset=True)
    env.reset()
    league = env.opponent_league(MEMBERS4, weights=WEIGHTS4, seat=seat)
    comp = _Composition(evg, n, seat, dtype, MEMBERS4, WEIGHTS4, True)
    gen = torch.Generator(device=env.device).manual_seed(3)
    shared = torch.zeros((n, 34), device=env.device)
    swarm = torch.zeros((n, 12, 13), device=env.device)
    assert np.array_equal(_np(league.assign), comp.model.assign)
    for t in range(turns):
        rows = _rows(torch, n, gen, env.device)
        got = env.step_vs(league, rows, features=(shared, swarm) if t % 2 else None)
        want = comp.step(rows)
        _same_outputs(torch, got, want, t)
        if t % 2:
            s2, w2 = env.smart_state_compact(-1, got[0])
            assert torch.equal(shared, s2) and torch.equal(swarm, w2), t
        if t % 10 == 9 or bool(got[2].any()):
            assert np.array_equal(_np(league.assign), comp.model.assign), t
    h = comp.model.history
    assert max(len(a) for a in h) >= 4                                      # three full episodes
    assert any(a[i] != a[i + 1] for a in h for i in range(len(a) - 1))       # a member changed ...
    assert any(a[i] != a[i - 1] and a[i] in a[:i - 1] for a in h for i in range(2, len(a)))     # ... and one came back
    _same_end_state(env, league, comp)
    assert int(league.counts[:, 0].sum()) == int(env.episode_stats()["totals"][0]) >= 3 * n


@gpu
def test_league_q_form_equals_get_action_plus_the_league_step(evg):
    import torch
    n, seat, turns = N_SMALL, 1, 310
    envs, leagues = [], []
    for _ in range(2):
        env = evg.EvergladesVecEnv(n, seed=SEED, auto_reset=True)
        env.reset()
        envs.append(env)
        leagues.append(env.opponent_league(MEMBERS4, weights=WEIGHTS4, seat=seat))
    a, b = envs
    gen = torch.Generator(device=a.device).manual_seed(4)
    prev = b.observe_seat(seat).clone()
    feat = [(torch.zeros((n, 34), device=a.device), torch.zeros((n, 12, 13), device=a.device)) for _ in range(2)]
    outs = [[torch.zeros((n, 7, 2), dtype=torch.int32, device=a.device) for _ in range(2)] + [torch.zeros(n, dtype=torch.uint8, device=a.device)] for _ in range(2)]
    eps_env = torch.rand(n, generator=gen, device=a.device) * 0.4
    for t in range(turns):
        q = (torch.randn((n, 12, 5), generator=gen, device=a.device) * 2.0).round().div(2.0).contiguous()
        eps = eps_env if t % 3 == 0 else 0.1
        got = a.step_vs_q(leagues[0], q, eps, features=feat[0], actions_out=outs[0][0], directions=outs[0][1], explored=outs[0][2])
        b.smart_get_action(q, eps, seat=seat, obs=prev, out=outs[1][0], directions=outs[1][1], explored=outs[1][2])
        want = b.step_vs(leagues[1], outs[1][0], features=feat[1])
        _same_outputs(torch, got, want, t)
        for x, y in zip(outs[0] + list(feat[0]), outs[1] + list(feat[1])):
            assert torch.equal(x, y), t
        assert torch.equal(leagues[0].assign, leagues[1].assign), t
        prev = want[0].clone()
    s1, s2 = a.get_state(), b.get_state()
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    r1, r2 = a.get_run_state(), b.get_run_state()
    assert all(np.array_equal(r1[k], r2[k]) for k in r1)
    l1, l2 = leagues[0].state(), leagues[1].state()
    assert all(np.array_equal(l1[k], l2[k]) for k in l1)
    # (a game may end before turn 150: at least two episodes per env)
    assert int(l1["counts"][:, 0].sum()) == int(a.episode_stats()["totals"][0]) >= 2 * n and len(set(l1["assign"].tolist())) == 3


@gpu
def test_all_fifteen_at_once_with_a_fixed_assignment(evg):
    import torch
    n, turns, seat, M = 4096 + 37, 160, 0, 15
    env = evg.EvergladesVecEnv(n, seed=SEED, auto_reset=True)
    env.reset()
    league = env.opponent_league(lm.SCRIPT_MEMBERS, seat=seat, resample=False)
    assign = np.arange(n) % M
    league.assign.copy_(torch.as_tensor(assign.astype(np.uint8)))
    plain = []
    for m in range(M):
        e = evg.EvergladesVecEnv(n, seed=SEED, auto_reset=True)
        e.reset()
        plain.append(e)
    gen = torch.Generator(device=env.device).manual_seed(5)
    tally = np.zeros((M, 4), np.int64)
    sel = [torch.as_tensor(np.nonzero(assign == m)[0], device=env.device) for m in range(M)]
    for t in range(turns):
        rows = _rows(torch, n, gen, env.device)
        o, r, d, i = env.step_vs(league, rows)
        for m in range(M):
            o2, r2, d2, i2 = plain[m].step_vs(lm.SCRIPT_MEMBERS[m], rows)
            s = sel[m]
            assert torch.equal(o[s], o2[s]) and torch.equal(r[s], r2[s]) and torch.equal(d[s], d2[s]), (t, m)
            assert torch.equal(i["winner"][s], i2["winner"][s]) and torch.equal(i["scores"][s], i2["scores"][s]), (t, m)
        dn, wn = _np(d).astype(bool), _np(i["winner"])
        for m in range(M):
            fin = dn & (assign == m)
            tally[m] += [fin.sum(), (fin & (wn == seat)).sum(), (fin & (wn == 2)).sum(), (fin & (wn == 1 - seat)).sum()]
    counts = _np(league.counts)
    assert np.array_equal(counts, tally)
    assert counts[:, 0].sum() == env.episode_stats()["totals"][0] >= n
    assert np.array_equal(_np(league.assign), assign) and league.status() == 0
    s1 = env.get_state()
    for m in range(M):
        s2 = plain[m].get_state()
        idx = np.nonzero(assign == m)[0]
        assert all(np.array_equal(s1[k][idx], s2[k][idx]) for k in s1), m
        a1, a2 = env.get_run_state()["agents"], plain[m].get_run_state()["agents"]
        assert np.array_equal(a1[idx], a2[idx]), m


@pytest.fixture(scope="module")
def explicit_reset_run(evg):
    """auto_reset=False: a run to the end of every game and a few turns beyond, league and composition side by side (shared by the tests below)"""
    import torch
    n, seat = N_SMALL, 0
    env = evg.EvergladesVecEnv(n, seed=SEED, auto_reset=False)
    env.reset()
    league = env.opponent_league(MEMBERS4, weights=WEIGHTS4, seat=seat)
    comp = _Composition(evg, n, seat, "float32", MEMBERS4, WEIGHTS4, True, auto_reset=False)
    gen = torch.Generator(device=env.device).manual_seed(6)
    for t in range(154):
        rows = _rows(torch, n, gen, env.device)
        _same_outputs(torch, env.step_vs(league, rows), comp.step(rows), t)
    return env, league, comp, gen


@gpu
def test_explicit_reset_then_assign(evg, explicit_reset_run):
    import torch
    env, league, comp, gen = explicit_reset_run
    n = env.num_envs
    assert bool(env.done.all())
    # every game was tallied once (the frozen turns behind the end did not tally again), and a frozen env's bot was not consulted
    assert int(league.counts[:, 0].sum()) == n
    _same_end_state(env, league, comp)
    mask = (np.arange(n) % 3 != 1)
    env.reset(mask)
    league.assign_after_reset(mask)
    comp.reset(mask)
    _same_end_state(env, league, comp)
    assert (comp.model.assign[mask] != np.asarray([h[0] for h in comp.model.history])[mask]).any()
    for t in range(3):
        rows = _rows(torch, n, gen, env.device)
        _same_outputs(torch, env.step_vs(league, rows), comp.step(rows), t)
    _same_end_state(env, league, comp)


@gpu
def test_reweight_and_bad_input(evg, explicit_reset_run):
    import torch
    env, league, comp, gen = explicit_reset_run
    L, lib = evg._lib, env.L
    out = torch.zeros(4, dtype=torch.float64, device=env.device)
    counts = _np(league.counts)
    assert np.array_equal(_np(league.reweight(out)), lm.importance(counts)) and counts[:, 0].sum() > 0
    keep_w, keep_a = league.weights.clone(), league.assign.clone()
    for bad in ([0.0, 0.0, 0.0, 0.0], [1.0, float("inf"), 1.0, 1.0]):
        league._ctl.zero_()
        league.weights.copy_(torch.as_tensor(bad, dtype=torch.float64))
        league.assign_after_reset()
        assert league.status() == L.LEAGUE_S_BAD_WEIGHTS and torch.equal(league.assign, keep_a)
    league.weights.copy_(keep_w)
    league._ctl.zero_()
    league.reweight()                                    # in place: weights_out may be the league's own
    assert np.array_equal(_np(league.weights), lm.importance(counts))
    league.weights.copy_(keep_w)
    # assign = 200 under resample=False plays member 0 and says so
    n = 70
    a, b = [evg.EvergladesVecEnv(n, seed=SEED, auto_reset=True) for _ in range(2)]
    a.reset(), b.reset()
    fixed = a.opponent_league(["cycle_rush_turn50", "swarm_agent"], seat=0, resample=False)
    fixed.assign.fill_(200)
    for t in range(4):
        rows = _rows(torch, n, gen, env.device)
        _same_outputs(torch, a.step_vs(fixed, rows), b.step_vs("cycle_rush_turn50", rows), t)
    assert fixed.status() == L.LEAGUE_S_BAD_ASSIGN and int(fixed.assign[0]) == 200
    # descriptors out of range are refused before anything is enqueued
    rows = _rows(torch, n, gen, env.device)

    def refused(**kw):
        d = L.EvgLeague()
        C.memmove(C.byref(d), C.byref(fixed._desc), C.sizeof(d))
        for k, v in kw.items():
            if k == "member0":
                d.members[0] = v
            else:
                setattr(d, k, v)
        p = a._p
        rcs = [lib.evg_league_clear(a._h, C.byref(d), a._stream()), lib.evg_league_assign(a._h, C.byref(d), None, a._stream()),
               lib.evg_league_importance(a._h, C.byref(d), C.c_void_p(out.data_ptr()), a._stream()),
               lib.evg_step_vs_league(a._h, C.c_void_p(rows.data_ptr()), 0, C.byref(d), C.c_void_p(a._seat_buffers().data_ptr()), None, None, p["reward"],
                                      p["done"], p["winner"], p["scores"], p["status"], a._stream())]
        return rcs
    before = a.get_state()
    for kw in (dict(num_members=0), dict(num_members=17), dict(member0=15), dict(seat=2)):
        assert refused(**kw) == [L.ERR_ARG] * 4, kw
    after = a.get_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)


@gpu
def test_resume_continues_bit_for_bit(evg):
    import torch
    n, seat = 200, 0

    def make():
        env = evg.EvergladesVecEnv(n, seed=SEED, auto_reset=True)
        env.reset()
        return env, env.opponent_league(MEMBERS4, weights=WEIGHTS4, seat=seat)
    env, league = make()
    gen = torch.Generator(device=env.device).manual_seed(7)
    all_rows = [_rows(torch, n, gen, env.device) for _ in range(240)]
    for t in range(120):
        env.step_vs(league, all_rows[t])
    ck, st = env.checkpoint(), league.state()
    env2, league2 = make()
    for t in range(7):                                   # the fresh pair has a history of its own before it is restored
        env2.step_vs(league2, all_rows[t])
    env2.restore(ck)
    league2.load_state(st)
    for t in range(120, 240):
        got = env.step_vs(league, all_rows[t])
        want = env2.step_vs(league2, all_rows[t])
        _same_outputs(torch, got, want, t)
    s1, s2 = env.get_state(), env2.get_state()
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    r1, r2 = env.get_run_state(), env2.get_run_state()
    assert all(np.array_equal(r1[k], r2[k]) for k in r1 if k != "totals")
    l1, l2 = league.state(), league2.state()
    assert all(np.array_equal(l1[k], l2[k]) for k in l1)
    assert int(l1["counts"][:, 0].sum()) == int(env.episode_stats()["totals"][0]) >= n


@gpu
def test_the_example_runs_both_ways(evg):
    spec = importlib.util.spec_from_file_location("smart_state_league_training", os.path.join(ROOT, "examples", "smart_state_league_training.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    counts, rates = ex.main(num_envs=150, turns=160, batch=64, reweight_every=75, verbose=False)
    assert counts[:, 0].sum() >= 150 and (counts[:, 1:].sum(1) == counts[:, 0]).all()
    fused, _ = ex.main(num_envs=150, turns=160, batch=64, learn=False, verbose=False)
    composed, _ = ex.main(num_envs=150, turns=160, batch=64, learn=False, fused=False, verbose=False)
    assert np.array_equal(fused, composed) and fused[:, 0].sum() >= 150
    counts, rates = ex.main(num_envs=150, turns=160, evaluate_all=True, verbose=False)
    assert all(g >= 10 for g in counts[:, 0].tolist()) and len(rates) == 15 and all(0.0 <= r <= 1.0 for r in rates)
