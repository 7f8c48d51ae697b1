"""GPU tests of self-royale (everglades_amd.QPopulation; evg_population_clear / _assign / _qnet): a per-env Minimized Q network drawn from a population.

The reference side of every forward comparison is the plain evaluator: one MinimizedQNet launch per member over ALL rows, merged by torch.where on the
member ids -- bit equality, nothing rounded.  Assignment, history and tallies are compared with the host model (tests/population_model.py), whose
assignments for the forward tests a CPU test checks for coverage.

Sizes: a wavefront of the grouped forward owns 16 rows of one member's list and a workgroup 64, the bucket pass works in blocks of 256 rows: N = 15 / 16 /
17 and member counts of exactly 16 / 17 straddle the group, 77 a workgroup, 4096 sixteen bucket blocks and more than one workgroup per member."""
import ctypes as C

import numpy as np
import pytest

import minimized_model as mm
import population_model as pm

gpu = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 33, 77, 4096]
TEAMS = [(1, 1), (2, 3), (4, 4), (16, 16)]
HIDDEN = [17, 80, 128]
GUARD = 64
WIDE_SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


_ENVS, _WEIGHTS, _FEATS = {}, {}, {}


def _env(evg, N):
    if N not in _ENVS:
        _ENVS[N] = evg.EvergladesVecEnv(N, seed=11, auto_reset=True)
        _ENVS[N].reset()
    return _ENVS[N]


def _weights(torch, h1, dev):
    """two teams of 16 members, each a tuple (w1, b1, w2, b2); computed once per hidden size"""
    if h1 not in _WEIGHTS:
        gen = torch.Generator(device="cpu").manual_seed(1000 + h1)
        r = lambda *s: (torch.randn(s, generator=gen) * 0.3).to(dev)
        _WEIGHTS[h1] = [[(r(h1, 59), r(h1), r(11, h1), r(11)) for _ in range(16)] for _ in range(2)]
    return _WEIGHTS[h1]


def _features(torch, N, dev):
    if N not in _FEATS:
        gen = torch.Generator(device="cpu").manual_seed(N)
        _FEATS[N] = (torch.randn((N, 2, 34), generator=gen).to(dev), torch.randn((N, 2, 12, 13), generator=gen).to(dev))
    return _FEATS[N]


class _Guarded(object):
    """an output tensor with GUARD sentinels on each side"""

    def __init__(self, torch, shape, dev, fill=-77.0):
        n = int(np.prod(shape))
        self.fill, self.n = fill, n
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=dev)
        self.out = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())


def _merged_two_seats(torch, evg, env, teams, K, relu, shared, swarm, member):
    """K plain two-seat launches merged by torch.where: row [e, p] from the launch of member[e, p]"""
    want = torch.full(tuple(shared.shape[:2]) + (12, 11), float("nan"), device=env.device)
    for m in range(max(K)):
        pair = (teams[0][min(m, K[0] - 1)], teams[1][min(m, K[1] - 1)])
        q = evg.MinimizedQNet(env, pair, final_relu=relu)(shared, swarm)
        for p in range(2):
            if m < K[p]:
                want[:, p] = torch.where((member[:, p] == m)[:, None, None], q[:, p], want[:, p])
    return want


# ---------------------------------------------------------------------------------------------- the forward
@gpu
@pytest.mark.parametrize("K", TEAMS)
@pytest.mark.parametrize("N", SIZES)
def test_forward_equals_the_plain_launches_merged(evg, N, K):
    import torch
    env = _env(evg, N)
    dev = env.device
    shared, swarm = _features(torch, N, dev)
    for h1 in HIDDEN:
        w = _weights(torch, h1, dev)
        teams = [w[0][:K[0]], w[1][:K[1]]]
        for relu in (False, True):
            pop = env.q_population(teams[0], teams[1], final_relu=relu)
            assert pop.h1 == h1 and pop.num_members == K and tuple(pop.member.shape) == (N, 2)
            for kind in pm.ASSIGNMENTS:
                a = pm.assignment(kind, N, K)
                pop.member.copy_(torch.as_tensor(a))
                g = _Guarded(torch, (N, 2, 12, 11), dev)
                got = pop(shared, swarm, out=g.out)
                assert got is g.out and g.intact(), (h1, relu, kind)
                want = _merged_two_seats(torch, evg, env, teams, K, relu, shared, swarm, pop.member)
                assert not bool(torch.isnan(want).any())
                assert torch.equal(got, want), (h1, relu, kind, int((got != want).sum()))
                rows = pop.rows_per_member
                for p in range(2):
                    assert torch.equal(rows[p].long().cpu(), torch.bincount(torch.as_tensor(a[:, p]).long(), minlength=16)), (h1, relu, kind, p)
            assert pop.status() == 0
            pop.check()


@gpu
@pytest.mark.parametrize("rows", [1, 12, 16 * 12 + 5])
def test_expanded_layout_equals_the_plain_launches_merged(evg, rows):
    import torch
    env = _env(evg, 17)
    dev = env.device
    K = (3, 2)
    w = _weights(torch, 80, dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = env.q_population(teams[0], teams[1], final_relu=True)
    gen = torch.Generator(device="cpu").manual_seed(rows)
    x = torch.randn((rows, 59), generator=gen).to(dev)
    for seat in (0, 1):
        member = ((torch.arange(rows) * 7 + seat) % K[seat]).to(torch.uint8).to(dev)
        g = _Guarded(torch, (rows, 11), dev)
        got = pop.expanded(x, member, seat, out=g.out)
        want = torch.full((rows, 11), float("nan"), device=dev)
        for m in range(K[seat]):
            q = evg.MinimizedQNet(env, teams[seat][m], final_relu=True).expanded(x)
            want = torch.where((member == m)[:, None], q, want)
        assert g.intact() and torch.equal(got, want), (rows, seat)
        assert torch.equal(pop.rows_per_member[0].long().cpu(), torch.bincount(member.long().cpu(), minlength=16))
    # a batch [B, 12, 59] with one id per transition: the id is repeated over the transition's 12 rows
    B = 5
    xb = torch.randn((B, 12, 59), generator=gen).to(dev)
    mb = torch.tensor([2, 0, 1, 1, 2], dtype=torch.uint8, device=dev)
    got = pop.expanded(xb, mb, 0)
    for b in range(B):
        assert torch.equal(got[b], evg.MinimizedQNet(env, teams[0][int(mb[b])], final_relu=True).expanded(xb[b].contiguous()))
    assert pop.status() == 0


@gpu
def test_one_seat_compact_layout_for_seat_one(evg):
    import torch
    N, K = 77, (2, 3)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, 80, dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = env.q_population(teams[0], teams[1], final_relu=False)
    shared, swarm = _features(torch, N, dev)
    sh, sw = shared[:, 1].contiguous(), swarm[:, 1].contiguous()
    member = torch.as_tensor(pm.assignment("alternating", N, K)[:, 1].copy()).to(dev)
    g = _Guarded(torch, (N, 12, 11), dev)
    got = pop.seat(sh, sw, member, 1, out=g.out)
    want = torch.full((N, 12, 11), float("nan"), device=dev)
    for m in range(K[1]):
        want = torch.where((member == m)[:, None, None], evg.MinimizedQNet(env, teams[1][m], final_relu=False)(sh, sw), want)
    assert g.intact() and torch.equal(got, want)
    # ... and it is team 1's weights that were used, not team 0's
    other = evg.MinimizedQNet(env, teams[0][0], final_relu=False)(sh, sw)
    assert not torch.equal(got[member == 0], other[member == 0])


@gpu
def test_forward_equals_the_host_model_bit_for_bit(evg):
    import torch
    N, K, h1 = 17, (3, 3), 17
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, h1, dev)
    teams = [w[0][:3], w[1][:3]]
    pop = env.q_population(teams[0], teams[1], final_relu=True)
    a = pm.assignment("alternating", N, K)
    pop.member.copy_(torch.as_tensor(a))
    shared, swarm = _features(torch, N, dev)
    got = pop(shared, swarm).cpu().numpy()
    sh, sw = shared.cpu().numpy(), swarm.cpu().numpy()
    for p in range(2):
        for m in range(3):
            rows = np.nonzero(a[:, p] == m)[0]
            params = [t.cpu().numpy() for t in teams[p][m]]
            want = mm.forward_compact(sh[rows, p], sw[rows, p], params, True)
            assert np.array_equal(got[rows, p].view(np.uint32), want.view(np.uint32)), (p, m)


# ---------------------------------------------------------------------------------------------- status and sentinels
@gpu
def test_a_member_id_out_of_range_gives_zero_rows_and_the_status_bit(evg):
    import torch
    N, K = 77, (2, 3)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, 80, dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = env.q_population(teams[0], teams[1], final_relu=False)
    a = pm.assignment("alternating", N, K)
    good = a.copy()
    bad = [(0, 0, 2), (16, 0, 200), (40, 1, 3), (76, 1, 255), (76, 0, 16)]
    for e, p, v in bad:
        a[e, p] = v
    pop.member.copy_(torch.as_tensor(a))
    shared, swarm = _features(torch, N, dev)
    g = _Guarded(torch, (N, 2, 12, 11), dev)
    got = pop(shared, swarm, out=g.out)
    want = _merged_two_seats(torch, evg, env, teams, K, False, shared, swarm, torch.as_tensor(good).to(dev))
    for e, p, _ in bad:
        want[e, p] = 0.0
    assert g.intact() and torch.equal(got, want)
    assert pop.status() == evg._lib.POP_S_BAD_MEMBER
    with pytest.raises(evg.EvgError):
        pop.check()
    for p in range(2):
        ok = a[:, p] < K[p]
        assert torch.equal(pop.rows_per_member[p].long().cpu(), torch.bincount(torch.as_tensor(a[ok, p]).long(), minlength=16))
    pop.clear()
    assert pop.status() == 0 and int(pop.counts.sum()) == 0


# ---------------------------------------------------------------------------------------------- the assignment
def _episodes(env):
    return env.get_state()["env"][:, 2].astype(np.int64)


@gpu
def test_assignment_history_and_tallies_equal_the_host_model(evg):
    import torch
    N, K, base = 70, (3, 2), 4000000123
    envs = [evg.EvergladesVecEnv(N, seed=WIDE_SEED, env_id_base=base, auto_reset=False) for _ in range(2)]
    a, b = envs
    dev = a.device
    a.reset()
    w = _weights(torch, 17, dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = a.q_population(teams[0], teams[1], final_relu=True)
    model = pm.Population(WIDE_SEED, base, N, K)
    model.clear(_episodes(a))
    assert np.array_equal(pop.member.cpu().numpy(), model.member)
    assert all(len(set(model.member[:, p].tolist())) == K[p] for p in range(2))         # every member plays somewhere
    rng = np.random.RandomState(5)

    def round_(pop_, env_, model_, r):
        mask = (rng.rand(N) < 0.4).astype(np.uint8)
        mask[r % N] = 1
        winner = rng.randint(-1, 3, N).astype(np.int8)
        env_.reset(mask)                                                                # the envs of the mask start their next episode
        mt, wt = torch.as_tensor(mask).to(dev), torch.as_tensor(winner).to(dev)
        hist = torch.full((N, 2), 99, dtype=torch.uint8, device=dev)
        if r % 4 == 3:
            pop_.assign_after_reset(mt)                                                 # the draw alone: nothing tallied, no history
            want_hist = None
            model_.assign(mask, None, _episodes(env_))
        else:
            pop_.end_of_turn(done=mt, winner=wt, history=hist)
            want_hist = model_.assign(mask, winner, _episodes(env_))
        if want_hist is not None:
            h = hist.cpu().numpy()
            assert np.array_equal(h[mask != 0], want_hist[mask != 0]) and (h[mask == 0] == 99).all(), r
        assert np.array_equal(pop_.member.cpu().numpy(), model_.member), r
        assert np.array_equal(pop_.counts.cpu().numpy(), model_.counts), r
        return mask, winner

    for r in range(6):
        round_(pop, a, model, r)
    assert (_episodes(a) > 0).any() and (model.counts[:, :, 1:].sum(axis=(0, 1)) > 0).all()       # wins, ties and losses all occurred
    assert np.array_equal(model.counts[0, :, 0].sum(), model.counts[1, :, 0].sum())
    assert np.array_equal(model.counts[0, :, 1].sum(), model.counts[1, :, 3].sum())               # a seat's win is the other's loss
    # mask=None: every env
    a.reset()
    pop.assign_after_reset()
    model.assign(None, None, _episodes(a))
    assert np.array_equal(pop.member.cpu().numpy(), model.member) and pop.status() == 0
    # state() -> fresh objects -> load_state(): both continue identically
    st = pop.state()
    b.reset()
    b.restore(a.checkpoint())
    pop_b = b.q_population(teams[0], teams[1], final_relu=True)
    pop_b.load_state(st)
    model_b = pm.Population(WIDE_SEED, base, N, K)
    model_b.member[:], model_b.counts[:] = model.member, model.counts
    state = rng.get_state()
    for r in range(6, 10):
        round_(pop, a, model, r)
    rng.set_state(state)
    for r in range(6, 10):
        round_(pop_b, b, model_b, r)
    assert torch.equal(pop.member, pop_b.member) and torch.equal(pop.counts, pop_b.counts)
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------- end to end
@gpu
def test_self_royale_turns_equal_their_composition(evg):
    import torch
    N, K, turns, eps = 70, (3, 2), 310, (0.3, 0.3)
    a = evg.EvergladesVecEnv(N, seed=77, auto_reset=True)
    b = evg.EvergladesVecEnv(N, seed=77, auto_reset=True)
    dev = a.device
    w = _weights(torch, 80, dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    feats, rows = [], []
    for env in (a, b):
        obs = env.reset()
        f = (torch.zeros((N, 2, 34), device=dev), torch.zeros((N, 2, 12, 13), device=dev))
        for p in range(2):
            s, x = env.smart_state_compact(p, obs)
            f[0][:, p].copy_(s)
            f[1][:, p].copy_(x)
        feats.append(f)
        rows.append(torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=dev))
    pop = a.q_population(teams[0], teams[1], final_relu=True)
    model = pm.Population(77, 0, N, K)
    model.clear(_episodes(b))
    member_b = torch.as_tensor(model.member).to(dev)
    q = torch.zeros((N, 2, 12, 11), device=dev)
    ends = 0
    for t in range(turns):
        pop(feats[0][0], feats[0][1], out=q)
        got = a.step_q(q, eps, features=feats[0], actions_out=rows[0])
        pop.end_of_turn()
        qb = _merged_two_seats(torch, evg, b, teams, K, True, feats[1][0], feats[1][1], member_b)
        want = b.step_q(qb, eps, features=feats[1], actions_out=rows[1])
        assert torch.equal(q, qb), t
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), t
        assert torch.equal(rows[0], rows[1]), t
        assert torch.equal(feats[0][0], feats[1][0]) and torch.equal(feats[0][1], feats[1][1]), t
        done = want[2].cpu().numpy()
        if done.any():
            ends += int(done.sum())
            model.assign(done, b.winner.cpu().numpy(), _episodes(b))
            member_b = torch.as_tensor(model.member).to(dev)
            assert np.array_equal(pop.member.cpu().numpy(), model.member), t
    assert ends >= 2 * N                              # every env finished two games (150 turns at the most each)
    assert np.array_equal(pop.counts.cpu().numpy(), model.counts) and int(model.counts[0, :, 0].sum()) == ends
    assert pop.status() == 0
    a.close(), b.close()


@gpu
def test_self_royale_example_runs_with_finite_losses():
    import os
    import sys
    import torch
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import minimized_self_royale
    losses = minimized_self_royale.main(1024, 170, 256)
    assert losses.dim() == 3 and tuple(losses.shape[1:]) == (2, 4) and losses.shape[0] >= 100
    assert bool(torch.isfinite(losses).all())


# ---------------------------------------------------------------------------------------------- bad input
@gpu
def test_every_bad_argument_is_refused_with_nothing_launched(evg):
    import torch
    _lib = evg._lib
    N, K = 33, (2, 3)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, 80, dev)
    pop = env.q_population(w[0][:2], w[1][:3], final_relu=True)
    pop._descriptor(N)
    L, h, st = env.L, env._h, env._stream()
    shared, swarm = _features(torch, N, dev)
    out = torch.full((N, 2, 12, 11), -3.0, device=dev)
    member0 = pop.member.clone()
    counts0 = pop.counts.clone()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def desc(**kw):
        d = _lib.EvgPopulation()
        C.memmove(C.byref(d), C.byref(pop._desc), C.sizeof(d))
        for k, v in kw.items():
            if isinstance(v, tuple):
                f, p, m, val = (getattr(d, k),) + v
                f[p][m] = val
            else:
                setattr(d, k, v)
        return d

    def qnet(d, layout=_lib.QNET_COMPACT_SEATS, rows=N, seat=0, member=pop.member, in0=shared, in1=swarm, o=out):
        pv = lambda t: None if t is None else (t if isinstance(t, C.c_void_p) else ptr(t))
        return L.evg_population_qnet(h, None if d is None else C.byref(d), layout, rows, seat, pv(member), pv(in0), pv(in1), pv(o), st)

    good = desc()
    assert qnet(good) == 0                                                       # the descriptor the cases below spoil is accepted as it is
    out.fill_(-3.0)
    two = desc()
    two.num_members[0] = 0
    big = desc()
    big.num_members[1] = 17
    bad_descs = [None, desc(struct_size=C.sizeof(_lib.EvgPopulation) - 8), desc(h1=0), desc(h1=129), desc(final_relu=2), two, big,
                 desc(member=None), desc(counts=None), desc(ctl=None), desc(index=None), desc(first=None), desc(count=None), desc(hist=None),
                 desc(w1=(0, 1, None)), desc(b1=(1, 2, None)), desc(w2=(1, 0, None)), desc(b2=(0, 0, None)),
                 desc(w1=(1, 1, w[1][1][0].data_ptr() + 4)), desc(scratch_rows=N - 1)]
    for i, d in enumerate(bad_descs):
        assert qnet(d) == _lib.ERR_ARG, i
    misaligned = C.c_void_p(shared.data_ptr() + 4)
    for kw in (dict(layout=3), dict(layout=-1), dict(rows=0), dict(rows=(1 << 24) + 1), dict(member=None), dict(in0=None), dict(in1=None), dict(o=None),
               dict(in0=misaligned), dict(o=C.c_void_p(out.data_ptr() + 8)), dict(layout=_lib.QNET_COMPACT, seat=2),
               dict(layout=_lib.QNET_EXPANDED, seat=-1)):
        assert qnet(good, **kw) == _lib.ERR_ARG, kw
    assert L.evg_population_qnet(None, C.byref(good), _lib.QNET_COMPACT_SEATS, N, 0, ptr(pop.member), ptr(shared), ptr(swarm), ptr(out), st) == _lib.ERR_ARG
    # clear and assign take the descriptor's first part only
    for i, d in enumerate(bad_descs[:10]):
        ref = None if d is None else C.byref(d)
        assert L.evg_population_clear(h, ref, st) == _lib.ERR_ARG, i
        assert L.evg_population_assign(h, ref, None, None, None, st) == _lib.ERR_ARG, i
    assert L.evg_population_clear(None, C.byref(good), st) == _lib.ERR_ARG
    mt = evg.EvergladesVecEnv(4, rng_mode="mt19937")
    assert L.evg_population_clear(mt._h, C.byref(good), st) == _lib.ERR_ARG         # the draw is keyed
    assert L.evg_population_assign(mt._h, C.byref(good), None, None, None, st) == _lib.ERR_ARG
    mt.close()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and torch.equal(pop.member, member0) and torch.equal(pop.counts, counts0) and pop.status() == 0
    # the Python layer's own checks
    with pytest.raises(ValueError):
        env.q_population([], w[1][:1], final_relu=True)
    with pytest.raises(ValueError):
        env.q_population(w[0][:17] + w[0][:1], None, final_relu=True)
    with pytest.raises(ValueError):
        env.q_population(w[0][:2], _weights(torch, 17, dev)[1][:2], final_relu=True)      # another hidden size
    with pytest.raises(ValueError):
        pop(shared[:5], swarm[:5])
    with pytest.raises(ValueError):
        pop.expanded(torch.zeros((4, 59), device=dev), torch.zeros(3, dtype=torch.uint8, device=dev), 0)
    with pytest.raises(ValueError):
        pop.expanded(torch.zeros((4, 59), device=dev), torch.zeros(4, dtype=torch.uint8, device=dev), 2)
