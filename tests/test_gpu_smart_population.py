"""GPU tests of Smart_State self-royale (everglades_amd.SmartQPopulation; evg_smart_population_clear / _assign / _qnet): a per-env Smart_State Q
network (59 -> h1 -> h2 -> 5) drawn from a population.

The reference side of every forward comparison is the plain evaluator: one SmartQNet launch per member over ALL rows, merged by torch.where on the member
ids -- bit equality (torch.equal), nothing rounded.  Assignment, history and tallies are compared with the host model (tests/population_model.py) and
with a QPopulation of the same team sizes on a second, identical handle.

Sizes: a wavefront of the grouped forward owns 16 rows of one member's list and a workgroup 64, the bucket pass works in blocks of 256 rows: N = 15 / 16 /
17 straddle the group, 77 a workgroup, 4096 sixteen bucket blocks and more than one workgroup per member; 32 785 expanded rows give a grid at its cap
(two workgroups per CU), where a wavefront loops over its list and a member's share of the grid is below the grid."""
import ctypes as C

import numpy as np
import pytest

import population_model as pm

gpu = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 33, 77, 4096]
TEAMS = [(1, 1), (2, 3), (4, 4), (16, 16)]
HIDDEN = [(60, 60), (17, 64), (1, 1), (64, 64)]
ASSIGNMENTS = ("draw", "last", "round_robin", "skew")
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


def _weights(torch, hh, dev):
    """two teams of 16 members, each a tuple (w1, b1, w2, b2, w3, b3); computed once per pair of hidden sizes and never written to"""
    if hh not in _WEIGHTS:
        h1, h2 = hh
        gen = torch.Generator(device="cpu").manual_seed(2000 + 100 * h1 + h2)
        r = lambda *s: (torch.randn(s, generator=gen) * 0.3).to(dev)
        _WEIGHTS[hh] = [[(r(h1, 59), r(h1), r(h2, h1), r(h2), r(5, h2), r(5)) for _ in range(16)] for _ in range(2)]
    return _WEIGHTS[hh]


def _features(torch, N, dev):
    if N not in _FEATS:
        gen = torch.Generator(device="cpu").manual_seed(N)
        _FEATS[N] = (torch.randn((N, 2, 34), generator=gen).to(dev), torch.randn((N, 2, 12, 13), generator=gen).to(dev))
    return _FEATS[N]


def _assignment(kind, N, K, pop=None):
    """uint8 [N, 2]: the device's own draw, every row on the last member, round-robin, or a seeded skew that leaves two members (where a team has three or
    more; otherwise all but one) without a row"""
    if kind == "draw":
        pop.clear()
        return pop.member.cpu().numpy().copy()
    if kind == "last":
        return pm.assignment("one", N, K)
    if kind == "round_robin":
        return pm.assignment("alternating", N, K)
    assert kind == "skew"
    rng = np.random.RandomState(1000 * N + 17 * K[0] + K[1])
    a = np.zeros((N, 2), np.uint8)
    for p in range(2):
        k = K[p]
        used = np.arange(k)[1:-1] if k >= 3 else np.arange(k)[:1]                    # members 0 and k - 1 stay empty
        w = 0.5 ** np.arange(len(used))
        a[:, p] = rng.choice(used, size=N, p=w / w.sum())
    return a


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
    want = torch.full(tuple(shared.shape[:2]) + (12, 5), float("nan"), device=env.device)
    for m in range(max(K)):
        pair = (teams[0][min(m, K[0] - 1)], teams[1][min(m, K[1] - 1)])
        q = evg.SmartQNet(env, pair, final_relu=relu)(shared, swarm)
        for p in range(2):
            if m < K[p]:
                want[:, p] = torch.where((member[:, p] == m)[:, None, None], q[:, p], want[:, p])
    return want


def _merged_expanded(torch, evg, env, team, relu, x, member):
    """len(team) plain expanded launches over all rows of x [R, 59], merged by torch.where on member [R]"""
    want = torch.full((x.shape[0], 5), float("nan"), device=env.device)
    for m, net in enumerate(team):
        want = torch.where((member == m)[:, None], evg.SmartQNet(env, net, final_relu=relu).expanded(x), want)
    return want


def _check_two_seats(torch, evg, env, N, K, hh, relus, kinds):
    dev = env.device
    shared, swarm = _features(torch, N, dev)
    w = _weights(torch, hh, dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    for relu in relus:
        pop = env.smart_q_population(teams[0], teams[1], final_relu=relu)
        assert (pop.h1, pop.h2) == hh and pop.num_members == K and tuple(pop.member.shape) == (N, 2) and pop.OUT == 5
        for kind in kinds:
            a = _assignment(kind, N, K, pop)
            pop.member.copy_(torch.as_tensor(a))
            g = _Guarded(torch, (N, 2, 12, 5), dev)
            got = pop(shared, swarm, out=g.out)
            assert got is g.out and g.intact(), (hh, relu, kind)
            want = _merged_two_seats(torch, evg, env, teams, K, relu, shared, swarm, pop.member)
            assert bool(torch.isfinite(want).all())
            assert torch.equal(got, want), (hh, relu, kind, int((got != want).sum()))
            rows = pop.rows_per_member
            for p in range(2):
                assert torch.equal(rows[p].long().cpu(), torch.bincount(torch.as_tensor(a[:, p]).long(), minlength=16)), (hh, relu, kind, p)
        assert pop.status() == 0
        pop.check()


# ---------------------------------------------------------------------------------------------- the forward
@gpu
@pytest.mark.parametrize("K", TEAMS)
@pytest.mark.parametrize("N", SIZES)
def test_forward_equals_the_plain_launches_merged(evg, N, K):
    import torch
    _check_two_seats(torch, evg, _env(evg, N), N, K, (60, 60), (False, True), ASSIGNMENTS)


@gpu
@pytest.mark.parametrize("hh", HIDDEN)
def test_forward_at_every_hidden_size(evg, hh):
    import torch
    _check_two_seats(torch, evg, _env(evg, 77), 77, (4, 4), hh, (False, True), ASSIGNMENTS)


def test_the_skewed_assignment_leaves_two_members_without_a_row():
    a = _assignment("skew", 77, (4, 4))
    for p in range(2):
        assert sorted(set(a[:, p].tolist())) == [1, 2]
    a = _assignment("skew", 4096, (16, 16))
    assert 0 not in a and 15 not in a and len(set(a[:, 0].tolist())) >= 8


@gpu
@pytest.mark.parametrize("B", [1, 5, 257])
def test_expanded_layout_equals_the_plain_launches_merged(evg, B):
    import torch
    env = _env(evg, 17)
    dev = env.device
    K = (3, 2)
    w = _weights(torch, (60, 60), dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = env.smart_q_population(teams[0], teams[1], final_relu=True)
    gen = torch.Generator(device="cpu").manual_seed(B)
    x = torch.randn((B, 12, 59), generator=gen).to(dev)
    for seat in (0, 1):
        member = ((torch.arange(B) * 7 + seat) % K[seat]).to(torch.uint8).to(dev)           # [B]: one id per transition, repeated over its 12 rows
        g = _Guarded(torch, (B, 12, 5), dev)
        got = pop.expanded(x, member, seat, out=g.out)
        rows = member[:, None].expand(B, 12).reshape(-1)
        want = _merged_expanded(torch, evg, env, teams[seat], True, x.view(-1, 59), rows).view(B, 12, 5)
        assert bool(torch.isfinite(want).all())
        assert g.intact() and torch.equal(got, want), (B, seat)
        assert torch.equal(pop.rows_per_member[0].long().cpu(), torch.bincount(rows.long().cpu(), minlength=16))
        # ... and the same with one id per row
        got = pop.expanded(x, member[:, None].expand(B, 12).contiguous(), seat)
        assert torch.equal(got, want), (B, seat)
    assert pop.status() == 0


@gpu
def test_one_seat_compact_layout(evg):
    import torch
    N, K = 77, (2, 3)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, (17, 64), dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = env.smart_q_population(teams[0], teams[1], final_relu=False)
    shared, swarm = _features(torch, N, dev)
    for seat in (0, 1):
        sh, sw = shared[:, seat].contiguous(), swarm[:, seat].contiguous()
        member = torch.as_tensor(pm.assignment("alternating", N, K)[:, seat].copy()).to(dev)
        g = _Guarded(torch, (N, 12, 5), dev)
        got = pop.seat(sh, sw, member, seat, out=g.out)
        want = torch.full((N, 12, 5), float("nan"), device=dev)
        for m in range(K[seat]):
            want = torch.where((member == m)[:, None, None], evg.SmartQNet(env, teams[seat][m], final_relu=False)(sh, sw), want)
        assert g.intact() and torch.equal(got, want), seat
        # ... and it is this seat's team whose weights were used, not the other's
        other = evg.SmartQNet(env, teams[1 - seat][0], final_relu=False)(sh, sw)
        assert not torch.equal(got[member == 0], other[member == 0])


@gpu
@pytest.mark.parametrize("split", ["one", "even"])
def test_a_grid_at_its_cap(evg, split):
    """32 785 expanded rows: 2 050 groups of 16, more than the capped grid's wavefronts deal in one pass.  All rows on one member: its wavefronts loop over
    list_stride; an even split over 4: each member's share of the grid (live) is a quarter of gridDim.x."""
    import torch
    R = 32785
    env = _env(evg, 17)
    dev = env.device
    w = _weights(torch, (60, 60), dev)
    team = w[0][:4]
    pop = env.smart_q_population(team, None, final_relu=True, max_rows=R)
    gen = torch.Generator(device="cpu").manual_seed(R)
    x = torch.randn((R, 59), generator=gen).to(dev)
    member = (torch.full((R,), 2) if split == "one" else torch.arange(R) % 4).to(torch.uint8).to(dev)
    g = _Guarded(torch, (R, 5), dev)
    got = pop.expanded(x, member, 0, out=g.out)
    want = _merged_expanded(torch, evg, env, team, True, x, member)
    assert g.intact() and torch.equal(got, want), int((got != want).any(1).sum())
    assert torch.equal(pop.rows_per_member[0].long().cpu(), torch.bincount(member.long().cpu(), minlength=16))
    assert pop.status() == 0


# ---------------------------------------------------------------------------------------------- a member's weights stay with its rows
@gpu
def test_a_nan_weight_in_one_member_reaches_exactly_its_rows(evg):
    import torch
    N, K = 77, (4, 4)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, (60, 60), dev)
    sick = tuple(t.clone() for t in w[0][2])
    sick[2][5, 7] = float("nan")                                                # w2[5][7] of member 2 of team 0
    teams = [w[0][:2] + [sick] + w[0][3:4], w[1][:4]]
    clean = [w[0][:4], w[1][:4]]
    shared, swarm = _features(torch, N, dev)
    a = pm.assignment("alternating", N, K)
    member = torch.as_tensor(a).to(dev)
    for relu in (False, True):
        pop = env.smart_q_population(teams[0], teams[1], final_relu=relu)
        pop.member.copy_(member)
        got = pop(shared, swarm)
        want = _merged_two_seats(torch, evg, env, teams, K, relu, shared, swarm, member)          # the plain kernel's rule for the NaN
        healthy = _merged_two_seats(torch, evg, env, clean, K, relu, shared, swarm, member)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=-5.0), torch.nan_to_num(want, nan=-5.0))
        mine = torch.zeros((N, 2), dtype=torch.bool, device=dev)
        mine[:, 0] = member[:, 0] == 2
        assert bool(torch.isnan(got[mine]).any(-1).any(-1).all())             # every row of the member has a NaN ...
        assert torch.equal(got[~mine], healthy[~mine])                          # ... and every other row is what it was
        assert pop.status() == 0


# ---------------------------------------------------------------------------------------------- status and sentinels
@gpu
def test_a_member_id_out_of_range_gives_zero_rows_and_the_status_bit(evg):
    import torch
    N, K = 77, (2, 3)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, (60, 60), dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = env.smart_q_population(teams[0], teams[1], final_relu=False)
    a = pm.assignment("alternating", N, K)
    good = a.copy()
    bad = [(0, 0, 2), (16, 0, 200), (40, 1, 3), (76, 1, 255), (76, 0, 16)]
    for e, p, v in bad:
        a[e, p] = v
    pop.member.copy_(torch.as_tensor(a))
    shared, swarm = _features(torch, N, dev)
    g = _Guarded(torch, (N, 2, 12, 5), dev)
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
    pop.check()
    # the expanded layout: a bad row is 5 floats, and the rows behind it are untouched by its zeros
    R = 40
    gen = torch.Generator(device="cpu").manual_seed(R)
    x = torch.randn((R, 59), generator=gen).to(dev)
    ids = (torch.arange(R) % 3).to(torch.uint8)
    goodx = ids.clone()
    for r, v in ((0, 3), (17, 255), (39, 16)):
        ids[r] = v
    g = _Guarded(torch, (R, 5), dev)
    got = pop.expanded(x, ids.to(dev), 1, out=g.out)
    want = _merged_expanded(torch, evg, env, teams[1], False, x, goodx.to(dev))
    want[[0, 17, 39]] = 0.0
    assert g.intact() and torch.equal(got, want)
    assert pop.status() == evg._lib.POP_S_BAD_MEMBER
    pop.clear()
    assert pop.status() == 0


# ---------------------------------------------------------------------------------------------- the assignment
def _episodes(env):
    return env.get_state()["env"][:, 2].astype(np.int64)


@gpu
def test_assignment_history_and_tallies_equal_the_host_model_and_a_minimized_population(evg):
    import torch
    N, K, base = 70, (3, 2), 4000000123
    envs = [evg.EvergladesVecEnv(N, seed=WIDE_SEED, env_id_base=base, auto_reset=False) for _ in range(3)]
    a, b, c = envs
    dev = a.device
    for e in envs:
        e.reset()
    w = _weights(torch, (17, 64), dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    pop = a.smart_q_population(teams[0], teams[1], final_relu=True)
    gen = torch.Generator(device="cpu").manual_seed(3)
    mini = [[tuple((torch.randn(s, generator=gen) * 0.3).to(dev) for s in ((17, 59), (17,), (11, 17), (11,))) for _ in range(K[p])] for p in range(2)]
    twin = c.q_population(mini[0], mini[1], final_relu=True)                   # the same team sizes on a second, identical handle
    model = pm.Population(WIDE_SEED, base, N, K)
    model.clear(_episodes(a))
    assert np.array_equal(pop.member.cpu().numpy(), model.member) and torch.equal(pop.member, twin.member)
    assert all(len(set(model.member[:, p].tolist())) == K[p] for p in range(2))         # every member plays somewhere
    rng = np.random.RandomState(5)

    def round_(pops, env_s, model_, r):
        mask = (rng.rand(N) < 0.4).astype(np.uint8)
        mask[r % N] = 1
        winner = rng.randint(-1, 3, N).astype(np.int8)
        mt, wt = torch.as_tensor(mask).to(dev), torch.as_tensor(winner).to(dev)
        hists = []
        for pop_, env_ in zip(pops, env_s):
            env_.reset(mask)                                                            # the envs of the mask start their next episode
            hist = torch.full((N, 2), 99, dtype=torch.uint8, device=dev)
            if r % 4 == 3:
                pop_.assign_after_reset(mt)                                             # the draw alone: nothing tallied, no history
            else:
                pop_.end_of_turn(done=mt, winner=wt, history=hist)
            hists.append(hist)
        want_hist = model_.assign(mask, None if r % 4 == 3 else winner, _episodes(env_s[0]))
        for pop_, hist in zip(pops, hists):
            h = hist.cpu().numpy()
            if r % 4 == 3:
                assert (h == 99).all(), r
            else:
                assert np.array_equal(h[mask != 0], want_hist[mask != 0]) and (h[mask == 0] == 99).all(), r
            assert np.array_equal(pop_.member.cpu().numpy(), model_.member), r
            assert np.array_equal(pop_.counts.cpu().numpy(), model_.counts), r
        assert torch.equal(hists[0], hists[-1])

    for r in range(6):
        round_((pop, twin), (a, c), model, r)
    assert (_episodes(a) > 0).any() and (model.counts[:, :, 1:].sum(axis=(0, 1)) > 0).all()       # wins, ties and losses all occurred
    assert torch.equal(pop.member, twin.member) and torch.equal(pop.counts, twin.counts)
    st, st_twin = pop.state(), twin.state()
    assert sorted(st) == sorted(st_twin) and all(np.array_equal(st[k], st_twin[k]) for k in st)
    assert np.array_equal(st["member"], model.member) and np.array_equal(st["counts"], model.counts) and not st["ctl"].any()
    # mask=None: every env
    a.reset()
    pop.assign_after_reset()
    model.assign(None, None, _episodes(a))
    assert np.array_equal(pop.member.cpu().numpy(), model.member) and pop.status() == 0
    # state() -> fresh objects -> load_state(): both continue identically
    st = pop.state()
    b.restore(a.checkpoint())
    pop_b = b.smart_q_population(teams[0], teams[1], final_relu=True)
    pop_b.load_state(st)
    assert all(np.array_equal(v, pop_b.state()[k]) for k, v in st.items())
    model_b = pm.Population(WIDE_SEED, base, N, K)
    model_b.member[:], model_b.counts[:] = model.member, model.counts
    state = rng.get_state()
    for r in range(6, 10):
        round_((pop,), (a,), model, r)
    rng.set_state(state)
    for r in range(6, 10):
        round_((pop_b,), (b,), model_b, r)
    assert torch.equal(pop.member, pop_b.member) and torch.equal(pop.counts, pop_b.counts)
    with pytest.raises(ValueError):
        b.smart_q_population(teams[0][:2], teams[1], final_relu=True).load_state(st)    # other team sizes
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------- end to end
@gpu
def test_self_royale_turns_equal_their_composition(evg):
    import torch
    N, K, turns, eps = 64, (3, 2), 310, (0.3, 0.3)
    a = evg.EvergladesVecEnv(N, seed=77, auto_reset=True)
    b = evg.EvergladesVecEnv(N, seed=77, auto_reset=True)
    dev = a.device
    w = _weights(torch, (60, 60), dev)
    teams = [w[0][:K[0]], w[1][:K[1]]]
    feats, rows, dirs = [], [], []
    for env in (a, b):
        obs = env.reset()
        f = (torch.zeros((N, 2, 34), device=dev), torch.zeros((N, 2, 12, 13), device=dev))
        for p in range(2):
            s, x = env.smart_state_compact(p, obs)
            f[0][:, p].copy_(s)
            f[1][:, p].copy_(x)
        feats.append(f)
        rows.append(torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=dev))
        dirs.append(torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=dev))
    pop = a.smart_q_population(teams[0], teams[1], final_relu=True)
    model = pm.Population(77, 0, N, K)
    model.clear(_episodes(b))
    member_b = torch.as_tensor(model.member).to(dev)
    q = torch.zeros((N, 2, 12, 5), device=dev)
    hist = torch.full((N, 2), 99, dtype=torch.uint8, device=dev)
    ends = 0
    for t in range(turns):
        pop(feats[0][0], feats[0][1], out=q)
        got = a.step_q(q, eps, features=feats[0], directions=dirs[0], actions_out=rows[0])
        pop.end_of_turn(history=hist)
        qb = _merged_two_seats(torch, evg, b, teams, K, True, feats[1][0], feats[1][1], member_b)
        want = b.step_q(qb, eps, features=feats[1], directions=dirs[1], actions_out=rows[1])
        assert torch.equal(q, qb), t
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), t
        assert torch.equal(rows[0], rows[1]) and torch.equal(dirs[0], dirs[1]), t
        assert torch.equal(feats[0][0], feats[1][0]) and torch.equal(feats[0][1], feats[1][1]), t
        done = want[2].cpu().numpy()
        if done.any():
            ends += int(done.sum())
            played = model.assign(done, b.winner.cpu().numpy(), _episodes(b))
            member_b = torch.as_tensor(model.member).to(dev)
            assert np.array_equal(hist.cpu().numpy()[done != 0], played[done != 0]), t
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
    import smart_state_self_royale
    losses = smart_state_self_royale.main(2048, 60, 256)
    assert losses.dim() == 3 and tuple(losses.shape[1:]) == (2, 4) and losses.shape[0] == 60 - 2
    assert bool(torch.isfinite(losses).all())
    # 2 048 envs over teams of 4: every member plays from the first turn on, so every member has steps with a loss
    assert bool((losses != 0).any(dim=0).all())


# ---------------------------------------------------------------------------------------------- bad input
@gpu
def test_every_bad_argument_is_refused_with_nothing_launched(evg):
    import torch
    _lib = evg._lib
    N, K = 33, (2, 3)
    env = _env(evg, N)
    dev = env.device
    w = _weights(torch, (60, 60), dev)
    pop = env.smart_q_population(w[0][:2], w[1][:3], final_relu=True)
    pop._descriptor(N)
    L, h, st = env.L, env._h, env._stream()
    shared, swarm = _features(torch, N, dev)
    out = torch.full((N, 2, 12, 5), -3.0, device=dev)
    member0 = pop.member.clone()
    counts0 = pop.counts.clone()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def desc(**kw):
        d = _lib.EvgSmartPopulation()
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
        return L.evg_smart_population_qnet(h, None if d is None else C.byref(d), layout, rows, seat, pv(member), pv(in0), pv(in1), pv(o), st)

    good = desc()
    assert qnet(good) == 0                                                       # the descriptor the cases below spoil is accepted as it is
    torch.cuda.synchronize()
    out.fill_(-3.0)
    none0, big1 = desc(), desc()
    none0.num_members[0] = 0
    big1.num_members[1] = 17
    first_part = [None, desc(struct_size=C.sizeof(_lib.EvgSmartPopulation) - 8), desc(struct_size=C.sizeof(_lib.EvgPopulation)), desc(h1=0), desc(h1=65),
                  desc(h2=0), desc(h2=65), desc(final_relu=2), desc(final_relu=-1), none0, big1, desc(member=None), desc(counts=None), desc(ctl=None),
                  desc(member=pop.member.data_ptr() + 1), desc(counts=pop.counts.data_ptr() + 4), desc(ctl=pop._ctl.data_ptr() + 4)]
    forward_part = [desc(index=None), desc(first=None), desc(count=None), desc(hist=None),
                    desc(index=pop._index.data_ptr() + 2), desc(first=pop._bins[0].data_ptr() + 2), desc(count=pop._bins[1].data_ptr() + 1),
                    desc(hist=pop._hist.data_ptr() + 2),
                    desc(w1=(0, 1, None)), desc(b1=(1, 2, None)), desc(w2=(1, 0, None)), desc(b2=(0, 0, None)), desc(w3=(1, 1, None)), desc(b3=(0, 1, None)),
                    desc(w1=(1, 1, w[1][1][0].data_ptr() + 4)), desc(w3=(0, 0, w[0][0][4].data_ptr() + 8)), desc(b3=(1, 2, w[1][2][5].data_ptr() + 4)),
                    desc(scratch_rows=N - 1), desc(scratch_rows=0)]
    for i, d in enumerate(first_part + forward_part):
        assert qnet(d) == _lib.ERR_ARG, i
    misaligned = C.c_void_p(shared.data_ptr() + 4)
    for kw in (dict(layout=3), dict(layout=-1), dict(rows=0), dict(rows=-5), dict(rows=(1 << 24) + 1), dict(member=None), dict(in0=None), dict(in1=None),
               dict(o=None), dict(in0=misaligned), dict(in1=C.c_void_p(swarm.data_ptr() + 4)), dict(o=C.c_void_p(out.data_ptr() + 8)),
               dict(layout=_lib.QNET_COMPACT, seat=2), dict(layout=_lib.QNET_COMPACT, seat=-1), dict(layout=_lib.QNET_EXPANDED, seat=-1),
               dict(layout=_lib.QNET_EXPANDED, seat=2)):
        assert qnet(good, **kw) == _lib.ERR_ARG, kw
    assert L.evg_smart_population_qnet(None, C.byref(good), _lib.QNET_COMPACT_SEATS, N, 0, ptr(pop.member), ptr(shared), ptr(swarm), ptr(out), st) \
        == _lib.ERR_ARG
    # clear and assign take the descriptor's first part only
    for i, d in enumerate(first_part):
        ref = None if d is None else C.byref(d)
        assert L.evg_smart_population_clear(h, ref, st) == _lib.ERR_ARG, i
        assert L.evg_smart_population_assign(h, ref, None, None, None, st) == _lib.ERR_ARG, i
    hist = torch.full((N, 2), 99, dtype=torch.uint8, device=dev)
    assert L.evg_smart_population_assign(h, C.byref(good), None, None, C.c_void_p(hist.data_ptr() + 1), st) == _lib.ERR_ARG
    assert L.evg_smart_population_clear(None, C.byref(good), st) == _lib.ERR_ARG
    mt = evg.EvergladesVecEnv(4, rng_mode="mt19937")
    assert L.evg_smart_population_clear(mt._h, C.byref(good), st) == _lib.ERR_ARG   # the draw is keyed
    assert L.evg_smart_population_assign(mt._h, C.byref(good), None, None, None, st) == _lib.ERR_ARG
    mt.close()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((hist == 99).all())
    assert torch.equal(pop.member, member0) and torch.equal(pop.counts, counts0) and pop.status() == 0
    # the Python layer's own checks
    with pytest.raises(ValueError):
        env.smart_q_population([], w[1][:1], final_relu=True)
    with pytest.raises(ValueError):
        env.smart_q_population(w[0][:16] + w[0][:1], None, final_relu=True)
    with pytest.raises(ValueError):
        env.smart_q_population(w[0][:2], _weights(torch, (17, 64), dev)[1][:2], final_relu=True)     # other hidden sizes
    with pytest.raises(ValueError):
        env.smart_q_population(w[0][:2], w[1][:2])                                                  # tuples need final_relu
    with pytest.raises(ValueError):
        env.smart_q_population([(w[0][0], w[0][1])], None, final_relu=True)                         # a member is one network, not a pair
    with pytest.raises(ValueError):
        pop(shared[:5], swarm[:5])
    with pytest.raises(ValueError):
        pop(shared, swarm, out=torch.zeros((N, 2, 12, 11), device=dev))                             # the Minimized head's shape
    with pytest.raises(ValueError):
        pop.expanded(torch.zeros((4, 59), device=dev), torch.zeros(3, dtype=torch.uint8, device=dev), 0)
    with pytest.raises(ValueError):
        pop.expanded(torch.zeros((4, 59), device=dev), torch.zeros(4, dtype=torch.uint8, device=dev), 2)
    with pytest.raises(ValueError):
        pop.seat(shared[:, 0].contiguous(), swarm[:, 0].contiguous(), pop.member[:, 0].contiguous(), 3)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
