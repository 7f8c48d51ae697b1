"""GPU tests of evg_population_qnet_bf16 / evg_smart_population_qnet_bf16 (env.q_population / env.smart_q_population with precision="bf16";
include/evg_pop_bf16.h) and of PopulationLearner(target_precision="bf16_grouped"):

  exact tier     the families of tests/qnet_bf16_cases.py per member (the damaged weight set of `nonfinite` on members 1 and 3): bit-equal to the composed
                 host model (tests/population_bf16_cases.py) for 1, 15, 16, 17 and 37 rows, teams of 1, 2, 4 and 16 (two seats: 2 and 5), every id pattern
  plain          every row bit-equal to its member's own SmartQNetBf16 / MinimizedQNetBf16 in the same layout, random families included
  random tier    |Q^ - Q| <= E of the host model
  boundaries     rows of nobody, the published lists, the second sweep of the capped grid, sentinels, repeatability, capture, refusals, fp32 untouched
  use            one self-play turn, the learner, the two examples"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import learner_edge_cases as edge
import population_bf16_cases as pcases
import population_edge_cases as pedge
import qnet_bf16_cases as cases
import qnet_bf16_model as model

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
WORST = {}
SENTINEL = -7.25


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


@pytest.fixture(scope="module")
def env(evg):
    e = evg.EvergladesVecEnv(64, seed=5)
    e.reset()
    yield e
    e.close()


def _dev(env, a):
    import torch
    if isinstance(a, (tuple, list)):
        return tuple(_dev(env, x) for x in a)
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _pop(env, kind, team0, team1=None, final_relu=False, precision="bf16"):
    make = env.smart_q_population if kind == "smart" else env.q_population
    return make([_dev(env, p) for p in team0], None if team1 is None else [_dev(env, p) for p in team1], final_relu=final_relu, max_rows=4096,
                precision=precision)


def _shape(kind, layout, rows):
    return {"expanded": (rows,), "seat": (rows, 12), "seats": (rows, 2, 12)}[layout] + (cases.OUT[kind],)


def _run(env, evg, pop, layout, inputs, ids, out=None):
    """one grouped forward in a layout on host or device inputs; the two-seat layout at any row count (pop(shared, swarm) is that launch at num_envs rows
    with pop.member)"""
    d = inputs if not isinstance(inputs, np.ndarray) and not isinstance(inputs[0], np.ndarray) else _dev(env, inputs)
    idd = _dev(env, ids) if isinstance(ids, np.ndarray) else ids
    if layout == "expanded":
        return pop.expanded(d, idd, 0, out=out)
    if layout == "seat":
        return pop.seat(d[0], d[1], idd, 0, out=out)
    import torch
    rows = d[0].shape[0]
    out = torch.empty(_shape("smart" if pop.OUT == 5 else "mini", layout, rows), dtype=torch.float32, device=env.device) if out is None else out
    return pop._launch(evg._lib.QNET_COMPACT_SEATS, rows, 0, idd, d[0], d[1], out)


def _guarded(env, shape):
    """an output with 16 floats of sentinel on both sides -> (the whole buffer, the output's view)"""
    import torch
    n = int(np.prod(shape))
    whole = torch.full((n + 32,), SENTINEL, dtype=torch.float32, device=env.device)
    return whole, whole[16:16 + n].view(shape)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _relu(q):
    return np.where(q < 0, np.float32(0), q)


def _member_tables(kind, layout, teams, inputs, exact, rounds):
    """the host model of every member on every row: tables[p][m] = (Q, E) of team p's member m over the rows of its seat"""
    lay = pcases.model_layout(layout)
    if layout == "seats":
        return [[model.forward_layout(lay, prm, (inputs[0][:, p], inputs[1][:, p]), False, exact, rounds) for prm in teams[p]] for p in range(2)]
    return [[model.forward_layout(lay, prm, inputs, False, exact, rounds) for prm in teams]]


def _select(tables, layout, ids, rows, K):
    """(Q, E) of the first `rows` rows for the ids of a call, from the members' tables; zeros for the rows of nobody"""
    per_seat = []
    for p, table in enumerate(tables):
        one = ids[:, p] if layout == "seats" else ids
        q = np.zeros((rows,) + table[0][0].shape[1:], np.float32)
        e = np.zeros(q.shape, np.float64)
        for m in range(K[p] if layout == "seats" else K):
            at = np.flatnonzero(one == m)
            q[at], e[at] = table[m][0][at], table[m][1][at]
        per_seat.append((q, e))
    if layout == "seats":
        return np.stack([q for q, _ in per_seat], 1), np.stack([e for _, e in per_seat], 1)
    return per_seat[0]


def test_precision_argument_selects_the_class(evg, env):
    t = pcases.team("mini", (80,), "integer", 2)
    assert type(_pop(env, "mini", t, precision="fp32")) is evg.QPopulation and type(_pop(env, "mini", t)) is evg.QPopulationBf16
    assert type(env.q_population([_dev(env, p) for p in t], final_relu=False)) is evg.QPopulation
    s = pcases.team("smart", (60, 60), "integer", 2)
    assert type(_pop(env, "smart", s, precision="fp32")) is evg.SmartQPopulation and type(_pop(env, "smart", s)) is evg.SmartQPopulationBf16
    with pytest.raises(ValueError, match=r'precision must be "fp32" or "bf16" \(got \'int8\'\)'):
        _pop(env, "smart", s, precision="int8")


# ---------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("layout", pcases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden,family", cases.EXACT_CASES, ids=cases.EXACT_IDS)
def test_exact_tier_is_bit_equal_to_the_composed_host_model(evg, env, kind, hidden, family, layout):
    """every id pattern x 1, 15, 16, 17, 37 rows x teams of 1, 2, 4, 16 (two seats: 2 and 5, 5 and 2); the rows of nobody are zeros, the floats on both
    sides of q_out keep their sentinel, the status bit is set exactly when an id names nobody"""
    sizes = [(2, 5), (5, 2)] if layout == "seats" else pcases.TEAM_SIZES
    top = 5 if layout == "seats" else 16
    inputs = pcases.case_inputs(family, layout)
    full = [pcases.team(kind, hidden, family, top, p) for p in range(2)]
    # (tests/test_population_bf16_model.py has shown that these cases pass the model's exact=True: the float64 value is the fp32 value)
    tables = _member_tables(kind, layout, full if layout == "seats" else full[0], inputs, False, True)
    calls = 0
    for K in sizes:
        for final_relu in ((False, True) if K in (4, (2, 5)) else (False,)):
            pop = _pop(env, kind, full[0][:K[0]], full[1][:K[1]], final_relu) if layout == "seats" else _pop(env, kind, full[0][:K], None, final_relu)
            for pattern in pcases.PATTERNS:
                for rows in cases.ROWS:
                    ids = pcases.layout_ids(pattern, layout, rows, K)
                    want, _ = _select(tables, layout, ids, rows, K)
                    want = _relu(want) if final_relu else want
                    whole, out = _guarded(env, _shape(kind, layout, rows))
                    got = _run(env, evg, pop, layout, cases.first_rows("expanded" if layout == "expanded" else "compact", inputs, rows), ids, out=out)
                    got = got.cpu().numpy()
                    assert cases.same_values(got, want), (K, final_relu, pattern, rows)
                    w = whole.cpu().numpy()
                    assert (w[:16] == SENTINEL).all() and (w[-16:] == SENTINEL).all(), (K, pattern, rows)
                    calls += 1
            assert pop.status() == evg._lib.POP_S_BAD_MEMBER   # (the pattern "bad")
    if family == "nonfinite":                                  # the damage reached the damaged members' rows, and the model holds every NaN there is
        assert np.isnan(tables[0][1][0]).any() and not np.isnan(tables[0][0][0][np.arange(cases.MAX_ROWS) % 7 == 0]).any()
    print("%s %s %s %s: %d calls bit-equal" % (kind, hidden, family, layout, calls))


# ---------------------------------------------------------------------- every row against its member's plain evaluator; the random tier's bound
@pytest.mark.parametrize("layout", pcases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_rows_equal_their_members_plain_evaluator_and_stay_within_the_bound(evg, env, kind, hidden, layout):
    """signed, absorbed, zero_column (random tier: bit-equal to the member's own bf16 evaluator in the same layout, and within the host model's E) and
    integer, nonfinite (bit-equal to the plain evaluator as well), teams of 4 (two seats: 2 and 5)"""
    import torch
    single = env.smart_qnet if kind == "smart" else env.minimized_qnet
    K = (2, 5) if layout == "seats" else 4
    worst = 0.0
    for family in cases.RANDOM_FAMILIES + ["integer", "nonfinite"]:
        if family == "nonfinite" and (kind, hidden) not in cases.NONFINITE_NETS:
            continue
        inputs = pcases.case_inputs(family, layout)
        rows = pcases.num_rows(layout, inputs)
        dinputs = _dev(env, inputs)
        teams = [pcases.team(kind, hidden, family, 5 if layout == "seats" else 4, p) for p in range(2)]
        for final_relu in (False, True):
            if layout == "seats":
                pop = _pop(env, kind, teams[0][:2], teams[1], final_relu)
                plain = [single((_dev(env, teams[0][m % 2]), _dev(env, teams[1][m])), final_relu=final_relu, precision="bf16")(*dinputs).cpu().numpy()
                         for m in range(5)]
                tables = [[plain[0][:, 0], plain[1][:, 0]], [plain[m][:, 1] for m in range(5)]]
            else:
                pop = _pop(env, kind, teams[0], None, final_relu)
                nets = [single(_dev(env, p), final_relu=final_relu, precision="bf16") for p in teams[0]]
                tables = [[(n.expanded(dinputs) if layout == "expanded" else n(*dinputs)).cpu().numpy() for n in nets]]
            for pattern in ("round_robin", "bad", "exact17"):
                ids = pcases.layout_ids(pattern, layout, rows, K)
                got = _run(env, evg, pop, layout, dinputs, ids).cpu().numpy()
                want = np.zeros_like(got)
                for p, table in enumerate(tables):
                    one, g = (ids[:, p], want[:, p]) if layout == "seats" else (ids, want)
                    for m, t in enumerate(table):
                        g[one == m] = t[one == m]
                assert _bits(got, want), (family, final_relu, pattern)
                if family in cases.RANDOM_FAMILIES:
                    q, E = pcases.forward(kind, layout, teams if layout == "seats" else teams[0], inputs, ids, final_relu)
                    ok, ratio = cases.within_bound(got, q, E)
                    worst = max(worst, ratio)
                    assert ok, (family, final_relu, pattern, ratio)
    WORST[(kind, hidden, layout)] = worst
    print("%s %s %s: worst |Q^ - Q| / E = %.4f (so far, all cases: %.4f)" % (kind, hidden, layout, worst, max(WORST.values())))


# ---------------------------------------------------------------------- rows of nobody, published results
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_nobodys_rows_are_zeros_and_the_published_lists_are_the_fp32_populations(evg, env, kind, hidden):
    import torch
    K, rows = 4, 1000
    team = pcases.team(kind, hidden, "signed", K)
    x = np.random.default_rng(3).standard_normal((rows, 59)).astype(np.float32)
    pops = {p: _pop(env, kind, team, None, False, p) for p in ("fp32", "bf16")}
    clean = pcases.ids("round_robin", rows, K)
    for name, pop in pops.items():
        _run(env, evg, pop, "expanded", x, clean)
        assert pop.status() == 0
        pop.check()
    ids = pcases.ids("bad", rows, K)
    got = {}
    for name, pop in pops.items():
        whole, out = _guarded(env, (rows, cases.OUT[kind]))
        got[name] = _run(env, evg, pop, "expanded", x, ids, out=out).cpu().numpy()
        assert not got[name][ids >= K].any() and got[name][ids < K].any(1).all()
        assert pop.status() == evg._lib.POP_S_BAD_MEMBER
        with pytest.raises(evg.EvgError, match="population status 1"):
            pop.check()
    a, b = pops["fp32"], pops["bf16"]
    order, first, count = pedge.bucket_reference(ids, K)
    for pop in (a, b):
        index, f, c = pop.lists()
        assert np.array_equal(index[0, :rows].cpu().numpy(), order) and np.array_equal(f.cpu().numpy(), first) and np.array_equal(c.cpu().numpy(), count)
    assert torch.equal(a.rows_per_member, b.rows_per_member) and a.rows_per_member[0, :K].cpu().tolist() == count[:K].tolist()
    assert not _bits(got["fp32"], got["bf16"])                 # (the precision is not ignored)
    # the two-seat layout publishes both slots
    shared, swarm = edge.compact_inputs("signed", seats=2)
    ids2 = pcases.layout_ids("bad", "seats", shared.shape[0], (K, K))
    for pop in (a, b):
        _run(env, evg, pop, "seats", (shared, swarm), ids2)
    assert torch.equal(a.rows_per_member, b.rows_per_member) and torch.equal(a._bins, b._bins)
    assert torch.equal(a._index.view(-1)[:2 * shared.shape[0]], b._index.view(-1)[:2 * shared.shape[0]])     # slot 1's list begins at word `rows`


# ---------------------------------------------------------------------- the second sweep of the capped grid
@pytest.mark.parametrize("split", pedge.SPLITS)
@pytest.mark.parametrize("family", ["integer", "permutation"])
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_second_sweep_of_the_capped_grid(evg, env, kind, hidden, family, split):
    """rows = one full sweep of the grid + one group + one row over four members in population_edge_cases' splits, expanded and one-seat compact: a
    member whose share of the grid is short of its need strides over its list a second time.  A row the kernel skips keeps its sentinel."""
    import torch
    cus = torch.cuda.get_device_properties(env.device).multi_processor_count
    rows = cases.sweep_rows(cus)
    ids = pedge.split_ids(split, rows)
    pick = cases.sweep_checked_rows(rows, cus)
    team = pcases.team(kind, hidden, family, 4)
    pop = _pop(env, kind, team, None, True)
    for layout in ("expanded", "seat"):
        inputs = pcases.case_inputs(family, layout, rows)
        want, _ = pcases.forward(kind, layout, team, cases.pick_rows(pcases.model_layout(layout), inputs, pick), ids[pick], True)
        out = torch.full(_shape(kind, layout, rows), SENTINEL, dtype=torch.float32, device=env.device)
        got = _run(env, evg, pop, layout, inputs, ids, out=out).cpu().numpy()
        assert (got >= 0).all(), (layout, int((got < 0).sum()))          # final ReLU on: every row was written
        assert cases.same_values(got[pick], want), layout
    assert pop.status() == 0


# ---------------------------------------------------------------------- repeatability and capture
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_two_calls_and_a_captured_call_give_the_same_bits(evg, env, kind, hidden):
    import torch
    K = (2, 5)
    teams = [pcases.team(kind, hidden, "signed", K[p], p) for p in range(2)]
    pop = _pop(env, kind, teams[0], teams[1], False)
    shared, swarm = _dev(env, edge.compact_inputs("signed", seats=2))
    rows = shared.shape[0]
    ids = _dev(env, pcases.layout_ids("round_robin", "seats", rows, K))
    out = torch.empty(_shape(kind, "seats", rows), dtype=torch.float32, device=env.device)
    s = torch.cuda.Stream(env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(s):
        _run(env, evg, pop, "seats", (shared, swarm), ids, out=out)       # warm-up outside the capture
    torch.cuda.current_stream(env.device).wait_stream(s)
    eager = out.clone()
    out.fill_(SENTINEL)
    _run(env, evg, pop, "seats", (shared, swarm), ids, out=out)
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                              # four launches on one stream: no parallel branches
        _run(env, evg, pop, "seats", (shared, swarm), ids, out=out)
    out.fill_(SENTINEL)
    g.replay()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    ids.copy_(_dev(env, pcases.layout_ids("blocks", "seats", rows, K)))   # the replay reads the ids as they are now
    g.replay()
    want = _run(env, evg, pop, "seats", (shared, swarm), ids)
    assert torch.equal(out, want) and not torch.equal(out, eager)


# ---------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_refusals_are_those_of_the_fp32_entry_points_with_their_text(evg, env, kind, hidden):
    import torch
    _lib = evg._lib
    B = _lib.load_popbf16()
    fp32, bf16 = (B.evg_smart_population_qnet, B.evg_smart_population_qnet_bf16) if kind == "smart" else (B.evg_population_qnet, B.evg_population_qnet_bf16)
    pop = _pop(env, kind, pcases.team(kind, hidden, "signed", 3), None, False)
    shared, swarm = _dev(env, edge.compact_inputs("signed"))
    N = shared.shape[0]
    ids = _dev(env, pcases.ids("round_robin", N, 3))
    out = torch.full((N, 12, cases.OUT[kind]), 7.0, dtype=torch.float32, device=env.device)
    pop._descriptor(N)
    good = type(pop._desc).from_buffer_copy(pop._desc)

    def desc(**kw):
        d = type(good).from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    no_w1 = desc()
    no_w1.w1[0][1] = None
    odd_b1 = desc()
    odd_b1.b1[0][2] = good.b1[0][2] + 4
    many = desc()
    many.num_members[0] = 17
    base = dict(d=good, layout=_lib.QNET_COMPACT, rows=N, seat=0, member=ids.data_ptr(), in0=shared.data_ptr(), in1=swarm.data_ptr(), q=out.data_ptr())
    bad = [dict(layout=7), dict(seat=2), dict(seat=-1), dict(rows=0), dict(rows=(1 << 24) + 1), dict(rows=good.scratch_rows + 1), dict(member=None),
           dict(in0=None), dict(in1=None), dict(q=None), dict(in0=shared.data_ptr() + 4), dict(in1=swarm.data_ptr() + 8), dict(q=out.data_ptr() + 4),
           dict(d=desc(struct_size=8)), dict(d=desc(h1=0)), dict(d=desc(h1=129)), dict(d=desc(final_relu=2)), dict(d=many), dict(d=desc(member=None)),
           dict(d=desc(index=None)), dict(d=desc(first=good.first + 2)), dict(d=no_w1), dict(d=odd_b1)]

    def call(fn, a):
        vp = lambda v: None if v is None else C.c_void_p(v)
        rc = fn(env._h, C.byref(a["d"]), a["layout"], a["rows"], a["seat"], vp(a["member"]), vp(a["in0"]), vp(a["in1"]), vp(a["q"]), None)
        return rc, B.evg_last_error()

    for change in bad:
        a = dict(base, **change)
        want, got = call(fp32, a), call(bf16, a)
        assert want[0] == got[0] == _lib.ERR_ARG and want[1] == got[1] and len(got[1]) > 10, (change, want, got)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                            # nothing was launched
    assert call(bf16, base)[0] == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).any())


def test_fp32_populations_are_unchanged_with_the_new_library_loaded(evg, env):
    """QPopulation / SmartQPopulation give each member's fp32 evaluator bit for bit, before and after libevg_popbf16.so is loaded and used"""
    outs = {}
    for stage in ("before", "after"):
        for kind, hidden in (("smart", (60, 60)), ("mini", (80,))):
            team = pcases.team(kind, hidden, "signed", 4)
            inputs = edge.compact_inputs("signed")
            ids = pcases.ids("round_robin", inputs[0].shape[0], 4)
            got = _run(env, evg, _pop(env, kind, team, None, True, "fp32"), "seat", inputs, ids).cpu().numpy()
            single = env.smart_qnet if kind == "smart" else env.minimized_qnet
            for m in range(4):
                assert _bits(got[ids == m], single(_dev(env, team[m]), final_relu=True)(*_dev(env, inputs)).cpu().numpy()[ids == m])
            outs[(stage, kind)] = got
        evg._lib.load_popbf16()
        _run(env, evg, _pop(env, "smart", pcases.team("smart", (60, 60), "signed", 4), None, True), "seat", edge.compact_inputs("signed"),
             pcases.ids("round_robin", edge.ENVS_COMPACT, 4))
    for kind in ("smart", "mini"):
        assert _bits(outs[("before", kind)], outs[("after", kind)])


# ---------------------------------------------------------------------- use: a self-play turn, the learner, the examples
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_one_self_play_turn_draws_the_members_of_an_fp32_population_on_a_twin_handle(evg, kind, hidden):
    import torch
    N, K = 256, (4, 3)
    teams = [pcases.team(kind, hidden, "signed", K[p], p) for p in range(2)]
    members, hists = [], []
    for precision in ("fp32", "bf16"):
        e = evg.EvergladesVecEnv(N, seed=31, auto_reset=True)
        obs = e.reset()
        pop = (e.smart_q_population if kind == "smart" else e.q_population)([_dev(e, p) for p in teams[0]], [_dev(e, p) for p in teams[1]],
                                                                            final_relu=False, precision=precision)
        shared, swarm = torch.zeros((N, 2, 34), device=e.device), torch.zeros((N, 2, 12, 13), device=e.device)
        for p in range(2):
            s, x = e.smart_state_compact(p, obs)
            shared[:, p].copy_(s)
            swarm[:, p].copy_(x)
        before = pop.member.clone()
        q = pop(shared, swarm)
        assert tuple(q.shape) == (N, 2, 12, cases.OUT[kind]) and bool(torch.isfinite(q).all())
        e.step_q(q, (0.2, 0.2), features=(shared, swarm))
        hist = torch.full((N, 2), 99, dtype=torch.uint8, device=e.device)
        pop.end_of_turn(history=hist)
        pop.check()
        assert pop.rows_per_member.sum().item() == 2 * N
        members.append((before.cpu(), pop.member.cpu()))
        hists.append(hist.cpu())
        e.close()
    assert torch.equal(members[0][0], members[1][0]) and torch.equal(members[0][1], members[1][1]) and torch.equal(hists[0], hists[1])
    assert len(set(members[0][0][:, 0].tolist())) == K[0]


@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_learner_with_grouped_bf16_targets(evg, env, kind):
    """target_precision="bf16_grouped" at B = 257, K = 4, double_mean with weights and rows of nobody: q_next and q_select bit-equal to the members' own
    bf16 evaluators (zeros for nobody), the TD head, the backward and Adam within their models' bounds on the device's own previous-stage buffers
    (test_gpu_pop_learner's rule and helper); the same q_next bits as "bf16"; a captured step replays to the same targets"""
    import torch
    import pop_learner_cases as lcases
    import test_gpu_pop_learner as tl
    B, K = 257, 4
    hidden = lcases.HIDDEN[kind][0]
    name = "smart" if kind == "smart" else "minimized"
    team, targets = lcases.random_team(kind, hidden, K, "gathered"), lcases.random_team(kind, hidden, K, "gathered", seed=9)
    lrn, pol, tgt = tl._learner(env, name, team, targets, lr=1e-3, gamma=0.999, n_step=1, mode="double_mean", clamp=1.0, target_precision="bf16_grouped")
    Bf16 = evg.SmartQPopulationBf16 if kind == "smart" else evg.QPopulationBf16
    assert lrn.target_nets is None and lrn.select_nets is None and type(lrn.target_pop) is Bf16 and type(lrn.select_pop) is Bf16
    assert type(lrn.policy_pop) is not Bf16
    batch = tl._batch(kind, B, 3)
    w = (0.1 + 0.9 * np.random.default_rng(3).random(B)).astype(np.float32)
    ids = lcases.ids(B, K, "random", seed=3, nobody=0.2)
    counts = tl._check_step(env, evg, lrn, pol, tgt, kind, batch, ids, w, "double_mean", [0] * K, precision="bf16")
    assert all(counts) and (ids >= K).any()
    q_next = lrn.q_next.cpu().numpy().copy()
    assert not q_next[ids >= K].any() and q_next[ids < K].any()
    old, _, _ = tl._learner(env, name, [tl._np(p) for p in pol], [tl._np(t) for t in tgt], mode="double_mean", target_precision="bf16")
    assert old.target_pop is None and len(old.target_nets) == K
    dbatch, idd, wd = tuple(tl._dev(env, a) for a in batch), tl._dev(env, ids), tl._dev(env, w)
    old.step_on(dbatch, idd, weights=wd)
    assert _bits(old.q_next.cpu().numpy(), q_next)              # "bf16" and "bf16_grouped": the same targets, bit for bit
    ref, _, _ = tl._learner(env, name, [tl._np(p) for p in pol], [tl._np(t) for t in tgt], mode="double_mean")
    ref.step_on(dbatch, idd, weights=wd)
    assert not _bits(ref.q_next.cpu().numpy(), q_next)
    lrn.sync_target([2])
    assert all(_bits(a, b) for a, b in zip(tl._np(tgt[2]), tl._np(pol[2])))
    assert lrn.state_dict()["step"] == [1] * K
    want = lrn.target_pop.expanded(dbatch[2], lrn._buffers(B)["ids12"], 0).cpu().numpy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lrn.step_on(dbatch, idd, weights=wd)
    lrn.q_next.fill_(-1.0)
    g.replay()
    assert _bits(lrn.q_next.cpu().numpy(), want) and lrn.ctl[:, 0].cpu().tolist() == [2] * K and bool(torch.isfinite(lrn.loss).all())


@pytest.mark.parametrize("example", ["smart_state_self_royale.py", "minimized_self_royale.py"])
def test_self_royale_examples_run_on_the_bf16_matrix_cores(example):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", example), "256", "12", "64", "--acting-precision", "bf16", "--device-learner"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "device learner" in out.stdout and "all finite: True" in out.stdout, out.stdout[-2000:]
