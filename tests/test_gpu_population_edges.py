"""GPU tests of the population kernels (csrc/population_kernels.inc) at their edges; the cases are tests/population_edge_cases.py, shown on the CPU by
tests/test_population_edge_cases.py to reach what they name:

  A  the grouped forwards evg_mini_qnet_pop_kernel / evg_qnet_pop_kernel under the eight numeric families of tests/learner_edge_cases.py, at every hidden
     size of that module, in the three layouts and with both final_relu settings: teams of four in which ordinary and damaged weight sets alternate, rows
     dealt to the members in runs of three -- against the host model of each member over its rows, by value with equal NaN masks;
  B  the capped grid past one sweep (cases.sweep_rows: 32 785 rows on 256 CUs) in four splits over four members, Minimized in all layouts and the
     Smart_State compact ones -- against fresh plain launches over chunks of 4 096 rows merged by member, and against the host model on 1 169 rows;
  C  the bucket pass at 256, 257 and 513 blocks (per = 1, 2, 3 block counts per thread of the scan kernel): the published stable list, first and count
     against numpy's stable argsort, read by the layout include/evg.h states (seat slot s's list begins at index + s * rows of the call), with a two-seat
     population whose scratch_rows exceeds the call's rows; the forward against plain launches merged, zeros on the rows whose id names nobody.

Every output is a guarded view (64 sentinels on each side)."""
import numpy as np
import pytest

import learner_edge_cases as cases
import population_edge_cases as pec

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]     # (numpy's warnings of the overflow the cases are about)

NETS = [("smart", h) for h in cases.SMART_HIDDEN] + [("mini", h) for h in cases.MINI_HIDDEN]
GUARD = 64
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)        # noqa: E731


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


_ENVS = {}


def _env(evg, N):
    if N not in _ENVS:
        _ENVS[N] = evg.EvergladesVecEnv(N, seed=5, auto_reset=True)
        _ENVS[N].reset()
    return _ENVS[N]


def _dev(env, a):
    import torch
    if isinstance(a, (tuple, list)):
        return tuple(_dev(env, x) for x in a)
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _cus(env):
    import torch
    return torch.cuda.get_device_properties(env.device).multi_processor_count


class _Guarded(object):
    """an output tensor with GUARD sentinels on each side"""

    def __init__(self, env, shape, fill=-77.0):
        import torch
        n = int(np.prod(shape))
        self.fill, self.n = fill, n
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=env.device)
        self.out = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())


def _population(env, kind, teams, final_relu, max_rows=None):
    """teams: one team (played on both seats) or two, of host parameter tuples"""
    make = env.smart_q_population if kind == "smart" else env.q_population
    dev = [[_dev(env, m) for m in t] for t in teams]
    return make(dev[0], dev[1] if len(dev) == 2 else None, final_relu=final_relu, max_rows=max_rows), dev


def _grouped(pop, layout, dev_inputs, dev_member, out):
    """the grouped forward of one layout; the one-seat layouts play seat 0's team"""
    if layout == "expanded":
        return pop.expanded(dev_inputs, dev_member, 0, out=out)
    if layout == "seat":
        return pop.seat(dev_inputs[0], dev_inputs[1], dev_member, 0, out=out)
    pop.member.copy_(dev_member)
    return pop(dev_inputs[0], dev_inputs[1], out=out)


def _out_shape(kind, layout, rows):
    o = 5 if kind == "smart" else 11
    return {"expanded": (rows, o), "seat": (rows, 12, o), "seats": (rows, 2, 12, o)}[layout]


def _rows_per_member_match(pop, member):
    import torch
    ids = np.asarray(member).reshape(len(member), -1)
    K = pop.num_members if ids.shape[1] == 2 else (pop.num_members[0],)
    for s in range(ids.shape[1]):
        ok = ids[:, s] < K[s]
        want = np.bincount(ids[ok, s], minlength=16)
        if not torch.equal(pop.rows_per_member[s].long().cpu(), torch.as_tensor(want).long()):
            return False
    return True


def _report(tag, got, want):
    """the figures of a comparison, printed before it is asserted"""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    both = ~nan_g & ~nan_w
    print("%s: %d values, NaN %d (reference %d), Inf %d (reference %d), subnormal %d (reference %d), NaN masks differ at %d, values differ at %d" % (
        tag, got.size, nan_g.sum(), nan_w.sum(), np.isinf(got).sum(), np.isinf(want).sum(), cases.is_subnormal(got).sum(),
        cases.is_subnormal(want).sum(), (nan_g != nan_w).sum(), (got[both] != want[both]).sum()))


# ------------------------------------------------------------------------------------------------------------------ A: the numeric edges
_MODEL_Q = {}


def _model_q(kind, hidden, family, layout):
    """the host model's Q without the final ReLU, computed once per case (with it: the model's own np.maximum on top, as qnet_model.layer applies it)"""
    key = (kind, hidden, family, layout)
    if key not in _MODEL_Q:
        inputs, member = pec.case_inputs(family, layout)
        teams = [pec.team(kind, hidden, family, p) for p in range(2)]
        _MODEL_Q[key] = pec.team_model_q(kind, layout, teams if layout == "seats" else teams[0], inputs, member)
        _MODEL_Q[key].setflags(write=False)
    return _MODEL_Q[key]


@pytest.mark.parametrize("layout", pec.LAYOUTS)
@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("kind,hidden", NETS, ids=_ids)
def test_grouped_forwards_equal_the_host_model_at_the_numeric_edges(evg, kind, hidden, family, layout):
    env = _env(evg, cases.ENVS_COMPACT)
    inputs, member = pec.case_inputs(family, layout)
    teams = [pec.team(kind, hidden, family, p) for p in range(2)]
    dev_inputs, dev_member = _dev(env, inputs), _dev(env, member)
    raw = _model_q(kind, hidden, family, layout)
    rows = raw.shape[0]
    ids = member.reshape(rows, -1)
    ordinary = ~np.isin(ids, pec.DAMAGED_MEMBERS)
    bad = pec.damaged_inputs(family, layout, inputs).reshape(rows, -1)
    for final_relu in (False, True):
        want = np.maximum(raw, np.float32(0)) if final_relu else raw
        pop, _ = _population(env, kind, teams, final_relu)
        g = _Guarded(env, _out_shape(kind, layout, rows))
        got_t = _grouped(pop, layout, dev_inputs, dev_member, g.out)
        got = got_t.cpu().numpy()
        tag = (kind, hidden, family, layout, final_relu)
        _report("%s %s %s %s final_relu=%d" % tag, got, want)
        assert got_t is g.out and g.intact(), tag
        assert cases.same_values(got, want), tag
        assert pop.status() == 0 and _rows_per_member_match(pop, member), tag
        # what a damaged member or row must not reach, said of the device output itself
        flat = got.reshape(rows, ids.shape[1], -1)
        if family != "overflow":
            assert not np.isnan(flat[ordinary & ~bad]).any(), tag
        if family == "absorbed" and min(hidden) >= 17:
            assert np.isfinite(flat[bad & ~ordinary]).all() and np.isnan(flat[bad & ordinary]).any(-1).all(), tag
        if family in ("nan_weight", "inf_bias") and min(hidden) >= 16 and not final_relu:
            assert (~np.isfinite(flat[~ordinary])).any(-1).all(), tag


# ------------------------------------------------------------------------------------------------------------------ B: past one sweep of the capped grid
SWEEP_NETS = [("mini", (80,), lay) for lay in pec.LAYOUTS] + [("mini", (128,), lay) for lay in pec.LAYOUTS] + \
             [("smart", (60, 60), "seat"), ("smart", (60, 60), "seats")]        # (Smart expanded: tests/test_gpu_smart_population.py, test_a_grid_at_its_cap)
_SWEEP = {}


def _sweep_case(env, family, layout, R):
    """device inputs of a sweep case, uploaded once per (family, layout)"""
    key = (family, layout, R)
    if key not in _SWEEP:
        inputs = cases.expanded_inputs(family, R) if layout == "expanded" else cases.compact_inputs(family, R, 2 if layout == "seats" else 1)
        _SWEEP.clear()                                                      # one case resident at a time
        _SWEEP[key] = (inputs, _dev(env, inputs))
    return _SWEEP[key]


def _plain(env, kind, params, final_relu):
    make = env.smart_qnet if kind == "smart" else env.minimized_qnet
    return make(params, final_relu=final_relu)


def _merged_plain(env, kind, layout, dev_teams, final_relu, dev_inputs, dev_member, chunk, zeros_for_bad=False):
    """The plain kernel's answer: one fresh plain launch per member and chunk of `chunk` rows, merged by torch.where on the member ids.  dev_teams: the
    team of the call's seat, or both teams (two-seat layout: launches of pairs).  Rows whose id names nobody stay NaN, or zeros with zeros_for_bad."""
    import torch
    rows = (dev_inputs if layout == "expanded" else dev_inputs[0]).shape[0]
    want = torch.full(_out_shape(kind, layout, rows), 0.0 if zeros_for_bad else float("nan"), device=env.device)
    K = max(len(t) for t in dev_teams) if layout == "seats" else len(dev_teams)
    for m in range(K):
        if layout == "seats":
            net = _plain(env, kind, tuple(t[min(m, len(t) - 1)] for t in dev_teams), final_relu)
        else:
            net = _plain(env, kind, dev_teams[m], final_relu)
        for lo in range(0, rows, chunk):
            hi = min(lo + chunk, rows)
            if layout == "expanded":
                q = net.expanded(dev_inputs[lo:hi])
            else:
                q = net(dev_inputs[0][lo:hi], dev_inputs[1][lo:hi])
            mine = dev_member[lo:hi] == m
            if layout == "seats":
                for p in range(2):
                    if m < len(dev_teams[p]):
                        want[lo:hi, p] = torch.where(mine[:, p][:, None, None], q[:, p], want[lo:hi, p])
            else:
                want[lo:hi] = torch.where(mine.view((-1,) + (1,) * (q.dim() - 1)), q, want[lo:hi])
    return want


@pytest.mark.parametrize("split", pec.SPLITS)
@pytest.mark.parametrize("family", ["signed", "nonfinite"])
@pytest.mark.parametrize("kind,hidden,layout", SWEEP_NETS, ids=_ids)
def test_grouped_forward_past_one_sweep_of_the_capped_grid(evg, kind, hidden, layout, family, split):
    """R rows = one full sweep of the capped grid (2 workgroups per CU x 4 wavefronts x 16 rows) + one group + one row.  `one` and `crumbs`: a member whose
    workgroups are the whole grid loops over list_stride; `three_quarters`: member 0's share of the grid (live) is one workgroup below its need, so its
    wavefronts stride by live * 4 groups and one of them sweeps twice, ending on a partial group; `even`: four shares of a quarter."""
    cus = _cus(_env(evg, cases.ENVS_COMPACT))
    R = cases.sweep_rows(cus)
    env = _env(evg, R) if layout == "seats" else _env(evg, cases.ENVS_COMPACT)
    final_relu = family == "nonfinite"
    ids0 = pec.split_ids(split, R)
    if split == "three_quarters":
        cnt = int((ids0 == 0).sum())
        live, need = pec.share(cnt, R, cus)
        assert live < need and live * 64 < cnt, (cnt, live, need)
    member = np.stack([ids0, ids0[::-1]], 1) if layout == "seats" else ids0              # seat slot 1: the split mirrored
    teams = [[cases.net_params(kind, hidden, family, which=pec.MEMBERS * p + m) for m in range(pec.MEMBERS)] for p in range(2 if layout == "seats" else 1)]
    inputs, dev_inputs = _sweep_case(env, family, layout, R)
    dev_member = _dev(env, member)
    pop, dev_teams = _population(env, kind, teams, final_relu, max_rows=R)
    g = _Guarded(env, _out_shape(kind, layout, R))
    got_t = _grouped(pop, layout, dev_inputs, dev_member, g.out)
    assert got_t is g.out and g.intact()
    assert pop.status() == 0 and _rows_per_member_match(pop, member)
    # all rows: fresh plain launches over chunks of 4 096 rows (every row of them inside a plain kernel's first sweep), merged by member
    want_t = _merged_plain(env, kind, layout, dev_teams if layout == "seats" else dev_teams[0], final_relu, dev_inputs, dev_member, 4096)
    got, want = got_t.cpu().numpy(), want_t.cpu().numpy()
    tag = "sweep %d rows (%d CUs) %s %s %s %s %s" % (R, cus, kind, hidden, layout, family, split)
    _report(tag + " vs plain", got, want)
    assert cases.same_values(got, want), tag
    # the checked rows: the host model of each row's member
    pick = cases.sweep_checked_rows(R, cus)
    model = pec.team_model_q(kind, layout, teams if layout == "seats" else teams[0], inputs, member, rows=pick)
    if final_relu:
        model = np.maximum(model, np.float32(0))
    _report(tag + " vs model", got[pick], model)
    assert cases.same_values(got[pick], model), tag
    if family == "nonfinite":
        clean = ~pec.damaged_inputs(family, layout, inputs)
        assert np.isfinite(got[clean]).all() and not np.isfinite(got[~clean]).all()


# ------------------------------------------------------------------------------------------------------------------ C: the bucket pass at and past 256 blocks
def _published_lists(pop, rows, slots):
    """The bucket pass's results of the last forward as include/evg.h states them: seat slot s's list begins at index + s * rows, with the `rows` of that
    call (not at s * scratch_rows); first / count are [slot][17].  -> [(list, first, count)] per slot, host arrays."""
    index = pop._index.view(-1).cpu().numpy()
    bins = pop._bins.cpu().numpy()
    return [(index[s * rows:(s + 1) * rows], bins[0, s], bins[1, s]) for s in range(slots)]


BUCKET_CASES = [("mini", (17,), "expanded", rows, pat) for rows in pec.BUCKET_ROWS for pat in pec.PATTERNS if pat != "window" or rows > pec.WINDOW[1]] + \
               [("mini", (17,), "seats", 65537, pat) for pat in ("uniform", "one", "bad")] + \
               [("smart", (60, 60), "expanded", 65537, pat) for pat in ("uniform", "one", "bad")]


@pytest.mark.parametrize("kind,hidden,layout,rows,pattern", BUCKET_CASES, ids=_ids)
def test_bucket_pass_at_and_past_256_blocks(evg, kind, hidden, layout, rows, pattern):
    """65 536 rows: 256 blocks, the last size at which each thread of evg_population_scan_kernel owns one block count; 65 537: 257 blocks, two per
    thread, thread 128 owning the single last one; 131 073: 513 blocks, three per thread.  The two-seat population keeps its default scratch of 12 * N
    rows: seat slot 1's list at index + rows and the one a stride of scratch_rows would name are different words."""
    import torch
    K = pec.BUCKET_K
    slots = 2 if layout == "seats" else 1
    env = _env(evg, rows) if layout == "seats" else _env(evg, cases.ENVS_COMPACT)
    ids = np.stack([pec.bucket_ids(pattern, rows, s) for s in range(slots)], 1)          # [rows, slots]
    member = ids if slots == 2 else ids[:, 0]
    teams = [[cases.net_params(kind, hidden, "signed", which=8 * p + m) for m in range(K)] for p in range(slots)]
    inputs = cases.compact_inputs("signed", rows, 2) if layout == "seats" else cases.expanded_inputs("signed", rows)
    dev_inputs, dev_member = _dev(env, inputs), _dev(env, member)
    pop, dev_teams = _population(env, kind, teams, True)
    if slots == 2:
        assert pop._desc.scratch_rows == 12 * rows
        pop._index.fill_(-1)                                                # stale words, were anything to read the list elsewhere
    g = _Guarded(env, _out_shape(kind, layout, rows))
    got_t = _grouped(pop, layout, dev_inputs, dev_member, g.out)
    assert got_t is g.out and g.intact()
    # the published list, first and count
    for s, (lst, first, count) in enumerate(_published_lists(pop, rows, slots)):
        want_list, want_first, want_count = pec.bucket_reference(ids[:, s], K)
        tag = (rows, pattern, s)
        assert np.array_equal(count, want_count), (tag, count.tolist(), want_count.tolist())
        assert np.array_equal(first, want_first), (tag, first.tolist(), want_first.tolist())
        assert np.array_equal(lst, want_list), (tag, int((lst != want_list).sum()), int(np.flatnonzero(lst != want_list)[0]))
    bad = ids >= K
    assert _rows_per_member_match(pop, member)
    assert pop.status() == (evg._lib.POP_S_BAD_MEMBER if pattern == "bad" else 0) and bad.any() == (pattern == "bad")
    # the forward on all rows: plain launches merged by member, zeros where the id names nobody
    want_t = _merged_plain(env, kind, layout, dev_teams if slots == 2 else dev_teams[0], True, dev_inputs, dev_member, rows, zeros_for_bad=True)
    diff = int((got_t != want_t).any(-1).sum())
    print("bucket %s %s %s %d rows %s: %d bad ids, %d output rows differ" % (kind, hidden, layout, rows, pattern, int(bad.sum()), diff))
    assert bool(torch.isfinite(want_t).all()) and torch.equal(got_t, want_t), diff
    if pattern == "bad":
        zero = (got_t.cpu().numpy().reshape(rows, slots, -1) == 0).all(-1)
        assert zero[bad].all()                                              # (a row of a member may be all zeros too: the final ReLU is on)
