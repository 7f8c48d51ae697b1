"""GPU tests of the learner step's kernels past their grid caps and of the grouped Adam stage at its edges (include/evg_learn.h,
include/evg_pop_learn.h), on the cases of tests/pop_learner_edge_cases.py, against the existing host models (tests/learner_model.py,
tests/qnet_grad_model.py, tests/pop_learner_model.py):

  TD head   evg_td_head at 16 384, 16 385 and 2 * 16 384 + 19 rows and evg_td_head_grouped on 65 555 rows (members of 32 000, 16 400 and 16 384 rows
            and rows of nobody; members of 32 787, 16 385 and 16 383 rows): the second and third chunk of a workgroup, a slot that adds more than one
            term, the loss order past the cap.  Exact tier bit-equal, random tier within the counted bound and bit-equal to the fp32-order model,
            sentinels around every output.  Out-of-range actions in the grouped head.
  backward  evg_*population_backward on the same 65 555 rows: every member's share of the capped grid is below its need, so the stride loop runs
            twice; 16 members whose partials fill the packed workspace to X + K - 1; the random tier; rows of nobody deleted.
  Adam      evg_adam_step_grouped called as a stage on tensors the test owns, every one of them with sentinels: different control blocks in one
            launch, zero and extreme gradients, the clamp, fresh_state, members without rows.

Worst ratios to the counted bounds, printed by the tests and recorded in CHANGELOG.md."""
import numpy as np
import pytest

import learner_cases as cases
import learner_model as model
import pop_learner_cases as pcases
import pop_learner_edge_cases as ecases
import pop_learner_model as pmodel
import qnet_grad_cases as gcases

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
KW = dict(lr=float(F32(1e-3)), betas=(float(F32(0.9)), float(F32(0.999))), eps=float(F32(1e-8)))
KEYS = ("estimated", "gq", "priorities", "loss")
WORST = {}
Guarded = ecases.Guarded


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


@pytest.fixture(scope="module")
def G(evg):
    return evg._lib.load_learn()


def _dev(env, a):
    import torch
    if a is None:
        return None
    if isinstance(a, (tuple, list)):
        return [_dev(env, x) for x in a]
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _np(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)


def _cus(env):
    import torch
    return torch.cuda.get_device_properties(env.device).multi_processor_count


TD_OPERANDS = ("q_pred", "action", "q_next", "q_select", "reward", "not_done", "weights")


# ---------------------------------------------------------------------- 1. the TD head past the block cap: the plain entry point
_WS = {}


def _td_plain(evg, env, G, c):
    """one evg_td_head call on the case c: the four outputs as numpy, the sentinels on both sides of each checked"""
    import ctypes as C
    import torch
    _lib = evg._lib
    if "td" not in _WS:
        _WS["td"] = torch.empty(_lib.TD_HEAD_WORKSPACE_BYTES // 4, dtype=torch.float32, device=env.device)
    B, OUT = c["q_pred"].shape
    dev = {k: _dev(env, c[k]) for k in TD_OPERANDS}
    out = {"gq": Guarded(env, (B, OUT)), "loss": Guarded(env, (1,)), "priorities": Guarded(env, (B,)), "estimated": Guarded(env, (B,))}
    d = _lib.EvgTdHeadArgs()
    d.struct_size = C.sizeof(d)
    d.mode, d.batch, d.out, d.scale = _lib.TD_MODES[c["mode"]], B, OUT, float(c["scale"])
    for k, t in dev.items():
        setattr(d, k, None if t is None else t.data_ptr())
    for k in ("gq", "loss", "priorities", "estimated"):
        setattr(d, k, out[k].t.data_ptr())
    d.workspace, d.workspace_bytes = _WS["td"].data_ptr(), _WS["td"].numel() * 4
    rc = G.evg_td_head(env._h, C.byref(d), env._stream())
    assert rc == 0, G.evg_last_error()
    got = {k: o.numpy() for k, o in out.items()}
    got["loss"] = got["loss"][0]
    return got


@pytest.mark.parametrize("B,OUT,mode,weighted", ecases.PLAIN_TD, ids=ecases.PLAIN_IDS)
def test_td_head_past_the_block_cap_exact_random_and_the_loss_order(evg, env, G, B, OUT, mode, weighted):
    """16 384 rows: chunks == EVG_TD_HEAD_MAX_BLOCKS, one pass; 16 385: workgroup 0 alone takes a second chunk, of one live row; 32 787: every
    workgroup takes two chunks and two a third, the last of 3 rows.  The exact tier is bit-equal to the model; the random tier stays within the counted
    bound and is bit-equal to the fp32-order model, whose loss sum is learner_model.loss_order32's for chunks > MAX_BLOCKS."""
    c = cases.td_exact(B, OUT, mode, weighted)
    want, _ = model.td_head(exact=True, **c)
    got = _td_plain(evg, env, G, c)
    for k in KEYS:
        assert cases.same_bits(got[k], want[k]), ("exact", k, np.asarray(got[k]).ravel()[:4], np.asarray(want[k]).ravel()[:4])
    assert (got["gq"] != 0).sum() <= B and want["loss"] != 0
    c = cases.td_random(B, OUT, mode, weighted)
    want, E = model.td_head(**c)
    got = _td_plain(evg, env, G, c)
    for k in KEYS:
        ok, ratio = cases.within(got[k], want[k], E[k])
        _record("td plain " + k, ratio)
        print("plain B=%d OUT=%d %s weighted=%d %s: |device - model| / E = %.4f" % (B, OUT, mode, weighted, k, ratio))
        assert ok, (k, ratio)
    w32 = model.td_head32(**c)
    for k in KEYS:
        assert cases.same_bits(got[k], w32[k]), ("fp32 order", k, got[k] if k == "loss" else None, w32[k] if k == "loss" else None)
    c = ecases.td_signed(B, OUT, mode)                          # a loss that cancels: its bits depend on the order of the sum
    got, w32 = _td_plain(evg, env, G, c), model.td_head32(**c)
    for k in KEYS:
        assert cases.same_bits(got[k], w32[k]), ("fp32 order, signed weights", k, got["loss"], w32["loss"])
    print("worst ratio to the bound so far:", WORST)


# ---------------------------------------------------------------------- the grouped stages: learners and lists
def _learner(env, kind, team, final_relu, **kw):
    """-> (learner, the policies' device tensors): networks as tuples of tensors; the targets are copies of the policies"""
    pol = [tuple(_dev(env, p)) for p in team]
    tgt = [tuple(_dev(env, p)) for p in team]
    make = env.smart_population_learner if kind == "smart" else env.minimized_population_learner
    return make(pol, tgt, final_relu=final_relu, **kw), pol


def _lists(env, lrn, x, ids):
    """the policy forward that leaves the lists: -> (x on the device, its buffers); the counts are the intended ones"""
    xd, idd = _dev(env, x), _dev(env, ids)
    b = lrn._buffers(len(ids))
    lrn.policy_forward(xd, idd, b["q_pred"])
    assert lrn.counts.cpu().numpy().tolist() == ecases.counts_of(ids, lrn.K)
    return xd, b


_TD_LEARNERS = {}


def _td_learner(env, OUT, ids, key, K):
    """a learner of K members of the family with OUT outputs whose lists are those of `ids` (kept per key: one forward leaves them once)"""
    if (OUT, key) not in _TD_LEARNERS:
        kind = ecases.KIND_OF_OUT[OUT]
        hidden = pcases.HIDDEN[kind][1]
        lrn, _ = _learner(env, kind, pcases.exact_team(kind, hidden, K), pcases.final_relu(kind), clamp=None)
        x, _ = gcases.inputs(kind, hidden, "integer", len(ids))
        _lists(env, lrn, x, ids)
        _TD_LEARNERS[(OUT, key)] = lrn
    return _TD_LEARNERS[(OUT, key)]


def _td_grouped(env, lrn, c):
    """one evg_td_head_grouped call on the case c with the learner's lists: the four outputs (loss [K]) as numpy, sentinels checked"""
    B, OUT = c["q_pred"].shape
    d = {k: _dev(env, c[k]) for k in TD_OPERANDS}
    out = {"gq": Guarded(env, (B, OUT)), "loss": Guarded(env, (lrn.K,)), "priorities": Guarded(env, (B,)), "estimated": Guarded(env, (B,))}
    lrn.td_head(d["q_pred"], d["action"], d["q_next"], d["q_select"], d["reward"], d["not_done"], d["weights"], out["gq"].t, out["loss"].t,
                out["priorities"].t, out["estimated"].t, mode=c["mode"], scale=float(c["scale"]))
    return {k: o.numpy() for k, o in out.items()}


@pytest.mark.parametrize("how,OUT,mode,weighted", ecases.GROUPED_TD, ids=ecases.GROUPED_IDS)
def test_grouped_td_head_past_the_block_cap_exact_random_and_the_loss_order(env, how, OUT, mode, weighted):
    """65 555 rows, K = 3.  'random' / 'descending': members of 32 000 rows (G capped, 976 workgroups take a second chunk), 16 400 (workgroup 0 alone
    takes a second chunk) and 16 384 (chunks == G) while the grid is sized by the whole batch, and 771 rows of nobody.  'full': 32 787, 16 385 and
    16 383 rows -- a third chunk, partial last chunks on a later pass, no rows of nobody."""
    K = ecases.K_A
    ids = ecases.ids_a(how)
    lrn = _td_learner(env, OUT, ids, how, K)
    nobody = ids >= K
    assert lrn.counts.cpu().numpy().tolist() == list(ecases.COUNTS_FULL if how == "full" else ecases.COUNTS_A)
    c = cases.td_exact(ecases.BIG_B, OUT, mode, weighted)
    want, _ = pmodel.td_head(c, ids, K, exact=True)
    got = _td_grouped(env, lrn, c)
    for k in KEYS:
        assert cases.same_bits(got[k], want[k]), ("exact", k, got["loss"], want["loss"])
    assert not got["gq"][nobody].any() and not got["priorities"][nobody].any() and not got["estimated"][nobody].any()
    c = cases.td_random(ecases.BIG_B, OUT, mode, weighted)
    want, E = pmodel.td_head(c, ids, K)
    got = _td_grouped(env, lrn, c)
    for k in KEYS:
        ok, ratio = cases.within(got[k], want[k], E[k])
        _record("td grouped " + k, ratio)
        assert ok, (k, ratio)
    w32 = pmodel.td_head32(c, ids, K)
    for k in KEYS:
        assert cases.same_bits(got[k], w32[k]), ("fp32 order", k, got["loss"], w32["loss"])
    assert not got["gq"][nobody].any() and not got["priorities"][nobody].any() and not got["estimated"][nobody].any()
    assert got["loss"].all() and lrn.counts.cpu().numpy().tolist() == ecases.counts_of(ids, K)
    c = ecases.td_signed(ecases.BIG_B, OUT, mode)               # a loss that cancels: its bits depend on the order of the sum
    got, w32 = _td_grouped(env, lrn, c), pmodel.td_head32(c, ids, K)
    for k in KEYS:
        assert cases.same_bits(got[k], w32[k]), ("fp32 order, signed weights", k, got["loss"], w32["loss"])
    print("worst ratio to the bound so far:", WORST)


@pytest.mark.parametrize("OUT", cases.OUTS)
def test_grouped_out_of_range_actions_write_a_zero_row_and_nothing_else(env, OUT):
    B, K = 65, 4
    ids = pcases.ids(B, K, "random", seed=3, nobody=0.2)
    rows = [int(np.flatnonzero(ids == m)[1]) for m in (0, 2, 3)]                    # rows of three different members ...
    stray = int(np.flatnonzero(ids >= K)[0])                                        # ... and one of nobody
    c = cases.td_random(B, OUT, "max_mean", True)
    c["action"][rows] = [-1, OUT, 2 ** 40]
    c["action"][stray] = OUT
    lrn = _td_learner(env, OUT, ids, "small", K)
    assert lrn.K == K
    want, E = pmodel.td_head(c, ids, K)
    got = _td_grouped(env, lrn, c)                                                  # (the sentinels around the four outputs are checked there)
    assert not got["gq"][rows].any() and (got["priorities"][rows] == F32(1e-5)).all()
    assert not got["gq"][stray].any() and got["priorities"][stray] == 0.0 and got["estimated"][stray] == 0.0
    for k in KEYS:
        ok, ratio = cases.within(got[k], want[k], E[k])
        assert ok, (k, ratio)
    valid = (ids < K) & (c["action"] >= 0) & (c["action"] < OUT)
    assert valid.sum() == (ids < K).sum() - 3 and (got["gq"] != 0).sum() == valid.sum() and not got["gq"][~valid].any()


# ---------------------------------------------------------------------- 2. the grouped backward past one sweep of the capped grid
def _backward(env, kind, hidden, final_relu, team, x, gq, ids, clamp=None):
    """the grouped backward of `team` on the lists of `ids`: -> every member's gradients as numpy"""
    lrn, _ = _learner(env, kind, team, final_relu, clamp=clamp)
    xd, _ = _lists(env, lrn, x, ids)
    lrn.backward(xd, _dev(env, gq))
    return [_np(g) for g in lrn.grads]


def _exact_backward(env, case, K, ids):
    kind, hidden, fr = case
    team = pcases.exact_team(kind, hidden, K)
    x, gq = gcases.inputs(kind, hidden, "integer", len(ids))
    want, _ = pmodel.backward(x, team, fr, gq, ids, exact=True)
    got = _backward(env, kind, hidden, fr, team, x, gq, ids)
    for m in range(K):
        for i, (g, w) in enumerate(zip(got[m], want[m])):
            assert gcases.same_values(g, w), (m, i, int((g != w).sum()), ecases.counts_of(ids, K)[m])
    return got


@pytest.mark.parametrize("case", ecases.BACKWARD_A, ids=[ecases.backward_id(c) for c in ecases.BACKWARD_A])
def test_grouped_backward_exact_tier_when_every_share_is_below_its_need(env, case):
    """K = 3 on the 65 555 rows of the TD head: with X = 512 the members' shares are 250, 129 and 128 workgroups against needs of 500, 257 and 256, so
    the stride loop of every wavefront but 7 runs twice: the row fetch through ds_bpermute on a second pass, 507 packed partials, the reduction's
    unrolled loop over hundreds of them.  Bit-equal to the model's exact mode."""
    ids = ecases.ids_a()
    counts = ecases.counts_of(ids, ecases.K_A)
    shares, needs = ecases.shares(counts, len(ids), _cus(env)), ecases.needs(counts)
    print("CUs %d: shares %s of needs %s" % (_cus(env), shares, needs))
    assert all(s < n for s, n in zip(shares, needs))
    got = _exact_backward(env, case, ecases.K_A, ids)
    assert all(max(np.abs(g).max() for g in gs) > 100 for gs in got)


@pytest.mark.parametrize("case", ecases.BACKWARD_B, ids=[ecases.backward_id(c) for c in ecases.BACKWARD_B])
def test_grouped_backward_exact_tier_with_the_partials_packed_at_their_maximum(env, case):
    """K = 16 with counts (one single row, one of exactly 64) whose shares sum to X + K - 1 = 527 at X = 512: the last member's partials end in the
    workspace's last slots, and a dropped or misplaced partial is a wrong integer.  The larger counts are no multiples of 16: the tail mask on a later
    pass.  A device with fewer than 256 CUs has a smaller sum (printed); the gradients must be bit-equal all the same."""
    ids = ecases.ids_b()
    counts = ecases.counts_of(ids, ecases.K_B)
    shares = ecases.shares(counts, len(ids), _cus(env))
    print("CUs %d: the shares %s sum to %d (X + K - 1 = %d)" % (_cus(env), shares, sum(shares), ecases.grad_grid(len(ids), _cus(env)) + ecases.K_B - 1))
    if _cus(env) >= 256:
        assert sum(shares) == 527
    got = _exact_backward(env, case, ecases.K_B, ids)
    assert sum(any(g.any() for g in gs) for gs in got) >= 14


_RANDOM = {}


def _random_case(env, kind):
    """the random tier at 65 555 rows, K = 3 (the gathered family, random_team, clamp 1): the device's gradients on all rows and on the rows that are
    left when nobody's are deleted, and the model's values and bounds"""
    if kind not in _RANDOM:
        hidden, K = pcases.HIDDEN[kind][0], ecases.K_A
        ids = ecases.ids_a()
        team = pcases.random_team(kind, hidden, K, "gathered")
        x, gq = ecases.gathered_inputs(kind, hidden, len(ids))
        fr = pcases.final_relu(kind)
        keep = np.flatnonzero(ids < K)
        full = _backward(env, kind, hidden, fr, team, x, gq, ids, clamp=1.0)
        kept = _backward(env, kind, hidden, fr, team, x[keep], gq[keep], ids[keep], clamp=1.0)
        want, E = pmodel.backward(x, team, fr, gq, ids, clamp=1.0)
        _RANDOM[kind] = (ids, keep, full, kept, want, E)
    return _RANDOM[kind]


@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_grouped_backward_random_tier_past_one_sweep_stays_within_the_counted_bound(env, kind):
    ids, keep, full, kept, want, E = _random_case(env, kind)
    for m in range(ecases.K_A):
        for i, (g, w, e) in enumerate(zip(full[m], want[m], E[m])):
            ok, ratio = gcases.within_bound(g, w, e)
            _record("backward " + kind, ratio)
            assert ok, (m, i, ratio)
    assert all(any(g.any() for g in gs) for gs in full)
    print("worst ratio to the bound so far:", WORST)


@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_rows_of_nobody_do_not_count_past_one_sweep(env, kind):
    """the same ids with the 771 rows of nobody deleted: bit-equal gradients when every member keeps its share of the grid, else (another order of the
    sums) both within the counted bound -- the rule of test_gpu_pop_learner.test_rows_of_nobody_change_no_members_result"""
    ids, keep, full, kept, want, E = _random_case(env, kind)
    K, cus = ecases.K_A, _cus(env)
    counts = ecases.counts_of(ids, K)
    a, b = ecases.shares(counts, len(ids), cus), ecases.shares(counts, len(keep), cus)
    print(kind, "shares", a, b, "bit-equal" if a == b else "within the bound")
    if a == b:
        assert all(_bits(u, v) for m in range(K) for u, v in zip(full[m], kept[m]))
    else:
        for m in range(K):
            for u, v, w, e in zip(full[m], kept[m], want[m], E[m]):
                assert gcases.within_bound(u, w, e)[0] and gcases.within_bound(v, w, e)[0], m
                _record("backward without nobody " + kind, gcases.within_bound(v, w, e)[1])
    print("worst ratio to the bound so far:", WORST)


# ---------------------------------------------------------------------- 3. grouped Adam as a stage
class AdamTeam(object):
    """K members' parameters, moments and control blocks on the device, every tensor guarded; the learner's m, v and ctl ARE these tensors"""

    def __init__(self, env, kind, hidden, ctls, m=None, v=None, fresh_state=False):
        self.env, self.K = env, len(ctls)
        self.params = [cases.adam_case(kind, hidden, seed=mb)[0] for mb in range(self.K)]
        self.lrn, _ = _learner(env, kind, self.params, pcases.final_relu(kind), lr=1e-3, fresh_state=fresh_state)
        zeros = [[np.zeros_like(a) for a in ps] for ps in self.params]
        m, v = zeros if m is None else m, zeros if v is None else v
        self.p = [[Guarded(env, a.shape, a) for a in ps] for ps in self.params]
        self.m = [[Guarded(env, a.shape, a) for a in ps] for ps in m]
        self.v = [[Guarded(env, a.shape, a) for a in ps] for ps in v]
        self.ctl = ecases.GuardedCtl(env, ctls)
        self.lrn.m, self.lrn.v, self.lrn.ctl = [[g.t for g in gs] for gs in self.m], [[g.t for g in gs] for gs in self.v], self.ctl.t

    def host(self):
        """per member (params, m, v, ctl); every sentinel is checked"""
        ctls = self.ctl.ctls()
        return [([g.numpy() for g in self.p[mb]], [g.numpy() for g in self.m[mb]], [g.numpy() for g in self.v[mb]], ctls[mb]) for mb in range(self.K)]

    def step(self, grads, counts, clamp=0.0):
        """one evg_adam_step_grouped; the gradients are guarded too and must come back as they went in"""
        gd = [[Guarded(self.env, g.shape, g) for g in gs] for gs in grads]
        cd = _dev(self.env, np.asarray(counts, np.int32))
        self.lrn.adam_step([[g.t for g in gs] for gs in self.p], [[g.t for g in gs] for gs in gd], clamp, cd)
        assert all(_bits(g.numpy(), a) for gs, hs in zip(gd, grads) for g, a in zip(gs, hs))


def _check_member(before, after, grads, count, clamp=0.0, fresh=False, bits=True, what=""):
    """one member's state after a launch against the models applied to its state before: untouched when it had no rows, else within learner_model.adam's
    bounds and (bits) bit-equal to learner_model.adam32.  -> the worst ratio"""
    if count == 0:
        assert all(_bits(a, b) for k in range(3) for a, b in zip(after[k], before[k])) and after[3] == before[3], what
        return 0.0
    (wp, wm, wv, wctl), (Ep, Em, Ev) = model.adam(before[0], grads, before[1], before[2], before[3], clamp=clamp, fresh=fresh, **KW)
    assert after[3] == wctl, (what, after[3], wctl)
    worst = 0.0
    for got, want, E in zip(after[0] + after[1] + after[2], wp + wm + wv, Ep + Em + Ev):
        ok, ratio = cases.within(got, want, E)
        worst = max(worst, ratio)
        assert ok and np.isfinite(got).all(), (what, ratio)
    if bits:
        p32, m32, v32, c32 = model.adam32(before[0], grads, before[1], before[2], before[3], clamp=clamp, fresh=fresh, **KW)
        assert after[3] == c32 and all(cases.same_bits(a, b) for a, b in zip(after[0] + after[1] + after[2], p32 + m32 + v32)), what
    _record("adam grouped", worst)
    return worst


def _grads(kind, hidden, K, step, scales=None):
    return [cases.adam_case(kind, hidden, seed=mb, grad_scale=1.0 if scales is None else scales[mb])[1](step) for mb in range(K)]


@pytest.mark.parametrize("kind,hidden", ecases.ADAM_NETS, ids=[k for k, _ in ecases.ADAM_NETS])
def test_grouped_adam_reads_each_members_own_control_block(env, kind, hidden):
    """one launch over members at step 0, step 1 000 (used moments), step 1 and one without rows; five consecutive launches with changing counts, so
    that the members' step numbers diverge.  A workgroup that read another member's block would take another step size."""
    K = ecases.K_ADAM
    ctls = ecases.adam_start_ctls(KW["betas"])
    r = np.random.default_rng(3)
    shapes = cases.adam_shapes(kind, hidden)
    m0 = [[(r.standard_normal(s) * 0.1).astype(F32) if mb in (1, 3) else np.zeros(s, F32) for s in shapes] for mb in range(K)]
    v0 = [[(r.random(s) * 0.01).astype(F32) if mb in (1, 3) else np.zeros(s, F32) for s in shapes] for mb in range(K)]
    team = AdamTeam(env, kind, hidden, ctls, m0, v0)
    steps = [c[0] for c in ctls]
    for s, counts in enumerate(ecases.ADAM_STEP_COUNTS):
        grads = _grads(kind, hidden, K, s)
        before = team.host()
        team.step(grads, counts)
        after = team.host()
        for mb in range(K):
            _check_member(before[mb], after[mb], grads[mb], counts[mb], what="step %d member %d" % (s, mb))
        steps = [n + (c > 0) for n, c in zip(steps, counts)]
        assert [a[3][0] for a in after] == steps
    assert steps == [5, 1003, 5, 31]
    print("worst ratio to the bound so far:", WORST)


@pytest.mark.parametrize("kind,hidden", ecases.ADAM_NETS, ids=[k for k, _ in ecases.ADAM_NETS])
def test_grouped_adam_zero_and_extreme_gradients(env, kind, hidden):
    K = ecases.K_ADAM
    # zero gradients on zero state: the parameters keep their bits, the moments stay zero, the step is counted
    team = AdamTeam(env, kind, hidden, [model.new_ctl()] * K)
    team.step([[np.zeros_like(a) for a in ps] for ps in team.params], [1, 2, 3, 4])
    after = team.host()
    for mb in range(K):
        assert all(_bits(a, b) for a, b in zip(after[mb][0], team.params[mb])) and after[mb][3][0] == 1
        assert not any(a.any() for a in after[mb][1] + after[mb][2])
    # gradients of 1e-20 and of 1e+15, another scale per member in one launch, two steps
    scales = (1e-20, 1e15, 1.0, 1e15)
    team = AdamTeam(env, kind, hidden, [model.new_ctl()] * K)
    for s, counts in enumerate(((3, 3, 3, 0), (1, 1, 1, 1))):
        grads = _grads(kind, hidden, K, s, scales)
        before = team.host()
        team.step(grads, counts)
        after = team.host()
        for mb in range(K):
            _check_member(before[mb], after[mb], grads[mb], counts[mb], bits=False, what="gradients of %g, step %d" % (scales[mb], s))
    assert [a[3][0] for a in after] == [2, 2, 2, 1]


@pytest.mark.parametrize("kind,hidden", ecases.ADAM_NETS, ids=[k for k, _ in ecases.ADAM_NETS])
def test_grouped_adam_clamps_the_gradients_as_it_reads_them(env, kind, hidden):
    K = ecases.K_ADAM
    grads = _grads(kind, hidden, K, 0, (3.0,) * K)
    assert all(any((np.abs(g) > 1).any() for g in gs) for gs in grads)
    results = []
    for clamp in (0.0, 1.0):
        team = AdamTeam(env, kind, hidden, [model.new_ctl()] * K)
        before = team.host()
        team.step(grads, [7, 1, 0, 2], clamp=clamp)
        after = team.host()
        for mb, count in enumerate([7, 1, 0, 2]):
            _check_member(before[mb], after[mb], grads[mb], count, clamp=clamp, what="clamp %g member %d" % (clamp, mb))
        results.append(after)
    for mb in (0, 1, 3):
        assert not np.array_equal(results[0][mb][2][0], results[1][mb][2][0])
        assert all((np.abs(m) <= (1 - KW["betas"][0]) * 1.0000001).all() for m in results[1][mb][1])
        assert any((np.abs(m) > (1 - KW["betas"][0]) * 1.0000001).any() for m in results[0][mb][1])


@pytest.mark.parametrize("kind,hidden", ecases.ADAM_NETS, ids=[k for k, _ in ecases.ADAM_NETS])
def test_grouped_adam_fresh_state_ignores_the_stored_state_of_members_with_rows_only(env, kind, hidden):
    K = ecases.K_ADAM
    r = np.random.default_rng(4)
    shapes = cases.adam_shapes(kind, hidden)
    junk = [[r.standard_normal(s).astype(F32) for s in shapes] for _ in range(K)]
    team = AdamTeam(env, kind, hidden, [(77, 0.5, 0.25)] * K, junk, [[np.abs(j) for j in js] for js in junk], fresh_state=True)
    counts = [4, 2, 0, 9]
    for s in range(2):
        grads = _grads(kind, hidden, K, 0)
        before = team.host()
        team.step(grads, counts)
        after = team.host()
        for mb in range(K):
            _check_member(before[mb], after[mb], grads[mb], counts[mb], fresh=True, what="fresh step %d member %d" % (s, mb))
            if counts[mb]:
                assert after[mb][3] == (1, KW["betas"][0], KW["betas"][1])
    # member 2 had no rows: its junk and its control block are as they were
    assert after[2][3] == (77, 0.5, 0.25) and all(_bits(a, b) for a, b in zip(after[2][1], junk[2]))
    print("worst ratio to the bound so far:", WORST)
