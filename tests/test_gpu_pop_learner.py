"""GPU tests of the population learner (everglades_amd.PopulationLearner, include/evg_pop_learn.h): every grouped stage against
tests/pop_learner_model.py on the operands the device actually fed it -- bit-equal on the exact tier, within the counted bounds with B := c_m on the
random tier -- routing edges, separation of the members, K = 1 against DqnLearner, determinism, graph capture, and the two self-royale examples.

An end-to-end tolerance on the parameters would be vacuous after Adam's division (DESIGN, "Learner step"), so Adam too is checked on the gradients
the device computed."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import learner_cases as cases
import learner_model as model
import pop_learner_cases as pcases
import pop_learner_model as pmodel
import qnet_grad_cases as gcases

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
F32 = np.float32
KW = dict(lr=float(F32(1e-3)), betas=(float(F32(0.9)), float(F32(0.999))), eps=float(F32(1e-8)))
WORST = {}


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


def _learner(env, kind, team, targets=None, **kw):
    """-> (learner, the policies' device tensors, the targets'): networks as tuples of tensors"""
    pol = [tuple(_dev(env, p)) for p in team]
    tgt = [tuple(_dev(env, p)) for p in (team if targets is None else targets)]
    make = env.smart_population_learner if kind == "smart" else env.minimized_population_learner
    return make(pol, tgt, final_relu=pcases.final_relu(kind), **kw), pol, tgt


def _lists(env, lrn, x, ids):
    """the policy forward that leaves the lists: -> (x, ids on the device, the buffers)"""
    xd, idd = _dev(env, x), _dev(env, ids)
    b = lrn._buffers(len(ids))
    lrn.policy_forward(xd, idd, b["q_pred"])
    K = lrn.K
    assert lrn.counts.cpu().numpy().tolist() == [int((ids == m).sum()) for m in range(K)]
    return xd, idd, b


def _td(env, lrn, c, b):
    d = {k: _dev(env, c[k]) for k in ("q_pred", "action", "q_next", "q_select", "reward", "not_done", "weights")}
    for k in ("gq", "priorities", "estimated"):
        b[k].fill_(-7.5)
    lrn.loss.fill_(-7.5)
    lrn.td_head(d["q_pred"], d["action"], d["q_next"], d["q_select"], d["reward"], d["not_done"], d["weights"], b["gq"], lrn.loss, b["priorities"],
                b["estimated"], mode=c["mode"], scale=float(c["scale"]))
    return {"gq": b["gq"].cpu().numpy(), "priorities": b["priorities"].cpu().numpy(), "estimated": b["estimated"].cpu().numpy(),
            "loss": lrn.loss.cpu().numpy().copy()}


def _hidden(kind, B):
    return pcases.HIDDEN[kind][1 if B == 257 else 0]       # the padded pair at one B, the defaults elsewhere


def _shares(ids, K, cus):
    """the workgroups of the grouped backward that each member's rows use (include/evg_pop_learn.h)"""
    B = len(ids)
    X = min(-(-(-(-B // 16)) // 4), min(2 * cus, 512))
    return [min(-(-int((ids == m).sum()) // 64), -(-X * int((ids == m).sum()) // B)) for m in range(K)]


# ---------------------------------------------------------------------- 1. the stages on given operands
@pytest.mark.parametrize("kind", ["smart", "mini"])
@pytest.mark.parametrize("B,K", pcases.SHAPES)
def test_exact_tier_td_head_and_backward_are_bit_equal_to_the_model(env, kind, B, K):
    hidden = _hidden(kind, B)
    ids = pcases.ids(B, K, nobody=0.1 if B > 16 else 0.0)
    team = pcases.exact_team(kind, hidden, K)
    lrn, _, _ = _learner(env, "smart" if kind == "smart" else "minimized", team, clamp=None)
    x, gq = gcases.inputs(kind, hidden, "integer", B)
    xd, idd, b = _lists(env, lrn, x, ids)
    for mode, weighted in (("max_mean", True), ("double_mean", False), ("max_max", False)):
        c = cases.td_exact(B, gcases.OUT[kind], mode, weighted)
        got = _td(env, lrn, c, b)
        want, _ = pmodel.td_head(c, ids, K, exact=True)
        for k in ("gq", "priorities", "estimated", "loss"):
            assert cases.same_bits(got[k], want[k]), (mode, k)
    lrn.backward(xd, _dev(env, gq))
    want, _ = pmodel.backward(x, team, pcases.final_relu(kind), gq, ids, exact=True)
    for m in range(K):
        for i, (g, w) in enumerate(zip(_np(lrn.grads[m]), want[m])):
            assert gcases.same_values(g, w), (m, i)
    assert any(g.any() for m in range(K) for g in _np(lrn.grads[m]))


@pytest.mark.parametrize("family", ["dense", "gathered"])
@pytest.mark.parametrize("kind", ["smart", "mini"])
@pytest.mark.parametrize("B,K", pcases.SHAPES)
def test_random_tier_stays_within_the_counted_bound_for_each_members_count(env, kind, B, K, family):
    hidden = _hidden(kind, B)
    how = ("random", "descending", "interleaved", "one")[(B + K) % 4]
    ids = pcases.ids(B, K, how, nobody=0.15 if B > 16 else 0.0)
    team = pcases.random_team(kind, hidden, K, family)
    lrn, _, _ = _learner(env, "smart" if kind == "smart" else "minimized", team, clamp=1.0)
    x, gq = gcases.inputs(kind, hidden, family, B)
    xd, idd, b = _lists(env, lrn, x, ids)
    mode = model.MODES[(B + K) % 3]
    c = cases.td_random(B, gcases.OUT[kind], mode, family == "dense")
    got = _td(env, lrn, c, b)
    want, E = pmodel.td_head(c, ids, K)
    for k in ("gq", "priorities", "estimated", "loss"):
        ok, ratio = cases.within(got[k], want[k], E[k])
        WORST["td " + k] = max(WORST.get("td " + k, 0.0), ratio)
        assert ok, (k, ratio)
    w32 = pmodel.td_head32(c, ids, K)                        # the order of every sum is the model's: bit for bit
    for k in ("gq", "priorities", "estimated", "loss"):
        assert cases.same_bits(got[k], w32[k]), k
    lrn.backward(xd, _dev(env, gq))
    gwant, gE = pmodel.backward(x, team, pcases.final_relu(kind), gq, ids, clamp=1.0)
    for m in range(K):
        for i, (g, w, e) in enumerate(zip(_np(lrn.grads[m]), gwant[m], gE[m])):
            ok, ratio = gcases.within_bound(g, w, e)
            WORST["backward " + kind] = max(WORST.get("backward " + kind, 0.0), ratio)
            assert ok, (m, i, ratio, int((ids == m).sum()))
    print("worst ratio to the bound so far:", WORST)


# ---------------------------------------------------------------------- 2. a whole step, every stage on the device's own operands
def _batch(kind, B, seed, family="gathered"):
    r = np.random.default_rng([seed, B])
    x, _ = gcases.inputs(kind, pcases.HIDDEN[kind][0], family, B)
    nxt = np.zeros((B, 12, 59), F32)
    nxt[:, :, :47] = r.random((B, 12, 47))
    nxt[:, np.arange(12), 47 + np.arange(12)] = 1.0
    return (x, r.integers(0, gcases.OUT[kind], B).astype(np.int64), nxt, r.standard_normal(B).astype(F32), r.random(B) < 0.8)


def _check_step(env, evg, lrn, pol, tgt, kind, batch, ids, weights, mode, steps_before, clamp=1.0, precision="fp32"):
    """one step_on; every stage against its model on what the device fed it (q_next and q_select: bit-equal to each member's own evaluator at
    `precision`).  -> the members' counts"""
    K = lrn.K
    x, action, nxt, reward, not_done = batch
    fr = pcases.final_relu(kind)
    dbatch = tuple(_dev(env, a) for a in batch)
    idd, wd = _dev(env, ids), _dev(env, weights)
    params = [_np(p) for p in pol]
    m0, v0 = [_np(t) for t in lrn.m], [_np(t) for t in lrn.v]
    ctl0 = lrn.ctl.cpu().numpy().copy()
    single = env.smart_qnet if kind == "smart" else env.minimized_qnet
    want_pred, want_next = np.zeros((len(ids), lrn.OUT), F32), np.zeros((len(ids), 12, lrn.OUT), F32)
    want_sel = np.zeros_like(want_next)
    for m in range(K):
        R = ids == m
        want_pred[R] = single(pol[m], final_relu=fr).expanded(dbatch[0]).cpu().numpy()[R]
        want_next[R] = single(tgt[m], final_relu=fr, precision=precision).expanded(dbatch[2]).cpu().numpy()[R]
        want_sel[R] = single(pol[m], final_relu=fr, precision=precision).expanded(dbatch[2]).cpu().numpy()[R]
    ret = lrn.step_on(dbatch, idd, weights=wd)
    loss = ret[0] if weights is not None else ret
    assert tuple(loss.shape) == (K,) and loss.data_ptr() == lrn.loss.data_ptr()
    if weights is not None:
        assert ret[1].data_ptr() == lrn.priorities.data_ptr()
    counts = [int((ids == m).sum()) for m in range(K)]
    assert lrn.counts.cpu().numpy().tolist() == counts
    q_pred, q_next = lrn.q_pred.cpu().numpy(), lrn.q_next.cpu().numpy()
    assert _bits(q_pred, want_pred) and _bits(q_next, want_next)
    q_sel = None
    if mode == "double_mean":
        q_sel = lrn.q_select.cpu().numpy()
        assert _bits(q_sel, want_sel)                        # the member's own policy, as it was before the step, selects
    c = dict(q_pred=q_pred, action=action, q_next=q_next, q_select=q_sel, reward=reward, not_done=not_done, weights=weights, scale=F32(0.999), mode=mode)
    want, E = pmodel.td_head(c, ids, K)
    gq = lrn.gq.cpu().numpy()
    got = {"gq": gq, "loss": loss.cpu().numpy(), "priorities": lrn.priorities.cpu().numpy(), "estimated": lrn.estimated.cpu().numpy()}
    for k in got:
        ok, ratio = cases.within(got[k], want[k], E[k])
        assert ok, (k, ratio)
    nobody = ids >= K
    assert not gq[nobody].any() and not got["priorities"][nobody].any()
    gwant, gE = pmodel.backward(x, params, fr, gq, ids, clamp=clamp)
    grads = [_np(g) for g in lrn.grads]
    for m in range(K):
        for i, (g, w, e) in enumerate(zip(grads[m], gwant[m], gE[m])):
            ok, ratio = gcases.within_bound(g, w, e)
            assert ok, ("gradient", m, i, ratio)
    ctls = [model.ctl_from_words(ctl0[m]) for m in range(K)]
    res = pmodel.adam(params, grads, m0, v0, ctls, counts, **KW)
    after_p, after_m, after_v = [_np(p) for p in pol], [_np(t) for t in lrn.m], [_np(t) for t in lrn.v]
    ctl1 = lrn.ctl.cpu().numpy()
    for m in range(K):
        (wp, wm, wv, wctl), (Ep, Em, Ev) = res[m]
        if counts[m] == 0:                                   # no Adam step: everything bit-identical, loss 0, zero gradients
            assert all(_bits(a, b) for a, b in zip(after_p[m] + after_m[m] + after_v[m], params[m] + m0[m] + v0[m]))
            assert np.array_equal(ctl1[m], ctl0[m]) and got["loss"][m] == 0.0 and not any(g.any() for g in grads[m])
            continue
        for i, (a, w, e) in enumerate(zip(after_p[m] + after_m[m] + after_v[m], wp + wm + wv, Ep + Em + Ev)):
            ok, ratio = cases.within(a, w, e)
            WORST["adam"] = max(WORST.get("adam", 0.0), ratio)
            assert ok, ("parameter / m / v", m, i, ratio)
        assert model.ctl_from_words(ctl1[m]) == wctl and wctl[0] == steps_before[m] + 1
        assert any(not np.array_equal(a, b) for a, b in zip(after_p[m], params[m]))
    return counts


@pytest.mark.parametrize("mode,weighted", [("max_mean", False), ("max_max", True), ("double_mean", True)], ids=["max_mean", "max_max-weighted", "double_mean-weighted"])
@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_every_stage_of_a_step_agrees_with_its_model_on_the_devices_own_operands(evg, env, kind, mode, weighted):
    """three steps at B = 257, K = 4: random ids with rows of nobody; all rows to member 0 (the others keep every bit); member 3 with exactly one row.
    Each control block advances once per step in which its member had rows."""
    B, K = 257, 4
    hidden = pcases.HIDDEN[kind][0]
    team, targets = pcases.random_team(kind, hidden, K, "gathered"), pcases.random_team(kind, hidden, K, "gathered", seed=9)
    lrn, pol, tgt = _learner(env, "smart" if kind == "smart" else "minimized", team, targets, lr=1e-3, gamma=0.999, n_step=1, mode=mode, clamp=1.0)
    steps = [0] * K
    for call, (how, nobody) in enumerate((("random", 0.2), ("first", 0.0), ("one", 0.1))):
        ids = pcases.ids(B, K, how, seed=call, nobody=nobody)
        w = (0.1 + 0.9 * np.random.default_rng(call).random(B)).astype(F32) if weighted else None
        counts = _check_step(env, evg, lrn, pol, tgt, kind, _batch(kind, B, call), ids, w, mode, steps)
        steps = [s + (c > 0) for s, c in zip(steps, counts)]
        if how == "one":
            assert counts[K - 1] == 1
    assert steps == [3, 2, 2, 2] and lrn.ctl[:, 0].cpu().tolist() == steps
    assert lrn.policy_pop.status() == evg._lib.POP_S_BAD_MEMBER            # the sticky bit of the private population: expected, no error of the learner
    sd = lrn.state_dict()
    assert sd["step"] == steps
    lrn.sync_target([1])
    assert all(_bits(a, b) for a, b in zip(_np(tgt[1]), _np(pol[1]))) and not all(_bits(a, b) for a, b in zip(_np(tgt[0]), _np(pol[0])))
    lrn.ctl.zero_()
    lrn.load_state_dict(sd)
    assert lrn.ctl[:, 0].cpu().tolist() == steps
    print("worst ratio to the bound so far:", WORST)


@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_bf16_targets_run_a_whole_step_and_each_row_is_its_own_members_bf16_forward(evg, env, kind):
    """target_precision="bf16" at B = 257, K = 4, double_mean with weights: q_next and q_select are bit-equal to the members' own bf16 evaluators on
    their rows (zeros for the rows of nobody), every later stage agrees with its model on those operands; a second step with member 2 absent leaves
    it alone.  The fp32 learner on the same batch gives other q_next bits: the setting is not ignored."""
    B, K = 257, 4
    hidden = pcases.HIDDEN[kind][0]
    name = "smart" if kind == "smart" else "minimized"
    team, targets = pcases.random_team(kind, hidden, K, "gathered"), pcases.random_team(kind, hidden, K, "gathered", seed=9)
    lrn, pol, tgt = _learner(env, name, team, targets, lr=1e-3, gamma=0.999, n_step=1, mode="double_mean", clamp=1.0, target_precision="bf16")
    assert lrn.target_precision == "bf16" and lrn.target_pop is None and lrn.select_pop is None and len(lrn.target_nets) == len(lrn.select_nets) == K
    batch = _batch(kind, B, 3)
    w = (0.1 + 0.9 * np.random.default_rng(3).random(B)).astype(F32)
    ids = pcases.ids(B, K, "random", seed=3, nobody=0.2)
    counts = _check_step(env, evg, lrn, pol, tgt, kind, batch, ids, w, "double_mean", [0] * K, precision="bf16")
    assert all(counts) and (ids >= K).any()
    q_next16 = lrn.q_next.cpu().numpy().copy()
    ids2 = ids.copy()
    ids2[ids2 == 2] = pcases.NOBODY
    counts = _check_step(env, evg, lrn, pol, tgt, kind, batch, ids2, w, "double_mean", [1] * K, precision="bf16")
    assert counts[2] == 0 and lrn.ctl[:, 0].cpu().tolist() == [2, 2, 1, 2]
    ref, _, _ = _learner(env, name, [_np(p) for p in pol], [_np(t) for t in tgt], mode="double_mean")
    ref.step_on(tuple(_dev(env, a) for a in batch), _dev(env, ids), weights=_dev(env, w))
    assert not _bits(ref.q_next.cpu().numpy(), q_next16)
    # the bf16 step is launches alone: it can be captured, and the replay writes the same targets (the target networks have not moved)
    import torch
    dbatch, idd, wd = tuple(_dev(env, a) for a in batch), _dev(env, ids), _dev(env, w)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lrn.step_on(dbatch, idd, weights=wd)
    lrn.q_next.fill_(-1.0)
    g.replay()
    assert _bits(lrn.q_next.cpu().numpy(), q_next16) and lrn.ctl[:, 0].cpu().tolist() == [3, 3, 2, 3]
    # the merge alone: a member's rows are taken, the rows of nobody zeroed, every other row left as it was
    src = torch.full((B, 12, lrn.OUT), 2.5, device=env.device)
    dst = torch.full((B, 12, lrn.OUT), -7.5, device=env.device)
    ids12 = lrn.expand_ids(_dev(env, ids), torch.zeros((B, 12), dtype=torch.uint8, device=env.device))
    got = lrn.take_rows(src, ids12, 1, dst).cpu().numpy()
    assert (got[ids == 1] == 2.5).all() and (got[ids >= K] == 0.0).all() and (got[(ids != 1) & (ids < K)] == -7.5).all()


def test_final_relu_off_and_sixteen_members_at_a_padded_size(evg, env):
    """the Smart_State family without the final ReLU is the default above; here the Minimized one without it and Smart_State with it, K = 16"""
    for kind, fr in (("mini", False), ("smart", True)):
        hidden = pcases.HIDDEN[kind][1]
        B, K = 259, 16
        team = pcases.random_team(kind, hidden, K, "dense")
        pol = [tuple(_dev(env, p)) for p in team]
        make = env.smart_population_learner if kind == "smart" else env.minimized_population_learner
        lrn = make(pol, pol, final_relu=fr)
        x, gq = gcases.inputs(kind, hidden, "dense", B)
        ids = pcases.ids(B, K, "interleaved", nobody=0.1)
        xd, idd, b = _lists(env, lrn, x, ids)
        lrn.backward(xd, _dev(env, gq))
        gwant, gE = pmodel.backward(x, team, fr, gq, ids, clamp=1.0)
        for m in range(K):
            assert all(gcases.within_bound(g, w, e)[0] for g, w, e in zip(_np(lrn.grads[m]), gwant[m], gE[m])), (kind, m)


# ---------------------------------------------------------------------- 3. routing: rows of nobody are as good as deleted
@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_rows_of_nobody_change_no_members_result(evg, env, kind):
    import torch
    cus = torch.cuda.get_device_properties(env.device).multi_processor_count
    hidden = pcases.HIDDEN[kind][0]
    K = 3
    team = pcases.random_team(kind, hidden, K, "gathered")
    for B in (100, 1100):
        ids = pcases.ids(B, K, "random", seed=B, nobody=0.25)
        keep = np.flatnonzero(ids < K)
        batch = _batch(kind, B, 3)
        results = []
        for rows, who in ((np.arange(B), ids), (keep, ids[keep])):
            lrn, pol, _ = _learner(env, "smart" if kind == "smart" else "minimized", team, lr=1e-3)
            sub = tuple(_dev(env, a[rows]) for a in batch)
            loss = lrn.step_on(sub, _dev(env, who)).cpu().numpy().copy()
            results.append((loss, lrn.gq.cpu().numpy(), lrn.priorities.cpu().numpy(), [_np(g) for g in lrn.grads], [_np(p) for p in pol]))
        (l0, gq0, pr0, g0, p0), (l1, gq1, pr1, g1, p1) = results
        assert _bits(l0, l1) and _bits(gq0[keep], gq1) and _bits(pr0[keep], pr1)        # the TD head's order is a function of the lists alone
        assert not gq0[ids >= K].any() and not pr0[ids >= K].any()
        same = _shares(ids, K, cus) == _shares(ids[keep], K, cus)
        if same:                                             # the same rows in the same order in the same workgroups: bit-equal
            assert all(_bits(a, b) for m in range(K) for a, b in zip(g0[m] + p0[m], g1[m] + p1[m]))
        else:                                                # another share of the grid, another order of the sums: the counted bound applies
            gwant, gE = pmodel.backward(batch[0], [list(t) for t in team], pcases.final_relu(kind), gq0, ids, clamp=1.0)
            assert all(gcases.within_bound(a, w, e)[0] and gcases.within_bound(b, w, e)[0]
                       for m in range(K) for a, b, w, e in zip(g0[m], g1[m], gwant[m], gE[m]))
        print(kind, B, "shares", _shares(ids, K, cus), _shares(ids[keep], K, cus), "bit-equal" if same else "within the bound")


# ---------------------------------------------------------------------- 4. separation of the members
def test_members_read_their_own_weights_and_only_their_own_rows(evg, env):
    kind, K, B = "smart", 2, 128
    hidden = pcases.HIDDEN[kind][0]
    one = pcases.random_team(kind, hidden, 1, "gathered")[0]
    two = pcases.random_team(kind, hidden, 2, "gathered", seed=4)
    x, action, nxt, reward, not_done = _batch(kind, B, 5)
    ids = (np.arange(B) >= B // 2).astype(np.uint8)
    fr = pcases.final_relu(kind)

    def grads_of(team, batch):
        lrn, _, _ = _learner(env, "smart", team, lr=1e-3)
        lrn.step_on(tuple(_dev(env, a) for a in batch), _dev(env, ids))
        return [_np(g) for g in lrn.grads], lrn.gq.cpu().numpy(), lrn.loss.cpu().numpy().copy()

    # identical weights, disjoint rows: each member's gradients are the model's on ITS rows and not on the other's
    g, gq, loss = grads_of([one, one], (x, action, nxt, reward, not_done))
    want, E = pmodel.backward(x, [one, one], fr, gq, ids, clamp=1.0)
    swapped, _ = pmodel.backward(x, [one, one], fr, gq, 1 - ids, clamp=1.0)
    for m in range(2):
        assert all(gcases.within_bound(a, w, e)[0] for a, w, e in zip(g[m], want[m], E[m]))
        assert not all(gcases.within_bound(a, w, e)[0] for a, w, e in zip(g[m], swapped[m], E[m]))
    assert loss[0] != loss[1]
    # identical rows (the second half of the batch is the first), different weights: each member's gradients are its own network's
    dup = tuple(np.concatenate([a[:B // 2], a[:B // 2]]) for a in (x, action, nxt, reward, not_done))
    g, gq, loss = grads_of(two, dup)
    assert not _bits(gq[:B // 2], gq[B // 2:])
    want, E = pmodel.backward(dup[0], two, fr, gq, ids, clamp=1.0)
    other, _ = pmodel.backward(dup[0], two[::-1], fr, gq, ids, clamp=1.0)
    for m in range(2):
        assert all(gcases.within_bound(a, w, e)[0] for a, w, e in zip(g[m], want[m], E[m]))
        assert not all(gcases.within_bound(a, w, e)[0] for a, w, e in zip(g[m], other[m], E[m]))


def test_perturbing_one_row_of_a_member_leaves_every_other_member_bit_identical(evg, env):
    for kind in ("smart", "mini"):
        K, B = 4, 257
        hidden = pcases.HIDDEN[kind][0]
        team = pcases.random_team(kind, hidden, K, "gathered")
        ids = pcases.ids(B, K, "random", seed=2, nobody=0.1)
        batch = _batch(kind, B, 6)
        j = 2
        row = int(np.flatnonzero(ids == j)[3])
        moved = tuple(a.copy() for a in batch)
        moved[0][row, :47] += F32(0.25)
        moved[3][row] += F32(1.0)
        out = []
        for bt in (batch, moved):
            lrn, pol, _ = _learner(env, "smart" if kind == "smart" else "minimized", team, lr=1e-3, mode="double_mean")
            loss = lrn.step_on(tuple(_dev(env, a) for a in bt), _dev(env, ids)).cpu().numpy().copy()
            out.append((loss, lrn.gq.cpu().numpy(), lrn.priorities.cpu().numpy(), [_np(g) for g in lrn.grads], [_np(p) for p in pol],
                        [_np(t) for t in lrn.m], lrn.ctl.cpu().numpy()))
        a, b = out
        others = ids != j
        assert _bits(a[1][others], b[1][others]) and _bits(a[2][others], b[2][others]) and np.array_equal(a[6], b[6])
        for m in range(K):
            same = _bits(a[0][m], b[0][m]) and all(_bits(u, v) for k in (3, 4, 5) for u, v in zip(a[k][m], b[k][m]))
            assert same == (m != j), (kind, m)


# ---------------------------------------------------------------------- 5. K = 1 is DqnLearner
@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_one_member_agrees_with_the_plain_learner_stage_by_stage(evg, env, kind):
    B = 259
    hidden = pcases.HIDDEN[kind][0]
    net = pcases.random_team(kind, hidden, 1, "gathered")[0]
    fr = pcases.final_relu(kind)
    ids = np.zeros(B, np.uint8)
    batch = _batch(kind, B, 7)
    x, action, nxt, reward, not_done = batch
    pop, ppol, _ = _learner(env, "smart" if kind == "smart" else "minimized", [net], lr=1e-3, mode="double_mean")
    pol, tgt = tuple(_dev(env, net)), tuple(_dev(env, net))
    plain = (env.smart_learner if kind == "smart" else env.minimized_learner)(pol, tgt, None, lr=1e-3, mode="double_mean", final_relu=fr)
    dbatch = tuple(_dev(env, a) for a in batch)
    lp = pop.step_on(dbatch, _dev(env, ids)).cpu().numpy().copy()
    ld = plain.step_on(dbatch).cpu().numpy().copy()
    # forwards and the TD head: the same operands in the same order, bit for bit
    assert _bits(pop.q_pred.cpu().numpy(), plain.q_pred.cpu().numpy()) and _bits(pop.q_next.cpu().numpy(), plain.q_next.cpu().numpy())
    assert _bits(pop.q_select.cpu().numpy(), plain.q_select.cpu().numpy())
    gq = pop.gq.cpu().numpy()
    assert _bits(gq, plain.gq.cpu().numpy()) and _bits(lp[0], ld) and _bits(pop.priorities.cpu().numpy(), plain.priorities.cpu().numpy())
    # the backward and Adam: both within the model's bounds on the same operands (the grid may differ)
    gwant, gE = pmodel.backward(x, [list(net)], fr, gq, ids, clamp=1.0)
    for got in (_np(pop.grads[0]), _np(plain.grads)):
        assert all(gcases.within_bound(g, w, e)[0] for g, w, e in zip(got, gwant[0], gE[0]))
    z = [np.zeros_like(p) for p in net]
    for grads, after, mm, vv in ((_np(pop.grads[0]), _np(ppol[0]), _np(pop.m[0]), _np(pop.v[0])), (_np(plain.grads), _np(pol), _np(plain.m), _np(plain.v))):
        (wp, wm, wv, wctl), (Ep, Em, Ev) = model.adam(list(net), grads, z, z, model.new_ctl(), **KW)
        assert all(cases.within(a, w, e)[0] for a, w, e in zip(after + mm + vv, wp + wm + wv, Ep + Em + Ev))
    assert np.array_equal(pop.ctl.cpu().numpy()[0], plain.ctl.cpu().numpy())


# ---------------------------------------------------------------------- 6. determinism, capture, the control blocks
def test_two_steps_are_bit_equal_a_captured_step_replays_and_control_blocks_count_their_members_steps(evg, env):
    import torch
    kind, K, B = "smart", 4, 1100
    hidden = pcases.HIDDEN[kind][0]
    team = pcases.random_team(kind, hidden, K, "gathered")
    lrn, pol, tgt = _learner(env, "smart", team, lr=1e-3, mode="double_mean")
    dbatch = tuple(_dev(env, a) for a in _batch(kind, B, 8))
    idd = _dev(env, pcases.ids(B, K, "random", seed=1, nobody=0.1))
    wd = _dev(env, (0.5 + 0.5 * np.random.default_rng(0).random(B)).astype(F32))

    def snapshot():
        return [t.clone() for p in pol for t in p] + [t.clone() for ts in lrn.m + lrn.v for t in ts] + [lrn.ctl.clone()]

    def restore(s):
        for dst, src in zip([t for p in pol for t in p] + [t for ts in lrn.m + lrn.v for t in ts] + [lrn.ctl], s):
            dst.copy_(src)

    def result():
        return _np([lrn.loss, lrn.gq, lrn.priorities] + [g for gs in lrn.grads for g in gs] + snapshot())

    start = snapshot()
    lrn.step_on(dbatch, idd, weights=wd)                    # (also the warm-up: every buffer of this batch size exists from here on)
    first = result()
    restore(start)
    lrn.step_on(dbatch, idd, weights=wd)
    assert all(_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(first, result()))
    restore(start)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lrn.step_on(dbatch, idd, weights=wd)
    restore(start)
    lrn.loss.fill_(3.0)
    g.replay()
    assert all(_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(first, result()))
    # five consecutive steps; member 3 has rows in steps 0 and 3 only, member 1 never
    restore(start)
    lrn.ctl.zero_()
    lrn.ctl.view(torch.float64)[:, 1:3] = 1.0
    had = np.zeros(K, np.int64)
    for s in range(5):
        ids = pcases.ids(B, K, "random", seed=10 + s)
        ids[ids == 1] = pcases.NOBODY
        if s not in (0, 3):
            ids[ids == 3] = 0
        lrn.step_on(dbatch, _dev(env, ids))
        had += np.array([(ids == m).any() for m in range(K)])
        assert lrn.ctl[:, 0].cpu().numpy().tolist() == had.tolist()
    assert had.tolist() == [5, 0, 5, 2]
    words = lrn.ctl.cpu().numpy()
    assert model.ctl_from_words(words[1]) == model.new_ctl()
    assert model.ctl_from_words(words[3]) == (2, float(F32(0.9)) ** 2, float(F32(0.999)) * float(F32(0.999)))


def test_step_on_refuses_what_the_kernels_cannot_see(evg, env):
    import torch
    team = pcases.random_team("smart", (3, 3), 2, "dense")
    lrn, _, _ = _learner(env, "smart", team)
    batch = tuple(_dev(env, a) for a in _batch("smart", 16, 0))
    with pytest.raises(ValueError, match="member must be a contiguous"):
        lrn.step_on(batch, torch.zeros(16, dtype=torch.int64, device=env.device))
    with pytest.raises(ValueError, match="member must be a contiguous"):
        lrn.step_on(batch, torch.zeros(15, dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError, match=r"1\.\.2\^20"):
        lrn.step_on(tuple(t[:0] for t in batch), torch.zeros(0, dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError, match='target_precision must be "fp32" or "bf16"'):
        env.smart_population_learner([tuple(_dev(env, team[0]))], [tuple(_dev(env, team[0]))], final_relu=False, target_precision="fp16")
    lrn.step_on(batch, torch.zeros(16, dtype=torch.uint8, device=env.device))
    assert torch.isfinite(lrn.loss).all()


# ---------------------------------------------------------------------- 7. the examples
@pytest.mark.parametrize("example", ["smart_state_self_royale.py", "minimized_self_royale.py"])
def test_self_royale_examples_run_with_the_device_learner(example):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", example), "256", "12", "64", "--device-learner"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "device learner" in out.stdout and "all finite: True" in out.stdout, out.stdout[-2000:]
