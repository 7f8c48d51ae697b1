"""CPU tests of tests/pop_learner_edge_cases.py, on the host models alone: every precondition that tests/test_gpu_learner_step_edges.py relies on holds
before anything runs on a device -- the chunk counts of the TD head at and past its block cap, the model's exact mode on every operand set at these
sizes, share < need for every member of the grouped backward, the packing of the partials at its maximum, and the Adam stage's starting states."""
import numpy as np
import pytest

import learner_cases as cases
import learner_model as model
import pop_learner_cases as pcases
import pop_learner_edge_cases as ecases
import pop_learner_model as pmodel
import qnet_grad_cases as gcases


def test_constants_are_the_bindings():
    import everglades_amd
    _lib = everglades_amd._lib
    assert ecases.GRAD_MAX_BLOCKS == _lib.QNET_GRAD_MAX_BLOCKS and ecases.BIG_B == gcases.sweep_rows(_lib.QNET_GRAD_MAX_BLOCKS) == 65555
    assert _lib.TD_HEAD_WORKSPACE_BYTES == 4 * ecases.TD_MAX_BLOCKS and ecases.TD_SLOTS == 16 and ecases.TD_ONE_PASS == 16384
    assert _lib.POP_LEARN_MAX_PARTIALS == ecases.GRAD_MAX_BLOCKS + ecases.K_B == 528
    assert ecases.BIG_B <= _lib.TD_HEAD_MAX_BATCH


# ---------------------------------------------------------------------- 1. the TD head past its block cap
def test_plain_batches_sit_at_one_past_and_twice_past_the_block_cap():
    assert ecases.PLAIN_BATCHES == (16384, 16385, 32787)
    assert ecases.td_chunks(16384) == (1024, 1024) and ecases.td_passes(16384) == [0, 1024]
    assert ecases.td_chunks(16385) == (1025, 1024) and ecases.td_passes(16385) == [0, 1023, 1]           # workgroup 0 alone takes a second chunk ...
    assert 16385 - 1024 * 16 == 1                                                                       # ... which holds one live row
    assert ecases.td_chunks(32787) == (2050, 1024) and ecases.td_passes(32787) == [0, 0, 1022, 2]       # two workgroups take a third chunk
    assert 32787 - 2049 * 16 == 3                                                                       # the last of them partial
    assert max(cases.BATCHES) < 16385 and max(pcases.BATCHES) < 16385                                   # (what the older tests stop short of)
    used = {(o, m, w) for _, o, m, w in ecases.PLAIN_TD}
    assert {o for o, _, _ in used} == {5, 11} and {m for _, m, _ in used} == set(model.MODES) and {w for _, _, w in used} == {False, True}
    assert sorted(b for b, _, _, _ in ecases.PLAIN_TD) == sorted(2 * ecases.PLAIN_BATCHES)


def test_grouped_ids_hold_the_intended_counts_and_chunk_counts():
    for how in ("random", "descending"):
        ids = ecases.ids_a(how)
        assert ids.shape == (65555,) and ids.dtype == np.uint8
        assert ecases.counts_of(ids, 3) == [32000, 16400, 16384]
        assert int((ids == 255).sum()) + int((ids == 3).sum()) == 771 and (ids == 255).any() and (ids == 3).any()
    d = ecases.ids_a("descending")
    assert (np.diff(d.astype(np.int64)) <= 0).all() and d[0] == 255 and d[-1] == 0
    r = ecases.ids_a("random")
    assert (np.diff(r.astype(np.int64)) != 0).mean() > 0.5                                               # interleaved, not sorted
    # member 0: G is capped and most workgroups take two chunks; member 1: 1 025 chunks, workgroup 0 alone takes a second; member 2: chunks == G
    assert ecases.td_chunks(32000) == (2000, 1024) and ecases.td_passes(32000) == [0, 48, 976]
    assert ecases.td_chunks(16400) == (1025, 1024) and ecases.td_passes(16400) == [0, 1023, 1]
    assert ecases.td_chunks(16384) == (1024, 1024) and ecases.td_passes(16384) == [0, 1024]
    assert ecases.td_chunks(771)[0] == 49                                                                # nobody's bin: 49 chunks, the last of 3 rows
    # These counts are multiples of 16 and 32 000 rows are 2 000 chunks, fewer than the 2 049 a third pass needs.  The arrangement "full" has
    # no rows of nobody and gives member 0 more than 2 048 chunks, with a partial last chunk on the last pass of every member.
    assert all(c % 16 == 0 for c in ecases.COUNTS_A)
    f = ecases.ids_a("full")
    assert ecases.counts_of(f, 3) == list(ecases.COUNTS_FULL) == [32787, 16385, 16383] and sum(ecases.COUNTS_FULL) == 65555
    assert ecases.td_chunks(32787)[0] == 2050 > 2048 and ecases.td_passes(32787) == [0, 0, 1022, 2]
    assert ecases.td_passes(16385) == [0, 1023, 1] and ecases.td_chunks(16383) == (1024, 1024) and all(c % 16 for c in ecases.COUNTS_FULL)
    used = {(o, m, w) for _, o, m, w in ecases.GROUPED_TD}
    assert {o for o, _, _ in used} == {5, 11} and {m for _, m, _ in used} == set(model.MODES) and {w for _, _, w in used} == {False, True}


@pytest.mark.parametrize("B,OUT,mode,weighted", ecases.PLAIN_TD, ids=ecases.PLAIN_IDS)
def test_plain_exact_operands_pass_the_models_exact_mode(B, OUT, mode, weighted):
    """the loss terms are multiples of 2^-5 bounded by 5: 32 787 of them stay far below 2^24 units, which the model's own assertion confirms"""
    want, _ = model.td_head(exact=True, **cases.td_exact(B, OUT, mode, weighted))
    assert want["loss"] != 0 and np.abs(want["gq"]).sum() > 0


@pytest.mark.parametrize("how,OUT,mode,weighted", ecases.GROUPED_TD, ids=ecases.GROUPED_IDS)
def test_grouped_exact_operands_pass_the_models_exact_mode_for_every_member(how, OUT, mode, weighted):
    ids = ecases.ids_a(how)
    want, _ = pmodel.td_head(cases.td_exact(ecases.BIG_B, OUT, mode, weighted), ids, ecases.K_A, exact=True)
    assert want["loss"].all() and not want["gq"][ids >= ecases.K_A].any()


def test_the_order_model_of_the_loss_sum_sees_the_passes_past_the_cap(monkeypatch):
    """learner_model.loss_order32 is used as it is (a few thousand numpy steps at 32 787 rows: no vectorised copy is kept).  On the random tier the
    terms are positive and most orders of the sum round to the same float (printed): there the bit-equality of the loss sees a term that is missing
    or added twice, rarely the order.  On the signed family (pop_learner_edge_cases.td_signed) the loss that the capped grid's order gives differs, in most
    cases past the cap, from the one of a grid capped elsewhere (every chunk a partial of its own, or 512 workgroups): there it sees the order."""
    def orders(fn):
        out = []
        for cap in (1024, 1 << 20, 512):
            monkeypatch.setattr(model, "MAX_BLOCKS", cap)
            out.append(np.asarray(fn(), np.float32))
        monkeypatch.undo()
        assert model.MAX_BLOCKS == 1024
        return out

    random_same, signed_differ = [], []
    for B, OUT, mode, weighted in ecases.PLAIN_TD:
        if B <= ecases.TD_ONE_PASS:
            continue
        c = cases.td_random(B, OUT, mode, weighted)
        capped, lifted, halved = orders(lambda: model.td_head32(**c)["loss"])
        random_same.append(cases.same_bits(capped, lifted) and cases.same_bits(capped, halved))
        want, E = model.td_head(**c)
        assert cases.within(capped, want["loss"], E["loss"])[0] and cases.within(lifted, want["loss"], E["loss"])[0]
        s = ecases.td_signed(B, OUT, mode)
        capped, lifted, halved = orders(lambda: model.td_head32(**s)["loss"])
        signed_differ.append(not (cases.same_bits(capped, lifted) and cases.same_bits(capped, halved)))
    for how, OUT, mode, weighted in ecases.GROUPED_TD:
        s, ids = ecases.td_signed(ecases.BIG_B, OUT, mode), ecases.ids_a(how)
        capped, lifted, halved = orders(lambda: pmodel.td_head32(s, ids, ecases.K_A)["loss"])
        signed_differ.append(not (cases.same_bits(capped, lifted) and cases.same_bits(capped, halved)))
    print("random tier, loss bits independent of the cap:", random_same, "signed family, loss bits depend on the cap:", signed_differ)
    assert len(signed_differ) == 10 and sum(signed_differ) >= 8


# ---------------------------------------------------------------------- 2. the grouped backward past one sweep of the capped grid
def test_case_a_every_share_is_below_its_need():
    B, counts = ecases.BIG_B, list(ecases.COUNTS_A)
    assert ecases.grad_grid(B) == 512
    shares, needs = ecases.shares(counts, B), ecases.needs(counts)
    assert shares == [250, 129, 128] and needs == [500, 257, 256]
    assert all(s < n for s, n in zip(shares, needs))
    passes = [ecases.group_passes(c, s) for c, s in zip(counts, shares)]
    assert passes == [[0, 0, 1000], [0, 7, 509], [0, 0, 512]]                       # wavefronts by their number of group passes: two for almost all
    # Below one sweep the share equals the need and every wavefront runs one pass: what the older tests run
    assert ecases.shares([2050, 2049], 4099) == ecases.needs([2050, 2049])
    # Case A's counts are multiples of 16, so none of its later passes ends in a partial group.  Case B's do (below).
    assert all(c % 16 == 0 for c in counts)


def test_case_b_packs_the_partials_at_their_maximum():
    counts = ecases.counts_b()
    B, K, X = ecases.BIG_B, ecases.K_B, 512
    assert len(counts) == K and all(c > 0 for c in counts) and sum(counts) <= B
    assert 1 in counts and 64 in counts
    shares = ecases.shares(counts, B)
    assert sum(-(-X * c // B) for c in counts) == X + K - 1 == 527 == sum(shares)    # (the need never cuts a share here)
    assert counts == ecases.counts_b() and ecases.counts_of(ecases.ids_b(), K) == list(counts)
    big = [(c, s) for c, s in zip(counts, shares) if c > 64]
    assert len(big) == 14 and all(s < n for (c, s), n in zip(big, ecases.needs([c for c, _ in big])))
    # at least one member's last pass ends in a partial group: a second pass of a wavefront whose group holds fewer than 16 rows
    partial_later = [c for c, s in big if c % 16 and (-(-c // 16) - 1) >= 4 * s]
    assert partial_later, counts
    assert max(len(ecases.group_passes(c, s)) - 1 for c, s in big) >= 2
    # on a device with fewer CUs the grid is smaller and so is the sum: the GPU test prints it
    assert sum(ecases.shares(counts, B, cus=128)) < 527


@pytest.mark.parametrize("case", ecases.BACKWARD_A, ids=[ecases.backward_id(c) for c in ecases.BACKWARD_A])
def test_case_a_operands_pass_the_models_exact_mode(case):
    kind, hidden, fr = case
    x, gq = gcases.inputs(kind, hidden, "integer", ecases.BIG_B)
    grads, _ = pmodel.backward(x, pcases.exact_team(kind, hidden, ecases.K_A), fr, gq, ecases.ids_a(), exact=True)
    assert all(any(g.any() for g in gs) for gs in grads)


@pytest.mark.parametrize("case", ecases.BACKWARD_B, ids=[ecases.backward_id(c) for c in ecases.BACKWARD_B])
def test_case_b_operands_pass_the_models_exact_mode(case):
    kind, hidden, fr = case
    x, gq = gcases.inputs(kind, hidden, "integer", ecases.BIG_B)
    grads, _ = pmodel.backward(x, pcases.exact_team(kind, hidden, ecases.K_B), fr, gq, ecases.ids_b(), exact=True)
    assert sum(any(g.any() for g in gs) for gs in grads) >= 14


def test_random_tier_inputs_are_the_gathered_familys_with_repeating_rows():
    for kind in ("smart", "mini"):
        hidden = pcases.HIDDEN[kind][0]
        x, gq = ecases.gathered_inputs(kind, hidden)
        fx, fgq = gcases.inputs(kind, hidden, "gathered", ecases.BIG_B)
        assert np.array_equal(gq, fgq) and np.array_equal(x[:4099], fx[:4099]) and np.array_equal(x[4099:2 * 4099], fx[:4099])
        assert len(np.unique(x, axis=0)) == 4099 and (np.count_nonzero(gq, axis=1) == 1).all()
        ids = ecases.ids_a()
        same_member = ids[:-4099] == ids[4099:]                                      # a row and its repeat mostly belong to different members
        assert same_member.mean() < 0.5


# ---------------------------------------------------------------------- 3. grouped Adam as a stage
def test_adam_stage_starts_from_different_control_blocks_and_the_steps_diverge():
    ctls = ecases.adam_start_ctls((0.9, 0.999))
    assert ctls[0] == (0, 1.0, 1.0) and ctls[1][0] == 1000 and ctls[2] == (1, 0.9, 0.999) and len({c[0] for c in ctls}) == 4
    had = np.array([[c > 0 for c in step] for step in ecases.ADAM_STEP_COUNTS]).sum(0)
    assert had.tolist() == [5, 3, 4, 0] and len(ecases.ADAM_STEP_COUNTS) == 5
    for kind, hidden in ecases.ADAM_NETS:                                            # every member its own parameters and gradients
        a, b = cases.adam_case(kind, hidden, seed=0)[0], cases.adam_case(kind, hidden, seed=1)[0]
        assert not any(np.array_equal(u, v) for u, v in zip(a, b))
    w = model.ctl_words(ctls[1])
    assert model.ctl_from_words(w) == ctls[1]
