"""CPU tests (no GPU needed) of tests/population_edge_cases.py, on the host models alone: the teams, assignments and inputs that
tests/test_gpu_population_edges.py sends through the grouped forwards reach what they name -- every member holds full and partial groups and every damage
class, a damaged weight set stays with its member, `absorbed` tells the members apart, no case drowns in NaN -- and the splits of the capped grid and
the member ids of the bucket pass have the shapes their names promise."""
import numpy as np
import pytest

import learner_edge_cases as cases
import population_edge_cases as pec

NETS = [("smart", h) for h in cases.SMART_HIDDEN] + [("mini", h) for h in cases.MINI_HIDDEN]
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")           # numpy's overflow and invalid-value warnings are the subject here
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)        # noqa: E731

_Q = {}


def _q(kind, hidden, family, layout):
    """(inputs, member, the model's Q without the final ReLU) of one case of part A, computed once"""
    key = (kind, hidden, family, layout)
    if key not in _Q:
        inputs, member = pec.case_inputs(family, layout)
        teams = [pec.team(kind, hidden, family, p) for p in range(2)]
        _Q[key] = (inputs, member, pec.team_model_q(kind, layout, teams if layout == "seats" else teams[0], inputs, member))
    return _Q[key]


def test_the_assignment_gives_every_member_groups_and_every_damage_class():
    assert pec.members_cover_groups_and_damage(pec.member_ids(cases.ROWS_EXPANDED), cases.ROWS_EXPANDED).tolist() == [111, 110, 108, 108]
    assert pec.members_cover_groups_and_damage(pec.member_ids(cases.ENVS_COMPACT), cases.ENVS_COMPACT).tolist() == [22, 21, 21, 21]
    assert pec.members_cover_groups_and_damage(pec.member_ids(cases.ENVS_COMPACT, 1), cases.ENVS_COMPACT).tolist() == [21, 22, 21, 21]
    # the assignment that was tried first holds no damaged row on members 0 and 2
    r = np.arange(cases.ROWS_EXPANDED)
    first_try = (r + r // 7) % 4
    assert not np.isin(r[np.isin(first_try, (0, 2))] % 7, (1, 3, 5)).any()


def test_teams_alternate_ordinary_and_damaged_weight_sets():
    for kind, hidden in NETS:
        for family in cases.WEIGHT_DAMAGE:
            for p in range(2):
                t = pec.team(kind, hidden, family, p)
                clean = pec.team(kind, hidden, family, p, damaged=())
                for m in range(pec.MEMBERS):
                    same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(t[m], clean[m]))
                    if family == "absorbed" and min(hidden) == 1 and m in pec.DAMAGED_MEMBERS:
                        continue                                            # (one unit's two columns may be positive as drawn)
                    assert same == (m not in pec.DAMAGED_MEMBERS), (kind, hidden, family, p, m)
            w1 = [pec.team(kind, hidden, family, p)[m][0] for p in range(2) for m in range(pec.MEMBERS)]
            assert len({a.tobytes() for a in w1}) == 8                      # eight different members


@pytest.mark.parametrize("layout", pec.LAYOUTS)
@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("kind,hidden", NETS, ids=_ids)
def test_every_case_reaches_what_its_family_names(kind, hidden, family, layout):
    inputs, member, q = _q(kind, hidden, family, layout)
    rows = q.shape[0]
    flat = q.reshape((rows, 2, -1) if layout == "seats" else (rows, 1, -1))             # [rows, seat slot, values]
    ids = member.reshape(rows, -1)
    bad = pec.damaged_inputs(family, layout, inputs).reshape(rows, -1)
    nan = np.isnan(flat)
    # at most half of the compared values are NaN (with the final ReLU as without it: it keeps a NaN)
    assert nan.mean() <= 0.5, nan.mean()
    ordinary = ~np.isin(ids, pec.DAMAGED_MEMBERS)
    # a damaged weight set stays with its member: without a damaged input an ordinary member's Q holds no NaN
    if family != "overflow":
        assert (ordinary & ~bad).sum() >= 20 and not nan[ordinary & ~bad].any()
    if family in ("nan_weight", "inf_bias") and min(hidden) >= 16:
        assert (~np.isfinite(flat[~ordinary])).any(-1).all()               # ... and every row of a damaged member shows it
    if family == "absorbed" and min(hidden) >= 17:
        # the same -Inf input: NaN on members 0 and 2 (signed columns), finite on members 1 and 3 (positive columns, the ReLU absorbs it)
        assert (bad & ordinary).sum() >= 6 and (bad & ~ordinary).sum() >= 6
        assert nan[bad & ordinary].any(-1).all() and not nan[bad & ~ordinary].any()
        assert np.isfinite(flat[bad & ~ordinary]).all()
        if layout == "expanded":
            assert nan[bad & ordinary].mean() >= 0.9                       # (1.0 but for Minimized 17: 0.91 to 0.96)
    if family == "subnormal":
        for slot in range(ids.shape[1]):
            for m in range(pec.MEMBERS):
                assert cases.is_subnormal(flat[:, slot][ids[:, slot] == m]).any(), (slot, m)


def test_two_seat_case_has_two_different_teams_and_assignments():
    inputs, member, q = _q("mini", (17,), "signed", "seats")
    assert member.shape == (cases.ENVS_COMPACT, 2) and (member[:, 0] != member[:, 1]).all()
    other = pec.team_model_q("mini", "seat", pec.team("mini", (17,), "signed", 0), (inputs[0][:, 1], inputs[1][:, 1]), member[:, 1])
    assert not np.array_equal(other, q[:, 1])                               # seat 1's Q is team 1's


def test_model_of_chosen_rows_equals_the_rows_of_the_whole():
    inputs, member, q = _q("mini", (80,), "nonfinite", "seats")
    teams = [pec.team("mini", (80,), "nonfinite", p) for p in range(2)]
    rows = np.array([84, 0, 17, 3, 50])
    assert cases.same_values(pec.team_model_q("mini", "seats", teams, inputs, member, rows=rows), q[rows])


# ------------------------------------------------------------------------------------------------------------------ part B
@pytest.mark.parametrize("cus", [256])
def test_splits_of_the_capped_grid(cus):
    R = cases.sweep_rows(cus)
    grid = pec.grid_blocks(R, cus)
    assert R == 32785 and grid == 512 and grid * 64 < R
    counts = {s: np.bincount(pec.split_ids(s, R), minlength=pec.MEMBERS) for s in pec.SPLITS}
    assert counts["one"].tolist() == [0, 0, R, 0] and counts["even"].tolist() == [8197, 8196, 8196, 8196]
    assert counts["three_quarters"].tolist() == [24588, 8197, 0, 0] and counts["crumbs"].tolist() == [R - 3, 1, 1, 1]
    ids = pec.split_ids("three_quarters", R)
    assert (ids[np.arange(R) % 4 == 3] == 1).all() and (ids[:R - 1][np.arange(R - 1) % 4 != 3] == 0).all() and ids[R - 1] == 1
    # three_quarters: member 0's share of the grid is smaller than its need -- its wavefronts take a second sweep, which ends on a partial group
    cnt = int(counts["three_quarters"][0])
    live, need = pec.share(cnt, R, cus)
    assert (live, need) == (384, 385) and live * 64 < cnt
    groups = (cnt + 15) // 16
    assert groups == live * 4 + 1 and cnt % 16 == 12                        # one group past the first sweep, of 12 rows
    assert pec.share(int(counts["three_quarters"][1]), R, cus) == (129, 129)
    # with row R - 1 on member 0 as well the rounded-up share equals the need and nobody sweeps twice
    assert pec.share(cnt + 1, R, cus) == (385, 385)
    # one and crumbs: the whole grid, one workgroup short; even: members 1 to 3 (8 196 rows) are 4 rows past their 128 workgroups
    assert pec.share(R, R, cus) == (512, 513) and pec.share(R - 3, R, cus) == (512, 513) and pec.share(1, R, cus) == (1, 1)
    assert [pec.share(int(c), R, cus) for c in counts["even"]] == [(129, 129)] + [(128, 129)] * 3
    crumbs = pec.split_ids("crumbs", R)
    assert (crumbs[0], crumbs[R // 2], crumbs[R - 1]) == (1, 2, 3)


# ------------------------------------------------------------------------------------------------------------------ part C
def test_bucket_row_counts_straddle_256_blocks():
    assert [pec.scan_per(r) for r in pec.BUCKET_ROWS] == [(256, 1), (257, 2), (513, 3)]
    nb, per = pec.scan_per(65537)
    owners = [(t * per, min(t * per + per, nb)) for t in range(256) if t * per < nb]
    assert len(owners) == 129 and owners[128] == (256, 257)                 # thread 128 owns the single last block, threads 129 to 255 none
    nb, per = pec.scan_per(131073)
    assert len([t for t in range(256) if t * per < nb]) == 171


@pytest.mark.parametrize("rows", pec.BUCKET_ROWS)
def test_bucket_patterns_and_their_reference(rows):
    K = pec.BUCKET_K
    for pattern in pec.PATTERNS:
        if pattern == "window" and rows <= pec.WINDOW[1]:
            continue
        ids = pec.bucket_ids(pattern, rows)
        order, first, count = pec.bucket_reference(ids)
        assert ids.dtype == np.uint8 and len(order) == rows and count.sum() == rows and first[0] == 0
        assert np.array_equal(order, np.argsort(np.minimum(np.where(ids >= K, 16, ids), 16), kind="stable"))
        assert np.array_equal(first[1:], np.cumsum(count)[:-1])
        for b in range(pec.BINS):                                           # a bin's rows ascend, and they are that bin's rows
            mine = order[first[b]:first[b] + count[b]]
            assert (np.diff(mine) > 0).all() and ((ids[mine] == b).all() if b < K else b == 16 or len(mine) == 0)
        if pattern == "uniform":
            assert (count[:K] > rows // (2 * K)).all() and count[K:].sum() == 0
        elif pattern == "one":
            assert count[K - 1] == rows
        elif pattern == "window":
            blocks = np.add.reduceat((ids == 3).astype(np.int64), np.arange(0, rows, pec.BUCKET_BLOCK))
            with3 = np.flatnonzero(blocks)
            assert count[3] == 300 and with3.tolist() == [273, 274] and len(blocks) == 513        # 273 empty blocks before, 238 after
        else:
            bad = np.flatnonzero(ids >= K)
            assert count[16] == len(bad) and 64 <= len(bad) <= 68 and {0, 255, 256, rows - 1} <= set(bad.tolist())
            assert set(ids[bad].tolist()) == set(pec.BAD_IDS) and np.array_equal(order[first[16]:], bad)
    assert not np.array_equal(pec.bucket_ids("uniform", rows, 0), pec.bucket_ids("uniform", rows, 1))
