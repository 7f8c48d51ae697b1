"""What the CPU and the GPU tests of the population kernels at their edges share (tests/test_population_edge_cases.py,
tests/test_gpu_population_edges.py): the grouped forwards of csrc/population_kernels.inc (evg_mini_qnet_pop_kernel, evg_qnet_pop_kernel) under the
numeric families of tests/learner_edge_cases.py, the capped grid past one sweep, and the bucket pass at and past 256 blocks.  Everything here is seeded
numpy on top of learner_edge_cases (`cases`) and the host models; nothing touches a device.

A  Teams of four: member m of team p is cases.net_params(kind, hidden, family, which=4 * p + m, damaged=(m in (1, 3))) -- ordinary and damaged weight sets
   alternate, so a NaN weight or an Inf bias must reach exactly its member's rows, and an `absorbed` input (a -Inf on all-positive columns) is finite on
   members 1 and 3 and NaN on members 0 and 2: the same input tells the members apart.  Row (env) r goes to member (r // 3) % 4, seat slot 1 of the
   two-seat layout to (r // 3 + 1) % 4: runs of three, so that every member holds every damage class r % 7 and undamaged rows, a full group of 16 and a
   partial last one (an assignment like (r + r // 7) % 4 puts every damaged row on members 1 and 3).  The reference is the host model of each member over
   that member's rows, scattered back (team_model_q).
B  R = cases.sweep_rows(cus) rows over four members in four splits (SPLITS); share() restates the grouped kernels' prologue, the member's share of a grid.
C  Member ids for the bucket pass (bucket_ids) and what numpy says the stable list, first and count are (bucket_reference)."""
import numpy as np

import learner_edge_cases as cases

MEMBERS = 4                                  # per team, parts A and B
DAMAGED_MEMBERS = (1, 3)
LAYOUTS = ["expanded", "seat", "seats"]      # pop.expanded, pop.seat, pop(shared, swarm)
MAX_MEMBERS, BINS, BUCKET_BLOCK = 16, 17, 256
GROUP, WAVES = 16, 4                         # rows per wavefront's group, wavefronts per workgroup of the grouped forwards


# ------------------------------------------------------------------------------------------------------------------ part A
def team(kind, hidden, family, p, damaged=DAMAGED_MEMBERS):
    """the four weight sets of team p"""
    return [cases.net_params(kind, hidden, family, which=MEMBERS * p + m, damaged=(m in damaged)) for m in range(MEMBERS)]


def member_ids(rows, slot=0):
    """uint8 [rows]: row r -> member (r // 3 + slot) % 4"""
    return ((np.arange(rows) // 3 + slot) % MEMBERS).astype(np.uint8)


def case_inputs(family, layout):
    """(inputs, member): x [437, 59] and ids [437]; (shared [85, 34], swarm [85, 12, 13]) and ids [85]; or the two-seat pair and ids [85, 2]"""
    if layout == "expanded":
        return cases.expanded_inputs(family), member_ids(cases.ROWS_EXPANDED)
    if layout == "seat":
        return cases.compact_inputs(family), member_ids(cases.ENVS_COMPACT)
    return cases.compact_inputs(family, seats=2), np.stack([member_ids(cases.ENVS_COMPACT, 0), member_ids(cases.ENVS_COMPACT, 1)], 1)


def damaged_inputs(family, layout, inputs):
    """bool [rows] or [envs, 2]: the rows (envs, seats) that carry a non-finite input"""
    if layout == "expanded":
        return cases.damaged_rows(family, inputs.shape[0])
    shared, swarm = inputs
    if layout == "seat":
        return cases.damaged_rows(family, shared.shape[0])
    return ~(np.isfinite(shared).all(2) & np.isfinite(swarm).all((2, 3)))


def _take(layout, inputs, idx):
    return inputs[idx] if layout == "expanded" else (inputs[0][idx], inputs[1][idx])


def team_model_q(kind, layout, teams, inputs, member, final_relu=False, rows=None):
    """The host model's Q of a grouped forward: every member's rows through that member's parameters, scattered back to their places.  teams: the team
    of the call's seat, or the two teams of the two-seat layout; member as case_inputs gives it; rows: the rows (envs) to compute (default all) -- the
    result then has len(rows) rows, in that order."""
    if layout == "seats":
        shared, swarm = inputs
        return np.stack([team_model_q(kind, "seat", teams[p], (shared[:, p], swarm[:, p]), member[:, p], final_relu, rows) for p in range(2)], 1)
    n = (inputs if layout == "expanded" else inputs[0]).shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out_dim = 5 if kind == "smart" else 11
    q = np.zeros((len(rows),) + ((out_dim,) if layout == "expanded" else (12, out_dim)), np.float32)
    ids = np.asarray(member)[rows]
    for m in range(len(teams)):
        at = np.flatnonzero(ids == m)
        if len(at):
            q[at] = cases.model_q(kind, "expanded" if layout == "expanded" else "compact", teams[m], _take(layout, inputs, rows[at]), final_relu)
    assert (ids < len(teams)).all()
    return q


def members_cover_groups_and_damage(member, rows):
    """every member has a full group of 16 and a partial last one, every damage class r % 7 in (1, 3, 5) and undamaged rows; -> the member counts"""
    r = np.arange(rows)
    counts = np.bincount(member, minlength=MEMBERS)
    for m in range(MEMBERS):
        assert counts[m] > GROUP and counts[m] % GROUP != 0, (m, counts)
        mine = r[member == m] % 7
        assert all((mine == c).sum() >= (15 if rows >= 400 else 3) for c in (1, 3, 5)), (m, np.bincount(mine, minlength=7))
        assert np.isin(mine, (0, 2, 4, 6)).sum() >= 3
    return counts


# ------------------------------------------------------------------------------------------------------------------ part B
SPLITS = ["one", "even", "three_quarters", "crumbs"]


def split_ids(split, R):
    """uint8 [R], arithmetic on arange(R):
    one             every row on member 2: its workgroups are the whole grid and sweep twice
    even            r % 4: each member's share is a quarter of the grid
    three_quarters  member 0 where r % 4 != 3 and r != R - 1, else member 1.  On 256 CUs (R = 32 785, a grid of 512 workgroups): cnt = 24 588 rows for
                    member 0, live = ceil(512 * 24 588 / 32 785) = 384 workgroups, need = ceil(24 588 / 64) = 385 -- its share of the grid is one workgroup
                    short of its need, live * 64 = 24 576 < cnt, so its wavefronts run with a stride of live * 4 = 1 536 groups and wavefront 0 of workgroup
                    0 sweeps a second time, over group 1 536: the last 12 rows, a partial group.  (With row R - 1 on member 0 as well, cnt = 24 589 gives
                    ceil(384.004) = 385 = need and nobody sweeps twice: the share is rounded up, and R is 17 rows past the grid.)  Member 1: cnt = 8 197,
                    live = need = 129.
    crumbs          members 1 to 3 hold one row each (rows 0, R // 2, R - 1), member 0 the other R - 3 (live = 512 < need = 513 on 256 CUs)"""
    r = np.arange(R)
    if split == "one":
        ids = np.full(R, 2)
    elif split == "even":
        ids = r % 4
    elif split == "three_quarters":
        ids = np.where((r % 4 != 3) & (r != R - 1), 0, 1)
    elif split == "crumbs":
        ids = np.zeros(R, np.int64)
        ids[[0, R // 2, R - 1]] = [1, 2, 3]
    else:
        raise ValueError(split)
    return ids.astype(np.uint8)


def grid_blocks(rows, cus):
    """gridDim.x of a grouped forward: the plain launch's grid, capped at two workgroups per CU"""
    return min((rows + GROUP * WAVES - 1) // (GROUP * WAVES), 2 * cus)


def share(cnt, rows, cus):
    """(live, need) of a member with cnt of the call's rows: the workgroups it gets of the grid, and those it would fill (the grouped kernels' prologue)"""
    need = (cnt + GROUP * WAVES - 1) // (GROUP * WAVES)
    live = (grid_blocks(rows, cus) * cnt + rows - 1) // rows
    return min(live, need), need


# ------------------------------------------------------------------------------------------------------------------ part C
BUCKET_K = 5
BUCKET_ROWS = [65536, 65537, 131073]         # nb = 256 (the last size with per = 1), 257 (per = 2: thread 128 owns one block), 513 (per = 3)
PATTERNS = ["uniform", "one", "window", "bad"]
WINDOW = (70000, 70300)                      # the only rows of member 3 in the pattern "window"
BAD_IDS = (5, 16, 200, 255)


def scan_per(rows):
    nb = (rows + BUCKET_BLOCK - 1) // BUCKET_BLOCK
    return nb, (nb + 255) // 256


def bucket_ids(pattern, rows, key=0):
    """uint8 [rows] member ids for a team of BUCKET_K:
    uniform  a seeded uniform draw
    one      every row on member 4
    window   the draw over members 0, 1, 2 and 4, member 3 in rows WINDOW alone: long runs of blocks without member 3 on either side (rows > WINDOW[1])
    bad      the draw with ids 5, 16, 200, 255 (nobody's) at rows 0, 255, 256, rows - 1 and 64 seeded others"""
    rng = np.random.default_rng([0xB0C7, PATTERNS.index(pattern), rows, key])
    if pattern == "one":
        return np.full(rows, BUCKET_K - 1, np.uint8)
    ids = rng.integers(0, BUCKET_K, rows)
    if pattern == "window":
        assert rows > WINDOW[1]
        ids = np.where(ids == 3, 4, ids)
        ids[WINDOW[0]:WINDOW[1]] = 3
    elif pattern == "bad":
        at = np.unique(np.concatenate([[0, 255, 256, rows - 1], rng.choice(rows, 64, replace=False)]))
        ids[at] = np.asarray(BAD_IDS)[np.arange(len(at)) % 4]
    elif pattern != "uniform":
        raise ValueError(pattern)
    return ids.astype(np.uint8)


def bucket_reference(ids, K=BUCKET_K):
    """(list, first, count) of one seat slot: the stable sort of the rows by bin, ids >= K in bin 16"""
    bins = np.where(ids < K, ids, MAX_MEMBERS).astype(np.int64)
    order = np.argsort(bins, kind="stable").astype(np.int32)
    count = np.bincount(bins, minlength=BINS).astype(np.int32)
    first = (np.cumsum(count) - count).astype(np.int32)
    return order, first, count
