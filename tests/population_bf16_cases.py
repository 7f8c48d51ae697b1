"""What the CPU and the GPU tests of the populations' grouped bf16 forward share (tests/test_population_bf16_model.py, tests/test_gpu_population_bf16.py;
include/evg_pop_bf16.h): teams, member-id patterns and the composed host model.  The model adds no arithmetic of its own: it routes every row to its
member as tests/population_edge_cases.team_model_q does and evaluates the member's rows with tests/qnet_bf16_model.py; a row of nobody is zeros.

Teams.  Member m of team p is net_params(kind, hidden, family, which=16 * p + m, damaged=(m in (1, 3))) of tests/qnet_bf16_cases.py (exact tier) or of
tests/learner_edge_cases.py (random tier): in the damaged families the damaged weight set sits on members 1 and 3 only.

Id patterns (ids(pattern, rows, K)), arithmetic on arange(rows):
  one           every row on member min(K - 1, 2)
  round_robin   r % K (slot 1 of the two-seat layout: (r + 1) % K): every list is strided through memory
  blocks        r * K // rows: contiguous blocks
  empty         member 0 has no rows: 1 + r % (K - 1); with K = 1 every row is nobody's (255)
  exact1 / exact16 / exact17   member 0 holds exactly the last min(c, rows) rows, the other rows go round the other members (K = 1: to nobody)
  bad           round_robin with the ids of population_edge_cases.BAD_IDS at rows 0, rows // 2, rows - 1 and where r % 5 == 3"""
import numpy as np

import learner_edge_cases as edge
import population_edge_cases as pedge
import qnet_bf16_cases as cases
import qnet_bf16_model as model

TEAM_SIZES = [1, 2, 4, 16]
SEATS_TEAMS = (2, 5)                         # unequal teams of the two-seat layout: ky is the larger one
PATTERNS = ["one", "round_robin", "blocks", "empty", "exact1", "exact16", "exact17", "bad"]
DAMAGED_MEMBERS = (1, 3)
LAYOUTS = pedge.LAYOUTS                      # "expanded", "seat", "seats"
NOBODY = 255


def team(kind, hidden, family, K, p=0):
    src = cases if family in cases.EXACT_FAMILIES else edge
    return [src.net_params(kind, hidden, family, which=16 * p + m, damaged=(m in DAMAGED_MEMBERS)) for m in range(K)]


def ids(pattern, rows, K, slot=0):
    r = np.arange(rows)
    if pattern == "one":
        out = np.full(rows, min(K - 1, 2))
    elif pattern == "round_robin":
        out = (r + slot) % K
    elif pattern == "blocks":
        out = r * K // rows
    elif pattern == "empty":
        out = 1 + (r + slot) % (K - 1) if K > 1 else np.full(rows, NOBODY)
    elif pattern.startswith("exact"):
        c = min(int(pattern[5:]), rows)
        out = 1 + (r + slot) % (K - 1) if K > 1 else np.full(rows, NOBODY)
        out[rows - c:] = 0
    elif pattern == "bad":
        out = (r + slot) % K
        bad = np.asarray(pedge.BAD_IDS)
        bad = np.where(bad < K, NOBODY, bad)                  # (5 is a member of a team of 16)
        at = np.unique(np.concatenate([[0, rows // 2, rows - 1], r[r % 5 == 3]]))
        out[at] = bad[np.arange(len(at)) % len(bad)]
    else:
        raise ValueError(pattern)
    return out.astype(np.uint8)


def layout_ids(pattern, layout, rows, K):
    """the ids of a call: [rows], or [rows, 2] for the two-seat layout with K = (K0, K1)"""
    if layout == "seats":
        return np.stack([ids(pattern, rows, K[0], 0), ids(pattern, rows, K[1], 1)], 1)
    return ids(pattern, rows, K)


def model_layout(layout):
    return "expanded" if layout == "expanded" else "compact"


def _take(layout, inputs, idx):
    return np.ascontiguousarray(inputs[idx]) if layout == "expanded" else tuple(np.ascontiguousarray(a[idx]) for a in inputs)


def forward(kind, layout, teams, inputs, member, final_relu, exact=False, rounds=True):
    """The composed host model -> (Q float32, E float64): every member's rows through qnet_bf16_model with that member's parameters, scattered back;
    zeros (and a zero bound) for the rows of nobody.  teams: the team of the call's seat, or the two teams of the two-seat layout."""
    if layout == "seats":
        shared, swarm = inputs
        qs = [forward(kind, "seat", teams[p], (shared[:, p], swarm[:, p]), member[:, p], final_relu, exact, rounds) for p in range(2)]
        return np.stack([q for q, _ in qs], 1), np.stack([e for _, e in qs], 1)
    n = (inputs if layout == "expanded" else inputs[0]).shape[0]
    shape = (n,) + ((cases.OUT[kind],) if layout == "expanded" else (12, cases.OUT[kind]))
    q, e = np.zeros(shape, np.float32), np.zeros(shape, np.float64)
    member = np.asarray(member)
    for m, params in enumerate(teams):
        at = np.flatnonzero(member == m)
        if len(at):
            q[at], e[at] = model.forward_layout(model_layout(layout), params, _take(layout, inputs, at), final_relu, exact, rounds)
    return q, e


def case_inputs(family, layout, rows=cases.MAX_ROWS):
    """the inputs of qnet_bf16_cases (exact tier) or learner_edge_cases (random tier, its own row counts) in a population's layout"""
    if family in cases.EXACT_FAMILIES:
        if layout == "expanded":
            return cases.expanded_inputs(family, rows)
        return cases.compact_inputs(family, rows, seats=2 if layout == "seats" else 1)
    if layout == "expanded":
        return edge.expanded_inputs(family)
    return edge.compact_inputs(family, seats=2) if layout == "seats" else edge.compact_inputs(family)


def num_rows(layout, inputs):
    return (inputs if layout == "expanded" else inputs[0]).shape[0]
