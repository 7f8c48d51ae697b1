"""What the CPU and the GPU tests of the Q networks' bf16 forward share (tests/test_qnet_bf16_model.py, tests/test_gpu_qnet_bf16.py): shapes, the seeded
exact-tier families and the comparisons.  The random tier's families are those of tests/learner_edge_cases.py.

Exact tier (the device result must be bit-equal to tests/qnet_bf16_model.py; every family passes the model's exact=True):
  integer      integer inputs in [-2, 2], w1 in {-1, 0, 1}, integer biases in [-3, 3]; a hidden row of a later layer has two weights of +-1, the output
               layer is dense in [-2, 2]: every hidden value is an integer of magnitude <= 256, every sum stays far below 2^24
  permutation  one non-zero per weight row, row j's at column pi(j mod width) for a seeded permutation pi, with a value of its own per row (layer 1:
               odd 4-bit mantissas times powers of two; later layers: powers of two), inputs with a 4-bit mantissa and a value of their own per
               column, zero biases: an asymmetric identity whose every product is a bfloat16 value
  rounding     one non-zero per row and zero biases, so that every sum is one exact product; inputs and weights that NEED rounding (both tie
               directions, just above a tie, negatives, the largest float: it rounds to Inf); the 16-bit products force the hidden rounding
  nonfinite    the integer family with, in row r, r % 7 == 1 a NaN, == 3 a +Inf, == 5 a -Inf input; in the (one, or seat 1's) weight set a NaN in the
               output layer's weight [3][5], b1[0] = -Inf and the output layer's bias [1] = +Inf; hidden sizes with padded units (17)
A row is a row of x in the expanded layout and an env in the compact ones; the two-seat layout has a weight set per seat, differently seeded."""
import numpy as np

import qnet_bf16_model as model

SMART_HIDDEN = [(60, 60), (17, 64), (1, 1), (64, 64)]
MINI_HIDDEN = [(80,), (128,), (17,), (1,)]
NETS = [("smart", h) for h in SMART_HIDDEN] + [("mini", h) for h in MINI_HIDDEN]
NONFINITE_NETS = [("smart", (17, 64)), ("mini", (17,))]
# (the nonfinite family runs at the hidden sizes with padded units)
EXACT_CASES = [(k, h, f) for k, h in NETS for f in ("integer", "permutation", "rounding")] + [(k, h, "nonfinite") for k, h in NONFINITE_NETS]
EXACT_IDS = ["%s-%s-%s" % (k, "x".join(map(str, h)), f) for k, h, f in EXACT_CASES]
NET_IDS = ["%s-%s" % (k, "x".join(map(str, h))) for k, h in NETS]
LAYOUTS = ["expanded", "compact", "seats"]
EXACT_FAMILIES = ["integer", "permutation", "rounding", "nonfinite"]
RANDOM_FAMILIES = ["signed", "absorbed", "zero_column"]
ROWS = [1, 15, 16, 17, 37]
MAX_ROWS = 37
DAMAGE = {1: np.nan, 3: np.inf, 5: -np.inf}
OUT = {"smart": 5, "mini": 11}
FLT_MAX = np.finfo(np.float32).max
# values that need rounding: the tie that goes down to even, the tie that goes up to even, just above a tie, a plain one, and their negatives
ROUNDED = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1.7182817, 3 + 2.0 ** -7, 0.3333333]


def _rng(*key):
    return np.random.default_rng([0xBF16] + [int(k) for k in key])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _sizes(kind, hidden):
    return (59,) + tuple(hidden) + (OUT[kind],)


def _one_per_row(rng, rows, width):
    """the column of each row's one non-zero: pi(j mod width)"""
    pi = rng.permutation(width)
    return pi[np.arange(rows) % width]


def net_params(kind, hidden, family, which=0, damaged=True):
    sizes = _sizes(kind, hidden)
    fam = "integer" if family == "nonfinite" else family
    rng = _rng(1, EXACT_FAMILIES.index(fam), kind == "smart", which, *hidden)
    p = []
    layers = len(sizes) - 1
    for layer in range(layers):
        H, K = sizes[layer + 1], sizes[layer]
        w, b = np.zeros((H, K)), np.zeros(H)
        j = np.arange(H)
        if fam == "integer":
            b = rng.integers(-3, 4, H).astype(np.float64)
            if layer == 0:
                w = rng.integers(-1, 2, (H, K)).astype(np.float64)
            elif layer == layers - 1:
                w = rng.integers(-2, 3, (H, K)).astype(np.float64)
            else:
                for c in range(2):
                    w[j, rng.integers(0, K, H)] = rng.choice([-1.0, 1.0], H)
        elif fam == "permutation":
            col = _one_per_row(rng, H, K)
            if layer == 0:          # 8 odd mantissas x 16 exponents: 128 values, one per row; every eighth negative
                w[j, col] = (2 * (j % 8) + 1) * 2.0 ** (j // 8 - 14) * np.where(j % 8 == 5, -1.0, 1.0)
            else:                   # powers of two 2^(6 - H) .. 2^5, one per row; every sixteenth negative
                w[j, col] = 2.0 ** (j + 6 - H) * np.where(j % 16 == 7, -1.0, 1.0)
        elif fam == "rounding":
            col = _one_per_row(rng, H, K)
            v = np.array(ROUNDED)[rng.integers(0, len(ROUNDED), H)] * rng.choice([1.0, 1.0, 1.0, -1.0], H) * 2.0 ** rng.integers(-2, 3, H)
            w[j, col] = v
        p += [_f32(w), _f32(b)]
    if family == "nonfinite" and damaged:
        p[1][0] = -np.inf
        wl, bl = p[-2], p[-1]
        wl[3, min(5, wl.shape[1] - 1)] = np.nan
        bl[1] = np.inf
    return tuple(p)


def _inputs_flat(family, rng, shape):
    """float64 array of `shape` whose last axis is a feature axis"""
    fam = "integer" if family == "nonfinite" else family
    n = int(np.prod(shape))
    if fam == "integer":
        return rng.integers(-2, 3, shape).astype(np.float64)
    if fam == "permutation":       # a value per column: 8 odd 4-bit mantissas x 8 exponents, rotated per row; every seventh negative
        k = (np.arange(n).reshape(shape) * 1 + rng.integers(0, 64)) % 64
        return (2 * (k % 8) + 1) * 2.0 ** (k // 8 - 3) * np.where(k % 7 == 3, -1.0, 1.0)
    v = np.array(ROUNDED)[rng.integers(0, len(ROUNDED), shape)] * rng.choice([1.0, 1.0, 1.0, -1.0], shape) * 2.0 ** rng.integers(-2, 3, shape)
    v[rng.random(shape) < 0.003] = FLT_MAX          # rounds to +Inf
    return v


def expanded_inputs(family, rows):
    x = _inputs_flat(family, _rng(2, EXACT_FAMILIES.index(family), rows), (rows, 59))
    if family == "nonfinite":
        r = np.arange(rows)
        for m, v in DAMAGE.items():
            rr = r[r % 7 == m]
            x[rr, (5 * rr + 2) % 59] = v
    return _f32(x)


def compact_inputs(family, envs, seats=1):
    rng = _rng(3, EXACT_FAMILIES.index(family), envs, seats)
    shared = _inputs_flat(family, rng, (envs, seats, 34))
    swarm = _inputs_flat(family, rng, (envs, seats, 12, 13))
    if family == "nonfinite":
        for r in range(envs):
            if r % 7 in DAMAGE:
                c, p = (5 * r + 2) % 47, (r // 7) % seats
                if c < 34:
                    shared[r, p, c] = DAMAGE[r % 7]
                else:
                    swarm[r, p, r % 12, c - 34] = DAMAGE[r % 7]
    if seats == 1:
        shared, swarm = shared[:, 0], swarm[:, 0]
    return _f32(shared), _f32(swarm)


def case(kind, hidden, family, layout, rows=MAX_ROWS):
    """(params, inputs) of one exact-tier case; params are one set, or the two sets of the two-seat layout (seat 1's the damaged one)"""
    if layout == "expanded":
        return net_params(kind, hidden, family), expanded_inputs(family, rows)
    if layout == "compact":
        return net_params(kind, hidden, family), compact_inputs(family, rows)
    return (net_params(kind, hidden, family, 0, damaged=False), net_params(kind, hidden, family, 1)), compact_inputs(family, rows, seats=2)


def first_rows(layout, inputs, rows):
    """the first `rows` rows (envs) of a case's inputs, contiguous"""
    if layout == "expanded":
        return np.ascontiguousarray(inputs[:rows])
    return tuple(np.ascontiguousarray(a[:rows]) for a in inputs)


def pick_rows(layout, inputs, idx):
    if layout == "expanded":
        return np.ascontiguousarray(inputs[idx])
    return tuple(np.ascontiguousarray(a[idx]) for a in inputs)


def same_values(got, want):
    """The exact tier's comparison: equal NaN masks, equal values elsewhere (the sign of a zero is not part of the contract)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)


def within_bound(got, want, bound):
    """The random tier's comparison -> (ok, the worst |got - want| / bound over the finite outputs): equal NaN masks, equal infinities, and
    |got - want| <= bound elementwise elsewhere."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False, np.inf
    inf = np.isinf(want) | np.isinf(got)
    fin = ~inf & ~np.isnan(want)
    ok = np.array_equal(got[inf], want[inf])
    diff = np.abs(got[fin] - want[fin])
    ok = ok and bool((diff <= bound[fin]).all())
    with np.errstate(all="ignore"):
        ratio = np.where(diff > 0, diff / bound[fin], 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0


def sweep_rows(cus):
    """One full sweep of the bf16 launches' capped grid (2 workgroups per CU x 4 wavefronts x 16 rows), one more group and one row: the wavefronts of the
    first workgroup take a second group, the last group holds one row."""
    return 16 * 4 * 2 * cus + 17


def sweep_checked_rows(rows, cus):
    """the rows compared with the host model: the first group, the 96 rows around the sweep boundary, the last 33 rows and 512 random rows"""
    edge = 16 * 4 * 2 * cus
    pick = np.concatenate([np.arange(16), np.arange(edge - 48, edge + 48), np.arange(rows - 33, rows), _rng(4, rows).choice(rows, 512, replace=False)])
    return np.unique(pick[(pick >= 0) & (pick < rows)])
