"""What the CPU and the GPU tests of the Q networks' backward pass share (tests/test_qnet_grad_model.py, tests/test_gpu_qnet_grad.py): shapes, the
seeded families and the comparisons.

Exact tier (the device result must be bit-equal to tests/qnet_grad_model.py; every family passes the model's exact=True at the B it is run at):
  integer      inputs in {-1, 0, 1}, three weights in {-1, 1, 2} per hidden unit (two of +-1 in a later hidden layer), a dense output layer in
               {-1, 0, 1}, integer biases, gq in {-1, 0, 1}: every term of every sum is an integer and the sums stay below 2^24, also over the
               65 555 rows of the sweep case (257 distinct rows, repeated; gq repeats with period 263)
  permutation  one non-zero weight per unit, unit j's at column pi(j mod width) for a seeded permutation, +-1 or +-2 by j; integer inputs in
               [-4, 4], zero hidden biases; integer gq in [-3, 3]: a signed, scaled identity, on which a wrong operand map moves a value
  pow2dup      B equal rows of powers of two (inputs +-2^[-1, 1], the permutation family's structure with weights +-2^[-1, 1], gq +-2^[-1, 1]):
               and positive biases: every row sum is B equal terms, so the gradients are B times the one-row gradients, exactly
Random tier (every element within the model's E): the condition of tests/test_qnet_grad_model.py holds on each -- between 20 % and 80 % of the
(row, hidden unit) pairs are active, and (networks with more than two hidden units in all) hidden unit 0 of layer 1 is dead in every row
  dense        gaussian inputs and weights (scaled by 1 / sqrt(fan-in)), gaussian gq
  gathered     feature-like inputs (34 + 13 values in [0, 1), a one-hot of 12) and gq with one non-zero per row, scaled by 1 / B: what
               gather(1, action) under a mean loss sends back"""
import numpy as np

SMART_HIDDEN = [(60, 60), (1, 1), (3, 64), (64, 7)]
MINI_HIDDEN = [(80,), (1,), (128,)]
NETS = [("smart", h) for h in SMART_HIDDEN] + [("mini", h) for h in MINI_HIDDEN]
NET_IDS = ["%s-%s" % (k, "x".join(map(str, h))) for k, h in NETS]
OUT = {"smart": 5, "mini": 11}
EXACT_FAMILIES = ["integer", "permutation", "pow2dup"]
RANDOM_FAMILIES = ["dense", "gathered"]
ROWS = [1, 15, 16, 17, 63, 65, 256 + 3]                 # row-group and wavefront edges; more than one workgroup
RANDOM_ROWS = 256 + 3
SENTINEL_HIDDEN = [1, 3, 60]
DEAD_UNIT = 0


def sweep_rows(max_blocks):
    """two sweeps of the capped grid (max_blocks workgroups x 4 wavefronts x 16 rows) and 19 rows: the first wavefront of the first workgroup takes
    a third group, the second a third group of 3 rows"""
    return 2 * max_blocks * 64 + 19


def _rng(*key):
    return np.random.default_rng([0x9AD] + [int(k) for k in key])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def sizes(kind, hidden):
    return (59,) + tuple(hidden) + (OUT[kind],)


def has_dead_unit(hidden):
    return sum(hidden) > 2


def params(kind, hidden, family):
    sz = sizes(kind, hidden)
    fam = (EXACT_FAMILIES + RANDOM_FAMILIES).index(family)
    rng = _rng(1, fam, kind == "smart", *hidden)
    layers = len(sz) - 1
    p = []
    for layer in range(layers):
        H, K = sz[layer + 1], sz[layer]
        last = layer == layers - 1
        w, b = np.zeros((H, K)), np.zeros(H)
        j = np.arange(H)
        if family == "integer":
            b = rng.integers(-1, 3, H).astype(np.float64)
            if last:
                w = rng.integers(-1, 2, (H, K)).astype(np.float64)
            else:
                for c in range(3 if layer == 0 else 2):
                    w[j, rng.integers(0, K, H)] = rng.choice([-1.0, 1.0, 2.0] if layer == 0 else [-1.0, 1.0], H)
        elif family in ("permutation", "pow2dup"):
            col = rng.permutation(K)[j % K]
            mag = np.where(j % 3 == 1, 2.0, 1.0) if family == "permutation" else 2.0 ** rng.integers(-1, 2, H)
            w[j, col] = mag * np.where(j % 4 == 2, -1.0, 1.0)
            if last and family == "permutation":
                b = rng.integers(-2, 3, H).astype(np.float64)
            if family == "pow2dup":                   # (positive biases keep most units and outputs of the one row active)
                b = np.full(H, 4.0 if last else 1.0)
        else:
            w = rng.standard_normal((H, K)) / np.sqrt(K) * (1.5 if family == "dense" else 2.0)
            b = rng.standard_normal(H) * 0.3 - (0.4 if (family == "gathered" and layer == 0) or (family == "dense" and not has_dead_unit(hidden)) else 0.0)
            if 0 < layer and not last and not has_dead_unit(hidden):      # (1, 1): a positive weight under a negative bias, so that the one unit is
                w, b = 2.0 * np.abs(w), -np.abs(b) - 0.3                      # active in some rows and dead in others
            if layer == 0 and has_dead_unit(hidden):
                b[DEAD_UNIT] = -1.0e3
        p += [_f32(w), _f32(b)]
    return tuple(p)


def inputs(kind, hidden, family, rows):
    """-> (x [rows, 59], gq [rows, OUT]) float32"""
    out = OUT[kind]
    fam = (EXACT_FAMILIES + RANDOM_FAMILIES).index(family)
    rng = _rng(2, fam, kind == "smart", *hidden)                 # (not a function of rows: the first rows of a longer case are a shorter case)
    r = np.arange(rows)
    if family == "integer":
        ux = rng.integers(-1, 2, (257, 59)) * (rng.random((257, 59)) < 0.5)
        ug = rng.integers(-1, 2, (263, out)) * (rng.random((263, out)) < 0.6)
        x, gq = ux[r % 257], ug[r % 263]
    elif family == "permutation":
        ux, ug = rng.integers(-4, 5, (257, 59)), rng.integers(-3, 4, (263, out))
        x, gq = ux[r % 257], ug[r % 263]
    elif family == "pow2dup":
        x1 = 2.0 ** rng.integers(-1, 2, 59) * rng.choice([-1.0, 1.0], 59)
        g1 = 2.0 ** rng.integers(-1, 2, out) * rng.choice([-1.0, 1.0], out)
        x, gq = np.repeat(x1[None], rows, 0), np.repeat(g1[None], rows, 0)
    elif family == "dense":
        n = max(rows, RANDOM_ROWS)
        x, gq = rng.standard_normal((n, 59))[:rows], rng.standard_normal((n, out))[:rows]
    else:
        n = max(rows, RANDOM_ROWS)
        x = np.zeros((n, 59))
        x[:, :47] = rng.random((n, 47))
        x[np.arange(n), 47 + rng.integers(0, 12, n)] = 1.0
        gq = np.zeros((n, out))
        gq[np.arange(n), rng.integers(0, out, n)] = rng.standard_normal(n) / rows
        x, gq = x[:rows], gq[:rows]
    return _f32(x), _f32(gq)


def case(kind, hidden, family, rows):
    x, gq = inputs(kind, hidden, family, rows)
    return params(kind, hidden, family), x, gq


def same_values(got, want):
    """the exact tier's comparison (the sign of a zero is not part of the contract)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got, want)


def within_bound(got, want, bound):
    """-> (ok, the worst |got - want| / bound); an element whose bound is zero must be equal"""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    if got.shape != want.shape or not np.isfinite(got).all():
        return False, np.inf
    diff = np.abs(got - want)
    ok = bool((diff <= bound).all())
    with np.errstate(all="ignore"):
        ratio = np.where(diff > 0, diff / bound, 0.0)
    return ok, float(ratio.max()) if ratio.size else 0.0
