"""What the CPU and the GPU tests of the agents/DQN Q network's backward pass share (tests/test_dqn_grad_model.py, tests/test_gpu_dqn_grad.py): shapes,
the seeded families for the 105-h1-132 network and the comparisons.

Exact tier (the device result must be bit-equal to tests/dqn_grad_model.py; every family passes the model's exact=True at every B it is run at):
  integer      inputs in {-1, 0, 1}, three weights in {-1, 1, 2} per hidden unit, a dense output layer in {-1, 0, 1}, integer biases, gq in
               {-1, 0, 1}: every term of every sum is an integer and the sums stay below 2^24, also over the 32 787 rows of the sweep case (257
               distinct rows, repeated; gq repeats with period 263)
  permutation  one non-zero weight per unit, unit j's at column pi(j mod width) for a seeded permutation, +-1 or +-2 by j; integer inputs in
               [-4, 4], zero hidden biases; integer gq in [-3, 3]: a signed, scaled identity, on which a wrong operand map moves a value
  pow2dup      B equal rows of powers of two (inputs +-2^[-1, 1], the permutation family's structure with weights +-2^[-1, 1], gq +-2^[-1, 1]) and
               positive biases: every row sum is B equal terms, so the gradients are B times the one-row gradients, exactly
Random tier (every element within the model's E): between 20 % and 80 % of the (row, hidden unit) pairs are active and hidden unit 0 is dead in
every row (tests/test_dqn_grad_model.py asserts it)
  dense        gaussian inputs and weights (scaled by 1 / sqrt(fan-in)), gaussian gq
  gathered7    inputs in [0, 1) and gq with seven entries per row at columns drawn WITH repetition, repeated columns adding, each scaled by
               1 / (7 B): what gather(1, action[B, 7]) under a mean loss sends back"""
import numpy as np

from qnet_grad_cases import same_values, within_bound       # noqa: F401  (the comparisons are the small networks')

IN, OUT = 105, 132
HIDDEN = [1, 17, 47, 48, 49, 96, 527, 528]              # one unit; tile and chunk edges; two chunks; the last chunk ragged and full
ROWS = [1, 2, 3, 5, 15, 16, 17, 63, 65, 256 + 3]
BOTH_RELU_HIDDEN = [48, 528]
EXACT_FAMILIES = ["integer", "permutation", "pow2dup"]
RANDOM_FAMILIES = ["dense", "gathered7"]
RANDOM_HIDDEN = [48, 528]
RANDOM_ROWS = 256 + 3
SENTINEL_HIDDEN = [1, 47, 528]
SWEEP_HIDDEN = 49
DEAD_UNIT = 0


def sweep_rows(max_blocks):
    """two sweeps of the delta kernel's capped grid (max_blocks workgroups x 4 wavefronts x 16 rows) and 19 rows: every workgroup runs its pass loop
    twice, the first takes a third pass, whose second wavefront holds 3 rows and whose last two hold none"""
    return 2 * max_blocks * 64 + 19


def _rng(*key):
    return np.random.default_rng([0xD9A] + [int(k) for k in key])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def has_dead_unit(h1):
    return h1 > 2


def params(h1, family):
    fam = (EXACT_FAMILIES + RANDOM_FAMILIES).index(family)
    rng = _rng(1, fam, h1)
    p = []
    for layer, (H, K) in enumerate(((h1, IN), (OUT, h1))):
        last = layer == 1
        w, b = np.zeros((H, K)), np.zeros(H)
        j = np.arange(H)
        if family == "integer":
            b = rng.integers(-1, 3, H).astype(np.float64)
            if last:
                w = rng.integers(-1, 2, (H, K)).astype(np.float64)
            else:
                for c in range(3):
                    w[j, rng.integers(0, K, H)] = rng.choice([-1.0, 1.0, 2.0], H)
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
            b = rng.standard_normal(H) * 0.3 - (0.4 if family == "gathered7" and layer == 0 else 0.0)
            if layer == 0 and has_dead_unit(h1):
                b[DEAD_UNIT] = -1.0e3
        p += [_f32(w), _f32(b)]
    return tuple(p)


def inputs(h1, family, rows):
    """-> (x [rows, 105], gq [rows, 132]) float32"""
    fam = (EXACT_FAMILIES + RANDOM_FAMILIES).index(family)
    rng = _rng(2, fam, h1)                               # (not a function of rows: the first rows of a longer case are a shorter case)
    r = np.arange(rows)
    if family == "integer":
        ux = rng.integers(-1, 2, (257, IN)) * (rng.random((257, IN)) < 0.5)
        ug = rng.integers(-1, 2, (263, OUT)) * (rng.random((263, OUT)) < 0.6)
        x, gq = ux[r % 257], ug[r % 263]
    elif family == "permutation":
        ux, ug = rng.integers(-4, 5, (257, IN)), rng.integers(-3, 4, (263, OUT))
        x, gq = ux[r % 257], ug[r % 263]
    elif family == "pow2dup":
        x1 = 2.0 ** rng.integers(-1, 2, IN) * rng.choice([-1.0, 1.0], IN)
        g1 = 2.0 ** rng.integers(-1, 2, OUT) * rng.choice([-1.0, 1.0], OUT)
        x, gq = np.repeat(x1[None], rows, 0), np.repeat(g1[None], rows, 0)
    elif family == "dense":
        n = max(rows, RANDOM_ROWS)
        x, gq = rng.standard_normal((n, IN))[:rows], rng.standard_normal((n, OUT))[:rows]
    else:
        n = max(rows, RANDOM_ROWS)
        x = rng.random((n, IN))
        cols, vals = rng.integers(0, OUT, (n, 7)), rng.standard_normal((n, 7)) / (7.0 * rows)
        gq = np.zeros((n, OUT))
        np.add.at(gq, (np.arange(n)[:, None], cols), vals)       # repeated columns add
        x, gq = x[:rows], gq[:rows]
    return _f32(x), _f32(gq)


def case(h1, family, rows):
    x, gq = inputs(h1, family, rows)
    return params(h1, family), x, gq
