"""What the CPU and the GPU tests of the learner-side kernels at their numeric and shape edges share (tests/test_learner_edge_cases.py,
tests/test_gpu_learner_edges.py): seeded input and weight families for the two Q networks (evg_smart_qnet, evg_minimized_qnet) and a synthetic driver of
the replay memory (evg_replay_*), with what the host models (qnet_model, minimized_model, replay_model) say about them.

Q-network families (every array float32, seeded by family, sizes and layout):
  signed       inputs N(0, 1) -- negative features, shared and swarm alike --, weights and biases N(0, 0.3^2)
  subnormal    inputs N(0, 1) * 2^-40, w1 N(0, 1) * 2^-88 (its one-hot columns 47.. * 2^-128), b1 N(0, 1) * 2^-128, later weights N(0, 0.3^2), later
               biases N(0, 1) * 2^-130: the first hidden layer and Q are partly non-zero subnormals
  overflow     inputs N(0, 1) * 2^(3 (row mod 24) - 12); Smart: every weight N(0, 1) * 2^40; Minimized: w1 N(0, 1) * 2^80 (hidden units overflow in the
               rows of large scale), w2 N(0, 1) * 2^40; biases N(0, 1): Q holds NaN (Inf - Inf in the next layer), +-Inf and finite values
  nonfinite    ordinary weights, inputs N(0, 1); row r with r % 7 == 1 holds one NaN, == 3 one +Inf, == 5 one -Inf (DAMAGE); the other rows are finite
  nan_weight   ordinary inputs; one NaN in the last layer but one's weight [3][5] (Smart w2, Minimized w2: the output layer), indices clipped to the sizes
  inf_bias     ordinary inputs; b1[0] = +Inf
  zero_column  columns 7 (shared) and 40 (swarm feature 6) of w1 are exact zeros; rows with r % 7 == 3 hold +Inf in column 7, == 5 in column 40:
               torch's Inf * 0 = NaN in every hidden unit
  absorbed     columns 9 (shared) and 41 (swarm feature 7) of w1 are positive in every unit; rows with r % 7 == 3 hold -Inf in column 9, == 5 in
               column 41: every hidden unit is -Inf before the ReLU and an exact 0 after it, so Q is finite and the same in all of these rows -- while a
               padded hidden unit's accumulator is 0 + (-Inf) * 0 = NaN.  The sharpest check that padding is not visible: a damaged row with a finite Q
A row is a row of x in the expanded layout and an env in the compact ones.  The two-seat layout has two different weight sets; the damaged set of
nan_weight / inf_bias / zero_column / absorbed is seat 1's, whose inputs alone carry zero_column's and absorbed's Inf, and nonfinite alternates the damaged seat."""
import numpy as np

import minimized_model as mm
import qnet_model as qm
from replay_model import ReplayModel

SEED = 0x9E3779B97F4A7C15   # the sample seed: both words of the Philox key non-zero and different (as tests/off_default_cases.py)

# ------------------------------------------------------------------------------------------------------------------ Q networks
SMART_HIDDEN = [(60, 60), (17, 64), (1, 1)]      # the reference's sizes; a padded first layer under a full second one; the smallest
MINI_HIDDEN = [(80,), (128,), (17,), (1,)]       # the reference's size; every tile full; one unit into the second tile; the smallest
FAMILIES = ["signed", "subnormal", "overflow", "nonfinite", "nan_weight", "inf_bias", "zero_column", "absorbed"]
WEIGHT_DAMAGE = ("nan_weight", "inf_bias", "zero_column", "absorbed")      # one weight set differs from an ordinary one
LAYOUTS = ["expanded", "compact", "seats"]
ROWS_EXPANDED = 437          # 27 groups of 16 and 5 rows: more than one workgroup, a partial last group, every r % 24 and r % 7 many times
ENVS_COMPACT = 85            # 5 groups and 5 envs; 1 020 expanded rows per model call (two calls for the two seats)
DAMAGE = {1: np.nan, 3: np.inf, 5: -np.inf}      # r % 7 -> the value of the damaged input
ZERO_COLUMNS = (7, 40)       # of w1: a shared feature and swarm feature 6
POSITIVE_COLUMNS = (9, 41)   # of w1: a shared feature and swarm feature 7
INF_COLUMNS = {"zero_column": (ZERO_COLUMNS, np.inf), "absorbed": (POSITIVE_COLUMNS, -np.inf)}


def _rng(*key):
    return np.random.default_rng([0x51ED] + [int(k) for k in key])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def net_params(kind, hidden, family, which=0, damaged=True):
    """The weight set number `which` of a family: Smart (w1, b1, w2, b2, w3, b3) for hidden (h1, h2), Minimized (w1, b1, w2, b2) for hidden (h1,)."""
    sizes = (59,) + tuple(hidden) + ((5,) if kind == "smart" else (11,))
    rng = _rng(1, FAMILIES.index(family), kind == "smart", which, *hidden)
    p = []
    for layer in range(len(sizes) - 1):
        w, b = rng.standard_normal((sizes[layer + 1], sizes[layer])), rng.standard_normal(sizes[layer + 1])
        if family == "subnormal":
            w, b = (w * 2.0 ** -88, b * 2.0 ** -128) if layer == 0 else (w * 0.3, b * 2.0 ** -130)
            if layer == 0:
                w[:, 47:] *= 2.0 ** -40          # the one-hot columns meet an input of 1, not of 2^-40: the compact layouts' VALU add is a subnormal add
        elif family == "overflow":
            w = w * 2.0 ** (80 if kind == "mini" and layer == 0 else 40)
        else:
            w, b = w * 0.3, b * 0.3
        p += [_f32(w), _f32(b)]
    if damaged and family == "nan_weight":
        w = p[2]
        w[min(3, w.shape[0] - 1), min(5, w.shape[1] - 1)] = np.nan
    if damaged and family == "inf_bias":
        p[1][0] = np.inf
    if damaged and family == "zero_column":
        p[0][:, list(ZERO_COLUMNS)] = 0.0
    if damaged and family == "absorbed":
        p[0][:, list(POSITIVE_COLUMNS)] = np.abs(p[0][:, list(POSITIVE_COLUMNS)])
    return tuple(p)


def row_scale(family, rows):
    r = np.arange(rows)
    if family == "subnormal":
        return np.full(rows, 2.0 ** -40)
    if family == "overflow":
        return 2.0 ** (3.0 * (r % 24) - 12.0)
    return np.ones(rows)


def expanded_inputs(family, rows=ROWS_EXPANDED):
    """x [rows, 59]: any 59 floats per row (the expanded layout does not ask for a one-hot tail)."""
    x = _rng(2, FAMILIES.index(family), rows).standard_normal((rows, 59)) * row_scale(family, rows)[:, None]
    r = np.arange(rows)
    if family == "nonfinite":
        for m, v in DAMAGE.items():
            rr = r[r % 7 == m]
            x[rr, rr % 59] = v
    if family in INF_COLUMNS:
        cols, v = INF_COLUMNS[family]
        x[r % 7 == 3, cols[0]] = v
        x[r % 7 == 5, cols[1]] = v
    return _f32(x)


def compact_inputs(family, envs=ENVS_COMPACT, seats=1):
    """(shared [envs, 34], swarm [envs, 12, 13]) or, for seats = 2, ([envs, 2, 34], [envs, 2, 12, 13]).  Env r's damaged input (nonfinite) is column
    r % 47 of its 47 inputs -- below 34 a shared feature, which reaches all 12 swarms, else feature r % 47 - 34 of swarm r % 12, which reaches that swarm
    alone -- on seat (r // 7) % 2 of the two; zero_column's and absorbed's Inf go to seat 1 only (seat 0's weight set is undamaged)."""
    rng = _rng(3, FAMILIES.index(family), envs, seats)
    sc = row_scale(family, envs)
    shared = rng.standard_normal((envs, seats, 34)) * sc[:, None, None]
    swarm = rng.standard_normal((envs, seats, 12, 13)) * sc[:, None, None, None]
    for r in range(envs):
        if family == "nonfinite" and r % 7 in DAMAGE:
            c, p = r % 47, (r // 7) % seats
            if c < 34:
                shared[r, p, c] = DAMAGE[r % 7]
            else:
                swarm[r, p, r % 12, c - 34] = DAMAGE[r % 7]
        if family in INF_COLUMNS and r % 7 == 3:
            shared[r, seats - 1, INF_COLUMNS[family][0][0]] = INF_COLUMNS[family][1]
        if family in INF_COLUMNS and r % 7 == 5:
            swarm[r, seats - 1, r % 12, INF_COLUMNS[family][0][1] - 34] = INF_COLUMNS[family][1]
    if seats == 1:
        shared, swarm = shared[:, 0], swarm[:, 0]
    return _f32(shared), _f32(swarm)


def damaged_rows(family, rows):
    """bool [rows]: the rows (envs) that carry a non-finite input"""
    r = np.arange(rows)
    if family == "nonfinite":
        return np.isin(r % 7, list(DAMAGE))
    if family in INF_COLUMNS:
        return np.isin(r % 7, (3, 5))
    return np.zeros(rows, bool)


def seat_params(kind, hidden, family):
    """the two weight sets of the two-seat layout: seat 0's undamaged, seat 1's the family's damaged one"""
    return net_params(kind, hidden, family, 0, damaged=False), net_params(kind, hidden, family, 1, damaged=True)


def _model(kind):
    return qm if kind == "smart" else mm


def model_q(kind, layout, params, inputs, final_relu, chunk=2048):
    """The host model's Q for one layout, at most `chunk` expanded rows per model call.  params: one set, or the two of the two-seat layout."""
    m = _model(kind)
    if layout == "expanded":
        x = inputs
        return np.concatenate([m.forward(x[lo:lo + chunk], params, final_relu) for lo in range(0, x.shape[0], chunk)])
    shared, swarm = inputs
    if layout == "seats":
        return np.stack([model_q(kind, "compact", params[p], (shared[:, p], swarm[:, p]), final_relu, chunk) for p in range(2)], 1)
    step = max(1, chunk // 12)
    return np.concatenate([m.forward_compact(shared[lo:lo + step], swarm[lo:lo + step], params, final_relu) for lo in range(0, shared.shape[0], step)])


def case(kind, hidden, family, layout):
    """(params, inputs) of one Q-network case"""
    if layout == "expanded":
        return net_params(kind, hidden, family), expanded_inputs(family)
    if layout == "compact":
        return net_params(kind, hidden, family), compact_inputs(family)
    return seat_params(kind, hidden, family), compact_inputs(family, seats=2)


def first_hidden(params, x):
    """the first hidden layer (after the ReLU) of expanded rows x"""
    return qm.layer(x, params[0], params[1], True)


def is_subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < np.finfo(np.float32).tiny)


def same_values(got, want):
    """The contract's comparison: equal NaN masks, equal values elsewhere (the sign of a zero is not part of it)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True)


# the Minimized kernel's second sweep: its grid is capped at 2 workgroups per CU, of 4 wavefronts x 16 rows
def sweep_rows(cus):
    """one full sweep of the capped grid, one more full group and one row short of another"""
    return 16 * 4 * 2 * cus + 17


def sweep_checked_rows(rows, cus):
    """the rows compared with the host model: the first group, the 96 rows around the sweep boundary, the last 33 rows and 1 024 random rows"""
    edge = 16 * 4 * 2 * cus
    pick = np.concatenate([np.arange(16), np.arange(edge - 48, edge + 48), np.arange(rows - 33, rows), _rng(4, rows).choice(rows, 1024, replace=False)])
    return np.unique(pick[(pick >= 0) & (pick < rows)])


# ------------------------------------------------------------------------------------------------------------------ replay memory
SHAPINGS = ["custom", "basic_reward", "normalized_score", ("transition", "basic_reward", "penalize_long_games", 2)]
RING = [(7, 6, 1.0), (5, 3, 0.0), (9, 4, 0.999)]             # (H, n, gamma): n = H - 1 with gamma 1, gamma 0, an ordinary one
SEAT_FORMS = [1, (0, 1)]
P_DONE = 0.15


class ReplayCase(object):
    def __init__(self, name, N, seats, H, n, gamma, shaping, auto_reset=True, turns=None, quiet=(), checks=None, per_turn=True):
        self.name, self.N, self.seats, self.H, self.n, self.gamma, self.shaping, self.auto_reset = name, N, seats, H, n, gamma, shaping, auto_reset
        self.S = 2 if seats == (0, 1) else 1
        self.seat = 0 if self.S == 2 else int(seats)
        self.turns = 3 * (H + 1) + 5 if turns is None else turns
        self.quiet = quiet                                   # env ranges whose rows all have direction 0: records without transitions
        sl = H + 1
        # three check turns: before the ring wraps, after one wrap, and the last turn (after two wraps where the turns allow)
        self.checks = (sl - 1, 2 * sl + 1, self.turns - 1) if checks is None else checks
        self.per_turn = per_turn                             # compare the metadata after every turn (else at the check turns only)
        self.key = [5, N, self.S, self.seat, H, n, SHAPINGS.index(shaping) if shaping in SHAPINGS else 9, int(auto_reset)]

    def __repr__(self):
        return self.name

    def features(self, t):
        """record t's features (shared [N, S, 34], swarm [N, S, 12, 13]), squeezed for one seat"""
        rng = _rng(*(self.key + [0, t]))
        sh, sw = _f32(rng.standard_normal((self.N, self.S, 34))), _f32(rng.standard_normal((self.N, self.S, 12, 13)))
        return (sh, sw) if self.S == 2 else (sh[:, 0], sw[:, 0])

    def turn(self, t):
        """turn t's step outputs: directions int32 [N, S, 7, 2] (swarm in -1..12: out of range and repeated; direction in 0..5, all 0 for a
        quarter of the records), reward float32 [N, 2]
        (halves, so that ties occur), done uint8 [N], custom float32 [N, S] ~ N(0, 3^2)"""
        rng = _rng(*(self.key + [1, t]))
        N, S = self.N, self.S
        dirs = np.stack([rng.integers(-1, 13, (N, S, 7)), rng.integers(0, 6, (N, S, 7))], -1).astype(np.int32)
        dirs[rng.random((N, S)) < 0.25, :, 1] = 0            # an idle seat: a record without transitions
        for lo, hi in self.quiet:
            dirs[lo:hi, :, :, 1] = 0
        reward = _f32(np.round(rng.standard_normal((N, 2)) * 2.0) / 2.0)
        done = (rng.random(N) < P_DONE).astype(np.uint8)
        if not self.auto_reset and t == self.turns - 4:
            done[:] = 1                                      # whoever still plays ends here: every env is frozen by the last turn
        custom = _f32(rng.standard_normal((N, S)) * 3.0)
        return (dirs if S == 2 else dirs[:, 0]), reward, done, (custom if S == 2 else custom[:, 0])

    def model(self):
        return ReplayModel(self.N, self.S, self.H, self.n, self.gamma, self.shaping, seat=self.seat, episode_base=0, auto_reset=self.auto_reset)

    def run_model(self, upto=None, on_turn=None):
        """the host model after turns 0 .. upto - 1 of the synthetic driver; on_turn(t, model) after each"""
        m = self.model()
        for t in range(self.turns if upto is None else upto):
            dirs, reward, done, custom = self.turn(t)
            m.record(dirs, reward, done, custom if self.shaping == "custom" else None)
            if on_turn is not None:
                on_turn(t, m)
        return m


def _shape_name(s):
    return s if isinstance(s, str) else "transition"


REPLAY_GRID = [ReplayCase("seats%s-H%d-n%d-%s" % ("01" if seats == (0, 1) else "1", H, n, _shape_name(shaping)), 37, seats, H, n, gamma, shaping)
               for seats in SEAT_FORMS for (H, n, gamma) in RING for shaping in SHAPINGS]
REPLAY_FROZEN = [ReplayCase("frozen-seats%s" % ("01" if seats == (0, 1) else "1"), 37, seats, 9, 4, 0.9, "custom", auto_reset=False, checks=(4, 12, 20))
                 for seats in SEAT_FORMS]
# A ring past 256 scan blocks of 1 024 records: R = 17 * 8 201 * 2 = 278 834 records = 273 blocks (the last one partial, R mod 4 = 2), two block sums per
# thread of the top kernel.  Envs 1 000 .. 3 100 never act (4 202 consecutive empty records in every slot: at least three whole empty blocks), nor do the
# last 600 envs (the trailing blocks of the last slot); after turn 16 the ring's slot 0 has just been emptied (the first 16 blocks).
BIG_N = 8201
REPLAY_BIG = ReplayCase("big-ring", BIG_N, (0, 1), 16, 3, 0.99, "custom", turns=29, quiet=((1000, 3101), (BIG_N - 600, BIG_N)), checks=(10, 16, 28),
                        per_turn=False)
SCAN_BLOCK = 1024
SAMPLE_SIZES = (1, 257, 4099)


def empty_blocks(model):
    """bool per scan block of 1 024 records (ring order): no transition in it"""
    c = model.count.reshape(-1).astype(np.int64)
    nb = (len(c) + SCAN_BLOCK - 1) // SCAN_BLOCK
    sums = np.add.reduceat(c, np.arange(nb) * SCAN_BLOCK)
    return sums == 0


def longest_run(mask):
    best = run = 0
    for v in mask:
        run = run + 1 if v else 0
        best = max(best, run)
    return best
