"""What the CPU and the GPU tests of the learner-step kernels past their grid caps share (tests/test_pop_learner_edge_cases.py,
tests/test_gpu_learner_step_edges.py): batch sizes, member ids and the grid arithmetic of include/evg_learn.h and include/evg_pop_learn.h restated on
the host, built from tests/learner_cases.py, tests/qnet_grad_cases.py and tests/pop_learner_cases.py.  No arithmetic model lives here.

The TD head (evg_learn_td_head_kernel, evg_poplearn_td_head_kernel) walks its samples in chunks of 16 over at most TD_MAX_BLOCKS = 1 024 workgroups:
below 16 385 rows every workgroup takes one chunk.
  PLAIN_BATCHES    16 384 (chunks == the cap, one pass), 16 385 (workgroup 0 alone takes a second chunk, of one live row), 2 * 16 384 + 19 (every
                   workgroup takes two chunks, two take a third, the last of them holds 3 rows)
  PLAIN_TD         (B, OUT, mode, weighted): every B twice, both OUT, the three modes, weights absent and present
The grouped kernels read member lists.  One id vector of BIG_B = 2 * EVG_QNET_GRAD_MAX_BLOCKS * 64 + 19 = 65 555 rows serves the grouped TD head and
the grouped backward:
  COUNTS_A         K = 3: 32 000 rows (2 000 chunks: G is capped, workgroups 0..975 take two chunks), 16 400 (1 025 chunks: workgroup 0 alone takes a
                   second), 16 384 (chunks == G); the other 771 rows belong to nobody (ids 255 and K mixed).  Arrangements "random" and "descending".
                   All three counts are multiples of 16, so no member's last chunk or last row group is partial, and 2 000 chunks are two passes, not
                   three.  COUNTS_FULL closes both gaps for the TD head:
  COUNTS_FULL      K = 3, no rows of nobody: 2 * 16 384 + 19 rows (2 050 chunks: two workgroups take a third, the last one holds 3 rows), 16 385 (the
                   second chunk of workgroup 0 holds one live row), 16 383 (the last chunk holds 15 rows).  Arrangement "random".
  counts_b()       K = 16 at BIG_B, found by a seeded search: sum_m ceil(X c_m / B) == X + K - 1 for X = 512, the documented maximum of the packed
                   partials; one member has a single row, one exactly 64, and the larger ones are no multiples of 16 (a partial last group on a
                   later pass of the backward's stride loop)
  td_signed()      the random tier's operands with weights of random sign: a loss whose fp32 bits depend on the order of the sum
  gathered_inputs()  the gathered family at BIG_B for the backward's random tier, x repeating with period 4 099
  adam_start_ctls(), ADAM_STEP_COUNTS   the grouped Adam stage: four different control blocks in one launch, five launches with changing counts
  Guarded, GuardedCtl   sentinel buffers around float32 tensors (tests/test_gpu_learner_step.py's) and around the int64 control blocks
"""
import numpy as np

import learner_cases as cases
import learner_model
import pop_learner_cases as pcases
import qnet_grad_cases as gcases

F32 = np.float32
SENTINEL = -7.5
TD_MAX_BLOCKS, TD_SLOTS = learner_model.MAX_BLOCKS, learner_model.SLOTS
TD_ONE_PASS = TD_MAX_BLOCKS * TD_SLOTS                  # 16 384 rows: the last batch size with one chunk per workgroup
GRAD_MAX_BLOCKS = 512                                   # EVG_QNET_GRAD_MAX_BLOCKS (the CPU test compares it with the binding's)
GRAD_ROWS_PER_BLOCK = 64                                # four wavefronts of one 16-row group
BIG_B = 2 * GRAD_MAX_BLOCKS * GRAD_ROWS_PER_BLOCK + 19  # 65 555

PLAIN_BATCHES = (TD_ONE_PASS, TD_ONE_PASS + 1, 2 * TD_ONE_PASS + 19)
PLAIN_TD = ((PLAIN_BATCHES[0], 5, "max_mean", False), (PLAIN_BATCHES[0], 11, "double_mean", True),
            (PLAIN_BATCHES[1], 11, "max_max", False), (PLAIN_BATCHES[1], 5, "double_mean", True),
            (PLAIN_BATCHES[2], 5, "max_max", True), (PLAIN_BATCHES[2], 11, "max_mean", False))
PLAIN_IDS = ["B%d-OUT%d-%s-%s" % (b, o, m, "weighted" if w else "plain") for b, o, m, w in PLAIN_TD]

K_A = 3
COUNTS_A = (32000, 16400, 16384)
COUNTS_FULL = (2 * TD_ONE_PASS + 19, TD_ONE_PASS + 1, TD_ONE_PASS - 1)
# (arrangement, OUT, mode, weighted) of the grouped TD head at BIG_B
GROUPED_TD = (("random", 5, "max_mean", True), ("random", 11, "double_mean", False), ("descending", 11, "max_max", True),
              ("descending", 5, "double_mean", True), ("full", 5, "max_max", False), ("full", 11, "max_mean", True))
GROUPED_IDS = ["%s-OUT%d-%s-%s" % (h, o, m, "weighted" if w else "plain") for h, o, m, w in GROUPED_TD]
KIND_OF_OUT = {5: "smart", 11: "mini"}

# (kind, hidden, final_relu) of the grouped backward past one sweep: both families, the defaults and the padded pair, the final ReLU on and off
BACKWARD_A = tuple((kind, hidden, fr) for kind in ("smart", "mini") for hidden in pcases.HIDDEN[kind] for fr in (False, True))
BACKWARD_B = (("smart", pcases.HIDDEN["smart"][0], False), ("smart", pcases.HIDDEN["smart"][1], True),
              ("mini", pcases.HIDDEN["mini"][0], True), ("mini", pcases.HIDDEN["mini"][1], False))


def backward_id(case):
    kind, hidden, fr = case
    return "%s-%s-%s" % (kind, "x".join(map(str, hidden)), "relu" if fr else "linear")


RANDOM_PERIOD = 4099


def gathered_inputs(kind, hidden, rows=BIG_B):
    """qnet_grad_cases' gathered family at `rows` rows (gq one non-zero per row, scaled by 1 / rows, every row its own), the rows of x repeating with
    period 4 099: the host model evaluates its forward in the fp32 order on the distinct rows only, which keeps the reference of 65 555 rows to a
    second or two.  Rows r and r + 4 099 carry other gq and mostly belong to other members, so no sum of the backward loses a term by it."""
    x, gq = gcases.inputs(kind, hidden, "gathered", rows)
    return np.ascontiguousarray(x[np.arange(rows) % RANDOM_PERIOD]), gq


K_B = 16
SEARCH_SEED = 0xB16


def ids_of_counts(counts, B, how="random", seed=0):
    """uint8 [B]: member m has counts[m] rows, the other rows belong to nobody (255 and K = len(counts), mixed); 'random': interleaved at random,
    'descending': the same counts in descending blocks (nobody's rows first, member 0's last)"""
    K = len(counts)
    r = np.random.default_rng([0xED6E, seed, B, K])
    rest = B - int(sum(counts))
    assert rest >= 0
    a = np.concatenate([np.full(c, m, np.int64) for m, c in enumerate(counts)] + [np.where(r.random(rest) < 0.5, pcases.NOBODY, K)])
    if how == "descending":
        a = np.sort(a, kind="stable")[::-1]
    elif how == "random":
        a = r.permutation(a)
    else:
        raise ValueError(how)
    return np.ascontiguousarray(a.astype(np.uint8))


def ids_a(how="random"):
    """the 65 555-row id vector of the grouped TD head and the grouped backward (COUNTS_A), or COUNTS_FULL's for how == 'full'"""
    if how == "full":
        return ids_of_counts(COUNTS_FULL, BIG_B, "random", seed=1)
    return ids_of_counts(COUNTS_A, BIG_B, how)


def td_signed(B, OUT, mode, seed=1):
    """learner_cases.td_random with weights whose signs are flipped at random: the loss is a sum that cancels, so its fp32 bits depend on the order of
    the additions -- with positive terms most orders round to the same float.  For the bit-equality with the fp32-order model alone: the counted
    bounds of learner_model.td_head are stated for weights >= 0."""
    c = cases.td_random(B, OUT, mode, True, seed)
    r = np.random.default_rng([0x516, seed, B, OUT])
    c["weights"] = (c["weights"] * r.choice([-1.0, 1.0], B)).astype(F32)
    return c


def counts_of(ids, K):
    return [int((np.asarray(ids) == m).sum()) for m in range(K)]


# ---------------------------------------------------------------------- the grids, as the headers state them
def td_chunks(rows):
    """(chunks, G) of the TD head for a batch (or a member's list) of `rows`"""
    chunks = -(-rows // TD_SLOTS)
    return chunks, min(chunks, TD_MAX_BLOCKS)


def td_passes(rows):
    """[number of workgroups that take p chunks for p = 0, 1, 2, ...]"""
    chunks, G = td_chunks(rows)
    per = [len(range(g, chunks, G)) for g in range(G)]
    return [per.count(p) for p in range(max(per) + 1)] if per else []


def grad_grid(B, cus=256):
    """X of include/evg_pop_learn.h: the plain backward's workgroups for B rows on a device of `cus` CUs (256: the MI355X, X at its cap)"""
    return min(-(-B // GRAD_ROWS_PER_BLOCK), 2 * cus, GRAD_MAX_BLOCKS)


def shares(counts, B, cus=256):
    """live_m = min(ceil(c_m / 64), ceil(X c_m / B)) for every member"""
    X = grad_grid(B, cus)
    return [min(-(-c // GRAD_ROWS_PER_BLOCK), -(-X * c // B)) for c in counts]


def needs(counts):
    return [-(-c // GRAD_ROWS_PER_BLOCK) for c in counts]


def group_passes(count, share):
    """[number of wavefronts of the member's share that run p group passes]: groups of 16 rows dealt over share * 4 wavefronts"""
    groups, stride = -(-count // 16), share * 4
    per = [len(range(w, groups, stride)) for w in range(stride)]
    return [per.count(p) for p in range(max(per) + 1)]


_COUNTS_B = {}


def counts_b(B=BIG_B, K=K_B, X=GRAD_MAX_BLOCKS, seed=SEARCH_SEED):
    """16 non-zero counts with sum_m ceil(X c_m / B) == X + K - 1.  ceil(X c / B) == j + 1 for every c in (j B / X, (j + 1) B / X], so the search
    draws j_0 + ... + j_(K-1) == X - 1 at random (a single row and exactly 64 rows are j == 0), gives member m a count just above j_m B / X, and
    keeps the first draw whose larger counts are no multiples of 16 and whose sum fits B; the rows left over belong to nobody."""
    key = (B, K, X, seed)
    if key not in _COUNTS_B:
        r = np.random.default_rng(seed)
        for _ in range(1000):
            cuts = np.sort(r.choice(np.arange(1, X - 1), K - 3, replace=False))
            j = np.diff(np.concatenate([[0], cuts, [X - 1]]))                  # K - 2 positive parts of X - 1
            big = [int(v) * B // X + 1 + int(r.integers(0, 3)) for v in j]
            counts = big[:5] + [1] + big[5:11] + [64] + big[11:]
            if sum(counts) <= B and all(c % 16 for c in big) and sum(-(-X * c // B) for c in counts) == X + K - 1:
                _COUNTS_B[key] = tuple(counts)
                break
        else:
            raise AssertionError("no counts found")
    return _COUNTS_B[key]


def ids_b():
    return ids_of_counts(counts_b(), BIG_B, "random", seed=2)


# ---------------------------------------------------------------------- grouped Adam as a stage
K_ADAM = 4
ADAM_NETS = (("smart", (60, 60)), ("mini", (80,)))
ADAM_STEP_COUNTS = ((5, 3, 7, 0), (1, 0, 2, 0), (9, 4, 0, 0), (2, 0, 6, 0), (3, 8, 1, 0))       # member 3 never has rows; the others' steps diverge


def adam_start_ctls(betas):
    """members 0..3: a new block, step 1 000 with consistent products, step 1, and one that must stay as it is"""
    b1, b2 = betas
    return [learner_model.new_ctl(), (1000, b1 ** 1000, b2 ** 1000), (1, b1, b2), (31, b1 ** 31, b2 ** 31)]


# ---------------------------------------------------------------------- sentinels
class Guarded(object):
    """a float32 tensor of `shape` inside a larger buffer of sentinels, 16 bytes from its start (tests/test_gpu_learner_step.py's)"""

    def __init__(self, env, shape, init=None):
        import torch
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 8 + (-self.n) % 4,), SENTINEL, dtype=torch.float32, device=env.device)
        self.t = self.buf[4:4 + self.n].view(shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init, F32)))

    def numpy(self):
        """the tensor's values; asserts the sentinels"""
        b = self.buf.cpu().numpy()
        assert (b[:4] == SENTINEL).all() and (b[4 + self.n:] == SENTINEL).all(), "a sentinel was overwritten"
        return b[4:4 + self.n].reshape(tuple(self.t.shape)).copy()


class GuardedCtl(object):
    """K control blocks of 32 bytes (int64 [K, 4]) with two sentinel words on each side"""
    WORD = -0x7A7A7A7A7A7A7A7A

    def __init__(self, env, ctls):
        import torch
        self.K = len(ctls)
        self.buf = torch.full((4 * self.K + 4,), self.WORD, dtype=torch.int64, device=env.device)
        self.t = self.buf[2:2 + 4 * self.K].view(self.K, 4)
        self.t.copy_(torch.from_numpy(np.stack([learner_model.ctl_words(c) for c in ctls])))

    def words(self):
        b = self.buf.cpu().numpy()
        assert (b[:2] == self.WORD).all() and (b[-2:] == self.WORD).all(), "a sentinel next to the control blocks was overwritten"
        return b[2:-2].reshape(self.K, 4).copy()

    def ctls(self):
        return [learner_model.ctl_from_words(w) for w in self.words()]
