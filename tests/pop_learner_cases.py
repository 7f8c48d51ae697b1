"""What the CPU and the GPU tests of the population learner share (tests/test_pop_learner_model.py, tests/test_gpu_pop_learner.py): shapes, member ids
and teams of networks, built from the families of tests/qnet_grad_cases.py and the operands of tests/learner_cases.py."""
import numpy as np

import qnet_grad_cases as gcases

BATCHES = (1, 15, 16, 17, 257, 4099)                   # 257 and 4 099 cross the bucket pass's 256-row blocks
TEAMS = (1, 4, 16)
HIDDEN = {"smart": ((60, 60), (33, 17)), "mini": ((80,), (33,))}       # the defaults and one padded pair
OUT = gcases.OUT
NOBODY = 255
# (B, K) of the stage tiers: every B and every K once, 4 099 with two members (about 32 workgroups each)
SHAPES = ((1, 1), (15, 4), (16, 16), (17, 4), (257, 16), (257, 4), (4099, 2))


def ids(B, K, how="random", seed=0, nobody=0.0):
    """member ids uint8 [B]: 'random', 'descending', 'interleaved' (b % K), 'first' (all rows to member 0), 'one' (member K - 1 has exactly one row);
    a fraction `nobody` of the rows gets an id >= K (255, or K itself)"""
    r = np.random.default_rng([seed, B, K, len(how)])
    if how == "random":
        a = r.integers(0, K, B)
    elif how == "descending":
        a = np.sort(r.integers(0, K, B))[::-1]
    elif how == "interleaved":
        a = np.arange(B) % K
    elif how == "first":
        a = np.zeros(B, np.int64)
    elif how == "one":
        a = r.integers(0, max(K - 1, 1), B)
        a[B // 2] = K - 1
    else:
        raise ValueError(how)
    a = a.astype(np.uint8)
    if nobody:
        drop = r.random(B) < nobody
        a[drop] = np.where(r.random(int(drop.sum())) < 0.5, NOBODY, K).astype(np.uint8)
    return np.ascontiguousarray(a)


def exact_team(kind, hidden, K):
    """member m's parameters: the integer family's for even m, the permutation family's for odd m (both exact on the integer family's inputs)"""
    return [gcases.params(kind, hidden, ("integer", "permutation")[m % 2]) for m in range(K)]


def random_team(kind, hidden, K, family="dense", seed=0):
    """the family's parameters, each member's scaled and shifted a little so that no two members are one network"""
    base = gcases.params(kind, hidden, family)
    team = []
    for m in range(K):
        r = np.random.default_rng([seed, m, K])
        team.append(tuple(np.ascontiguousarray(p * np.float32(1.0 + 0.05 * m) + (r.standard_normal(p.shape) * 0.02).astype(np.float32), np.float32)
                          for p in base))
    return team


def final_relu(kind):
    """the reference's QNetwork of the Minimized family ends in a ReLU, Smart_State's does not"""
    return kind in ("mini", "minimized")
