"""Host model of the device Q network (everglades_amd.SmartQNet, include/evg.h evg_smart_qnet): the numerics contract restated in numpy.  Every
pre-activation is acc = b[j], then acc = fmaf(W[j][k], x[k], acc) for k ascending, then torch's ReLU (acc < 0 ? 0 : acc; np.maximum: a NaN stays
a NaN, the sign of a zero is not part of the contract) on the hidden layers (and on the output with final_relu).  The model has no padded units.  Python has no exact fp32 fma, so fmaf32 emulates it in float64: the product of two fp32 values is exact in float64, the sum is taken
with TwoSum, and the rounding to fp32 is settled by the TwoSum error where the float64 sum lies exactly halfway between two fp32 values."""
import numpy as np


def fmaf32(a, b, c):
    """Exactly rounded fp32 fma(a, b, c), elementwise, over the whole of fp32: subnormal operands and results, overflow to Inf, NaN, +-Inf, Inf * 0 and
    Inf - Inf (float64 carries all of them, and its double rounding through float64 is settled by the TwoSum error); tests/test_qnet_host.py compares it
    with libm's fmaf class by class."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                                          # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                     # TwoSum: p + c == s + e exactly
    r = s.astype(np.float32)
    rd = r.astype(np.float64)
    # the other fp32 neighbour of s (on s's side of r); s is a tie iff it lies exactly midway between r and it
    other = np.nextafter(r, np.where(s > rd, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    tie = (s != rd) & ((rd + other) * 0.5 == s) & (e != 0)
    # at a tie the exact value s + e lies on the side of e: pick the neighbour in that direction
    toward_other = tie & ((e > 0) == (other > rd))
    out = np.where(toward_other, other, rd).astype(np.float32)
    return out


def layer(x, w, b, relu):
    """x [R, K], w [H, K], b [H] -> [R, H] by the chain (k ascending)."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    acc = np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], w.shape[0])).copy()
    for k in range(w.shape[1]):
        acc = fmaf32(w[None, :, k], x[:, k:k + 1], acc)
    return np.maximum(acc, np.float32(0)) if relu else acc


def forward(x, params, final_relu):
    """Expanded rows x [..., 59] -> Q [..., 5]."""
    w1, b1, w2, b2, w3, b3 = params
    lead = x.shape[:-1]
    h = layer(np.asarray(x, np.float32).reshape(-1, 59), w1, b1, True)
    h = layer(h, w2, b2, True)
    return layer(h, w3, b3, bool(final_relu)).reshape(lead + (5,))


def forward_compact(shared, swarm, params, final_relu):
    """Compact features shared [N, 34], swarm [N, 12, 13] -> Q [N, 12, 5]: the chain prefix b1 + the 34 shared terms once per env, continued per
    swarm with the 13 swarm terms and the one-hot term acc + W1[j][47 + s]."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(t, np.float32) for t in params)
    shared = np.asarray(shared, np.float32)
    swarm = np.asarray(swarm, np.float32)
    N = shared.shape[0]
    pre = layer(shared, w1[:, :34], b1, False)                                   # [N, H1]
    acc = np.repeat(pre[:, None, :], 12, axis=1).reshape(N * 12, -1)
    sw = swarm.reshape(N * 12, 13)
    for k in range(13):
        acc = fmaf32(w1[None, :, 34 + k], sw[:, k:k + 1], acc)
    oh = w1[:, 47:59].T                                                           # [12, H1]
    acc = (acc.reshape(N, 12, -1) + oh[None]).astype(np.float32)                  # fp32 add == fmaf(w, 1, acc)
    h = np.maximum(acc.reshape(N * 12, -1), np.float32(0))
    h = layer(h, w2, b2, True)
    return layer(h, w3, b3, bool(final_relu)).reshape(N, 12, 5)


def expand(shared, swarm):
    """[N, 12, 59] = cat(shared, swarm[s], onehot(s))."""
    N = shared.shape[0]
    x = np.zeros((N, 12, 59), np.float32)
    x[:, :, :34] = shared[:, None, :]
    x[:, :, 34:47] = swarm
    x[:, np.arange(12), 47 + np.arange(12)] = 1.0
    return x
