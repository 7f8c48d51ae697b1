"""Operands for the tests of the learner step's glue (tests/learner_model.py, include/evg_learn.h), shared by the CPU and the GPU tests.

  td_exact(B, OUT, mode, weighted, done)   the exact tier: small integers and powers of two the model's exact mode accepts
  td_random(B, OUT, mode, weighted)        the random tier
  adam_shapes(kind, hidden)                the parameter shapes of a network"""
import numpy as np

BATCHES = (1, 15, 16, 17, 63, 64, 65, 259, 4099)
OUTS = (5, 11)
TDS = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 3.0, -3.0], np.float32)
EXACT_SCALE = 0.5
GARBAGE = np.array([np.nan, np.inf, -np.inf, 1e30, -7.0], np.float32)


def td_exact(B, OUT, mode, weighted, done="alternating", seed=0):
    """Every swarm value v is 12 k, k in -2..3, so that the mean is an integer; scale 0.5, rewards multiples of 0.5, q_pred[b][action] = estimated +
    one of TDS (every one of them taken when B >= 7).  q_next holds its maximum twice per swarm.  In the double mode q_select takes its maximum at two
    indices i < j: q_next[i] = v, q_next[j] = v + 7 (the last-index rule would show), and another q_next entry is larger than both (the plain maximum
    would show).  Rows that are done hold GARBAGE in q_next and q_select."""
    r = np.random.default_rng([seed, B, OUT, len(mode)])
    k = r.integers(-2, 4, (B, 12))
    v = (12 * k).astype(np.float32)
    q_next = v[:, :, None] - r.integers(1, 6, (B, 12, OUT)).astype(np.float32)
    i = r.integers(0, OUT - 1, (B, 12))
    j = i + 1 + r.integers(0, OUT, (B, 12)) % (OUT - 1 - i)
    bi, si = np.meshgrid(np.arange(B), np.arange(12), indexing="ij")
    q_select = None
    if mode == "double_mean":
        q_select = r.integers(-5, 3, (B, 12, OUT)).astype(np.float32)
        q_select[bi, si, i] = 4.0
        q_select[bi, si, j] = 4.0
        q_next[bi, si, i] = v
        q_next[bi, si, j] = v + 7
        other = (j + 1) % OUT
        other = np.where(other == i, (other + 1) % OUT, other)
        other = np.where(other == j, (other + 1) % OUT, other)
        q_next[bi, si, other] = v + 9                        # (OUT >= 5: a third index always exists)
        q_select[bi, si, other] = -6.0
    else:
        q_next[bi, si, i] = v
        q_next[bi, si, j] = v                                # a tie in the maximum
    not_done = {"none": np.ones(B, bool), "all": np.zeros(B, bool), "alternating": np.arange(B) % 2 == 0}[done]
    future = (v.max(1) if mode == "max_max" else v.sum(1) / 12.0) * not_done
    reward = (r.integers(-4, 5, B) * 0.5).astype(np.float32)
    est = (future * EXACT_SCALE + reward).astype(np.float32)
    action = r.integers(0, OUT, B).astype(np.int64)
    q_pred = r.integers(-9, 10, (B, OUT)).astype(np.float32)
    q_pred[np.arange(B), action] = est + TDS[np.arange(B) % len(TDS)]
    g = GARBAGE[r.integers(0, len(GARBAGE), (B, 12, OUT))]
    q_next = np.where(not_done[:, None, None], q_next, g).astype(np.float32)
    if q_select is not None:
        q_select = np.where(not_done[:, None, None], q_select, g[:, :, ::-1]).astype(np.float32)
    weights = (2.0 ** r.integers(-2, 2, B)).astype(np.float32) if weighted else None
    return dict(q_pred=q_pred, action=action, q_next=q_next, q_select=q_select, reward=reward, not_done=not_done, weights=weights, scale=EXACT_SCALE,
                mode=mode)


def td_random(B, OUT, mode, weighted, seed=1):
    r = np.random.default_rng([seed, B, OUT, len(mode)])
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    return dict(q_pred=f(B, OUT) * 2, action=r.integers(0, OUT, B).astype(np.int64), q_next=f(B, 12, OUT) * 2,
                q_select=f(B, 12, OUT) if mode == "double_mean" else None, reward=f(B), not_done=r.random(B) < 0.8,
                weights=(0.1 + 0.9 * r.random(B)).astype(np.float32) if weighted else None, scale=np.float32(0.999 ** 3), mode=mode)


SMART_HIDDEN = ((1, 1), (3, 3), (60, 60), (64, 64))
MINI_HIDDEN = (1, 80, 128)
ADAM_NETS = [("smart", h) for h in SMART_HIDDEN] + [("mini", (h,)) for h in MINI_HIDDEN]
ADAM_IDS = ["%s-%s" % (k, "x".join(map(str, h))) for k, h in ADAM_NETS]


def adam_shapes(kind, hidden):
    if kind == "smart":
        h1, h2 = hidden
        return [(h1, 59), (h1,), (h2, h1), (h2,), (5, h2), (5,)]
    h1, = hidden
    return [(h1, 59), (h1,), (11, h1), (11,)]


def adam_case(kind, hidden, seed=0, grad_scale=1.0):
    """(params, a function step -> grads): fp32 arrays of the network's shapes"""
    r = np.random.default_rng([seed, len(kind)] + list(hidden))
    shapes = adam_shapes(kind, hidden)
    params = [(r.standard_normal(s) * 0.3).astype(np.float32) for s in shapes]
    grads = lambda step: [(np.random.default_rng([seed, step, i]).standard_normal(s) * grad_scale).astype(np.float32) for i, s in enumerate(shapes)]
    return params, grads


def within(got, want, bound):
    """(ok, worst |got - want| / bound) elementwise; a zero bound demands equality"""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return bool((err <= bound).all()), float(ratio.max()) if ratio.size else 0.0


def same_bits(a, b):
    """bit-equal fp32 values, the sign of a zero apart"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
