"""Host model of the learner step's glue (include/evg_learn.h): evg_td_head and evg_adam_step in numpy, each twice -- in the header's fp32 operation
order (bit for bit what the device computes) and in float64 with a counted bound E on |device - float64 model|.

  td_head(...)  -> dict(estimated, td, term, gq, priorities, loss) in float64 and dict of the same keys' bounds
  td_head32(...)-> the same values in the header's fp32 order, the loss summed in the header's order
  adam(...)     -> (param, m, v, (step, p1, p2)) in float64 and the bounds (E_param, E_m, E_v)
  adam32(...)   -> the same in the header's fp32 order

u = 2^-24 is the relative error of one correctly rounded fp32 operation.  Nothing here looks at a device result: every c below is counted.

The TD head's bound, per sample, with F = (sum_s |v[s]|) / 12 for the mean modes and max_s |v[s]| for max_max (0 where done), and
M = |q_pred[b][action]| + |reward| + scale * F the magnitude everything on the path is bounded by:

    future     mean modes: 11 additions and one division, c_f = 12; max_max: a maximum rounds nothing, c_f = 0.  Selecting (max, first argmax of
               q_select) compares exactly.
    estimated  one fmaf: c_f + 1                                                    E_est  = (c_f + 1) u M
    td         one subtraction: c_f + 2                                             E_td   = (c_f + 2) u M
    priority   |.| is exact, one addition of 1e-5f: c_f + 3                         E_prio = (c_f + 3) u (M + 1e-5)
    gq         the clamp is exact and 1-Lipschitz, one multiplication by w, one division by B: c_f + 4
                                                                                    E_gq   = (c_f + 4) u w M / B
    term       the Huber term is 1-Lipschitz in td (so the branch the device takes from ITS td costs no more than E_td, |td| near 1 included), its
               own operations round at most twice (0.5f * td is exact), w once:     E_term = w (E_td + 3 u term)
    loss       B - 1 additions in any order and one division:                       E_loss = (sum_b E_term_b + B u sum_b w term_b) / B

First-order in u, as tests/qnet_grad_model.py: a sum of c roundings is bounded by c u M without the second-order term (Jeannerod and Rump 2013); the
products of two rounded factors here add a relative u^2, which the factor (1 + 2^-20) on every E covers.

exact=True is for the test tier whose device result must be bit-equal: it asserts that nothing on the path can round in fp32 -- the 12-term sum is a
multiple of 3 * 2^e that divides by 12 exactly, estimated / td / term / w * term / the sum over b are fp32 values as computed in float64 -- so that the
float64 values ARE the device's, except gq and loss, whose single correctly rounded division by B is then taken in fp32 from the exact numerator, and
the priorities, whose single addition of 1e-5f is taken in fp32 from the exact |td|.

Adam's bound, per element (d = g - m, t = step_size * m' / den; the double-precision bias corrections cost one rounding each when converted):

    m'   subtraction, 1 - beta1, product, addition:  E_m = u (3 |d| (1 - beta1) + |m'|)
    v'   beta2 v: 1; (omb2 g) g: omb2, two products: 3; their sum (both >= 0): 1.  E_v = 4 u v' + 3 * 2^-149 (an underflowing g^2)
    den  sqrt halves 4 u and adds 1: 3; bc2s 1, the division 1, + eps (both >= 0) 1: 6.  sqrt(v' + dv) <= sqrt(v') + sqrt(dv) turns the underflow
         floor into FLOOR = sqrt(3 * 2^-149) / bc2s
    p'   E_p = u (|p'| + 9 |t| + step_size E_m / (u den)) + |t| FLOOR / den         (m' / den: 1, step_size: 1, the product: 1, 6 from den: 9)
"""
import numpy as np

import qnet_model

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
F32 = np.float32
MODES = ("max_mean", "max_max", "double_mean")
MAX_BLOCKS, SLOTS = 1024, 16                                # EVG_TD_HEAD_MAX_BLOCKS, samples per workgroup and sweep


def _swarm_values(q_next, q_select, mode):
    """v [B, 12] (the dtype of q_next): the swarm's value, selected exactly"""
    if mode == "double_mean":
        idx = np.argmax(q_select, axis=2)                   # numpy's argmax returns the first index of the maximum
        return np.take_along_axis(q_next, idx[:, :, None], axis=2)[:, :, 0]
    return q_next.max(axis=2)


def _is32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a.astype(F32).astype(np.float64), a)


def td_head(q_pred, action, q_next, q_select, reward, not_done, weights, scale, mode, exact=False, drop_sample=None):
    """float64 values and bounds.  Operands are fp32 arrays (action int64, not_done bool); scale is taken as its fp32 value."""
    assert mode in MODES
    q_pred, q_next, reward = (np.asarray(a, F32).astype(np.float64) for a in (q_pred, q_next, reward))
    action, not_done = np.asarray(action, np.int64), np.asarray(not_done).astype(bool)
    B, OUT = q_pred.shape
    scale = float(F32(scale))
    w = np.ones(B) if weights is None else np.asarray(weights, F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = _swarm_values(np.where(not_done[:, None, None], q_next, 0.0),
                          None if q_select is None else np.where(not_done[:, None, None], np.asarray(q_select, F32).astype(np.float64), 0.0), mode)
    if mode == "max_max":
        future, Fm, cf = v.max(1), np.abs(v).max(1), 0
    else:
        future, Fm, cf = v.sum(1) / 12.0, np.abs(v).sum(1) / 12.0, 12
    future, Fm = np.where(not_done, future, 0.0), np.where(not_done, Fm, 0.0)
    est = future * scale + reward
    valid = (action >= 0) & (action < OUT)
    qa = np.where(valid, q_pred[np.arange(B), np.clip(action, 0, OUT - 1)], 0.0)
    td = np.where(valid, qa - est, 0.0)
    ad = np.abs(td)
    term = np.where(ad < 1.0, 0.5 * td * td, ad - 0.5)
    wterm = w * term
    num = w * np.clip(td, -1.0, 1.0)
    if drop_sample is not None:
        wterm[drop_sample] = 0.0
        num[drop_sample] = 0.0
    gq = np.zeros((B, OUT))
    gq[np.arange(B)[valid], action[valid]] = num[valid] / B
    prio = ad + float(F32(1e-5))
    loss = wterm.sum() / B
    M = np.where(valid, np.abs(qa), 0.0) + np.abs(reward) + scale * Fm
    E_td = np.where(valid, (cf + 2) * U * M, 0.0)
    E_term = w * (E_td + 3 * U * term)
    bounds = {"estimated": (cf + 1) * U * M * SLACK, "td": E_td * SLACK, "priorities": np.where(valid, (cf + 3) * U * (M + 1e-5), 0.0) * SLACK,
              "gq": np.zeros((B, OUT)), "loss": (E_term.sum() + B * U * np.abs(wterm).sum()) / B * SLACK}
    bounds["gq"][np.arange(B)[valid], action[valid]] = ((cf + 4) * U * w * M / B * SLACK)[valid]
    out = {"estimated": est, "td": td, "term": term, "gq": gq, "priorities": prio, "loss": loss}
    if exact:
        if mode != "max_max":
            s = v.sum(1)
            assert _is32(s) and _is32(future) and all(_is32(np.cumsum(v, axis=1)[:, k]) for k in range(12)), "the sum over the swarms may round in fp32"
        for name, a in (("estimated", est), ("td", td), ("term", term), ("w * term", wterm), ("w * clamp(td)", num)):
            assert _is32(a), "%s is not an fp32 value: the path may round" % name
        out["priorities"] = (ad.astype(F32) + F32(1e-5)).astype(F32)       # one rounding of exact operands
        assert _is32(0.5 * td) and _is32(np.abs(wterm).sum()) and np.abs(wterm).sum() < 2.0 ** 24 * _lowest_unit(wterm), "the sum over the batch may round"
        out["gq"] = (gq * B).astype(F32) / F32(B)           # the one rounding: a correctly rounded fp32 division of exact numerators
        out["loss"] = F32(wterm.sum()) / F32(B)
    return out, bounds


def _lowest_unit(a):
    """the largest power of two every element of a is a multiple of (1.0 for all zeros)"""
    a = np.abs(np.asarray(a, np.float64))
    a = a[a > 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    return float(2.0 ** (e + np.log2((mi & -mi).astype(np.float64)) - 53).min())


def loss_order32(wterm, B):
    """sum of the fp32 wterm [B] in the header's order, divided by B: workgroup g of G takes the 16-sample groups g, g + G, ...; a slot (b % 16) adds its
    samples ascending, the workgroup its 16 slots ascending; lane l adds the partials l, l + 64, ...; the 64 lanes ascending"""
    wterm = np.asarray(wterm, F32)
    chunks = (B + SLOTS - 1) // SLOTS
    G = min(chunks, MAX_BLOCKS)
    pad = np.zeros(chunks * SLOTS, F32)
    pad[:B] = wterm
    pad = pad.reshape(chunks, SLOTS)
    partial = np.zeros(G, F32)
    for g in range(G):
        acc = np.zeros(SLOTS, F32)
        for c in range(g, chunks, G):
            live = np.arange(SLOTS) + c * SLOTS < B
            acc = np.where(live, acc + pad[c], acc).astype(F32)
        s = acc[0]
        for k in range(1, SLOTS):
            s = F32(s + acc[k])
        partial[g] = s
    lanes = np.zeros(64, F32)
    for l in range(64):
        s = F32(0.0)
        for i in range(l, G, 64):
            s = F32(s + partial[i])
        lanes[l] = s
    t = lanes[0]
    for k in range(1, 64):
        t = F32(t + lanes[k])
    return F32(t / F32(B))


def td_head32(q_pred, action, q_next, q_select, reward, not_done, weights, scale, mode):
    """the header's fp32 operation order, every statement one fp32 operation"""
    assert mode in MODES
    q_pred, q_next, reward = (np.asarray(a, F32) for a in (q_pred, q_next, reward))
    action, not_done = np.asarray(action, np.int64), np.asarray(not_done).astype(bool)
    B, OUT = q_pred.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v = _swarm_values(q_next, None if q_select is None else np.asarray(q_select, F32), mode)
        if mode == "max_max":
            future = v.max(1)
        else:
            future = v[:, 0]
            for s in range(1, 12):
                future = (future + v[:, s]).astype(F32)
            future = (future / F32(12.0)).astype(F32)
    future = np.where(not_done, future, F32(0.0)).astype(F32)
    est = qnet_model.fmaf32(future, np.full(B, F32(scale), F32), reward).astype(F32)
    valid = (action >= 0) & (action < OUT)
    qa = q_pred[np.arange(B), np.clip(action, 0, OUT - 1)]
    td = np.where(valid, (qa - est).astype(F32), F32(0.0)).astype(F32)
    ad = np.abs(td)
    term = np.where(ad < 1.0, ((F32(0.5) * td).astype(F32) * td).astype(F32), (ad - F32(0.5)).astype(F32)).astype(F32)
    g = np.clip(td, F32(-1.0), F32(1.0)).astype(F32)
    if weights is not None:
        w = np.asarray(weights, F32)
        term = (w * term).astype(F32)
        g = (w * g).astype(F32)
    g = (g / F32(B)).astype(F32)
    gq = np.zeros((B, OUT), F32)
    gq[np.arange(B)[valid], action[valid]] = g[valid]
    return {"estimated": est, "td": td, "term": term, "gq": gq, "priorities": (ad + F32(1e-5)).astype(F32), "loss": loss_order32(term, B)}


# ---------------------------------------------------------------------- Adam
def new_ctl():
    return (0, 1.0, 1.0)


def adam(params, grads, m, v, ctl, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, clamp=0.0, fresh=False):
    """One step in float64 over lists of arrays; lr, betas, eps are used as given (hand it the fp32 values to model the device).
    -> (params', m', v', ctl'), (E_param, E_m, E_v) elementwise."""
    b1, b2 = float(betas[0]), float(betas[1])
    step, p1, p2 = new_ctl() if fresh else ctl
    p1, p2 = p1 * b1, p2 * b2
    step_size = float(lr) / (1.0 - p1)
    bc2s = np.sqrt(1.0 - p2)
    floor = np.sqrt(3 * 2.0 ** -149) / bc2s
    P, Mo, V, EP, EM, EV = [], [], [], [], [], []
    for p, g, m0, v0 in zip(params, grads, m, v):
        p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
        m0 = np.zeros_like(p) if fresh else np.asarray(m0, np.float64)
        v0 = np.zeros_like(p) if fresh else np.asarray(v0, np.float64)
        if clamp:
            g = np.clip(g, -clamp, clamp)
        d = g - m0
        m1 = m0 + d * (1.0 - b1)
        v1 = b2 * v0 + (1.0 - b2) * g * g
        den = np.sqrt(v1) / bc2s + eps
        t = step_size * (m1 / den)
        p1_ = p - t
        Em = U * (3 * np.abs(d) * (1.0 - b1) + np.abs(m1))
        P.append(p1_), Mo.append(m1), V.append(v1)
        EM.append(Em * SLACK), EV.append((4 * U * v1 + 3 * 2.0 ** -149) * SLACK)
        EP.append((U * (np.abs(p1_) + 9 * np.abs(t)) + step_size * Em / den + np.abs(t) * floor / den) * SLACK)
    return (P, Mo, V, (step + 1, p1, p2)), (EP, EM, EV)


def adam32(params, grads, m, v, ctl, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, clamp=0.0, fresh=False):
    """the header's fp32 order; ctl's products stay Python floats (double)"""
    lr, b1, b2, eps, clamp = F32(lr), F32(betas[0]), F32(betas[1]), F32(eps), F32(clamp)
    step, p1, p2 = new_ctl() if fresh else ctl
    p1, p2 = p1 * float(b1), p2 * float(b2)
    step_size = F32(float(lr) / (1.0 - p1))
    bc2s = F32(np.sqrt(1.0 - p2))
    omb1, omb2 = F32(F32(1.0) - b1), F32(F32(1.0) - b2)
    P, Mo, V = [], [], []
    with np.errstate(under="ignore"):
        for p, g, m0, v0 in zip(params, grads, m, v):
            p, g = np.asarray(p, F32), np.asarray(g, F32)
            m0 = np.zeros_like(p) if fresh else np.asarray(m0, F32)
            v0 = np.zeros_like(p) if fresh else np.asarray(v0, F32)
            if clamp > 0:
                g = np.clip(g, -clamp, clamp).astype(F32)
            m1 = (m0 + ((g - m0).astype(F32) * omb1).astype(F32)).astype(F32)
            v1 = ((b2 * v0).astype(F32) + ((omb2 * g).astype(F32) * g).astype(F32)).astype(F32)
            den = ((np.sqrt(v1).astype(F32) / bc2s).astype(F32) + eps).astype(F32)
            P.append((p - (step_size * (m1 / den).astype(F32)).astype(F32)).astype(F32)), Mo.append(m1), V.append(v1)
    return P, Mo, V, (step + 1, p1, p2)


def ctl_words(ctl):
    """the 32-byte control block of a (step, p1, p2) as int64 [4]"""
    a = np.zeros(4, np.int64)
    a[0] = ctl[0]
    a[1:3] = np.array([ctl[1], ctl[2]], np.float64).view(np.int64)
    return a


def ctl_from_words(words):
    w = np.asarray(words, np.int64)
    p = w[1:3].view(np.float64)
    return (int(w[0]), float(p[0]), float(p[1]))
