"""Host model of the Q networks' backward pass (SmartQNet.with_grad / MinimizedQNet.with_grad, include/evg_qnet_grad.h): the contract in numpy.

  chain(x, params, final_relu)            -> ([x, a1, (a2)], q): the activations and the output of the exact fp32 fmaf chain (tests/qnet_model.py),
                                             computed once per distinct row of x
  backward(x, params, final_relu, gq)     -> (grads, E): the parameter gradients in float64, in the order of params (w1, b1, w2, b2[, w3, b3]), and the
                                             per-element bound on |device - model|

The backward is done in float64 on the chain's activations.  With L layers, a_0 = x and d_L = gq * (final_relu ? q > 0 : 1):

    gb_l = sum_r d_l[r]     gW_l = sum_r d_l[r] (x) a_(l-1)[r]     d_(l-1) = (W_l^T d_l) * (a_(l-1) > 0)

The bound.  E = c * 2^-24 * M, elementwise.  M is the same sums over absolute values (|gq|, |W|, |a|, the same masks).  c counts the fp32 roundings
on the longest path from the operands to a gradient element of layer l, whatever the order of the sums and whether or not products are fused into
the additions:

    the row sum           B terms: each term's product is rounded once and then passes through at most B - 1 additions      B
    each W^T d above it   n terms (n = the units of the layer the delta comes from): one product, at most n - 1 additions    n

so c_L = B, c_(l-1) = c_l + n_l.  Smart_State 59-h1-h2-5: c = B for gW3 / gb3, B + 5 for gW2 / gb2, B + 5 + h2 for gW1 / gb1; Minimized 59-h1-11:
B and B + 11.  The masks multiply by exact 0 or 1 and round nothing; gq * mask is exact.  That c u M bounds the error of a sum of c roundings to first
order is the classical result; that it holds without the second-order term for recursive sums and dot products is Jeannerod and Rump (2013).  c is
counted, not measured: nothing here looks at a device result.

exact=True is for the test families whose device result must be bit-equal: it asserts that no sum of the backward can round in fp32 in ANY order --
all terms of a sum are multiples of one power of two 2^e and the sum of their magnitudes is below 2^(24 + e) (integers: e = 0; a single non-zero
term; sums of equal powers of two), checked conservatively from the operands' lowest set bits -- so that the float64 result IS the fp32 result.

drop_row=r leaves row r's contribution out (its gq row is zeroed): what a skipped row does to the gradients; the CPU tests show the bound sees it."""
import numpy as np

import qnet_model

U = 2.0 ** -24
_BIG = 4096          # the "lowest set bit" of a zero: no constraint


def chain(x, params, final_relu):
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 59)
    ux, inv = np.unique(x, axis=0, return_inverse=True)
    inv = np.ravel(inv)
    layers = [(params[i], params[i + 1]) for i in range(0, len(params), 2)]
    acts, h = [ux], ux
    for i, (w, b) in enumerate(layers):
        last = i == len(layers) - 1
        h = qnet_model.layer(h, w, b, bool(final_relu) if last else True)
        if not last:
            acts.append(h)
    return [a[inv] for a in acts], h[inv]


def _lsb(a):
    """the exponent of the lowest set bit of every element (float64 holding fp32 values or exact products); _BIG for a zero"""
    a = np.asarray(a, np.float64)
    m, ex = np.frexp(a)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    with np.errstate(divide="ignore"):
        tz = np.where(mi > 0, np.log2(np.maximum(low, 1).astype(np.float64)), 0.0)
    return np.where(a != 0, ex - 53 + tz, _BIG)


def _assert_sums_exact(A, Bm, what):
    """sum_k A[m, k] Bm[k, n] cannot round in fp32 in any order: every term is a multiple of 2^e, e = min_k lsb A[m, k] + min_k lsb Bm[k, n] (a lower
    bound of the terms' own), and the magnitudes sum to less than 2^(24 + e)"""
    e = _lsb(A).min(1)[:, None] + _lsb(Bm).min(0)[None, :]
    S = np.abs(A) @ np.abs(Bm)
    with np.errstate(divide="ignore"):
        ok = (S == 0) | (np.log2(np.where(S > 0, S, 1.0)) < 24 + e)
    assert ok.all(), "a sum of %s may round in fp32" % what


def backward(x, params, final_relu, gq, exact=False, drop_row=None, clamp=0.0):
    params = [np.asarray(p, np.float32) for p in params]
    acts, q = chain(x, params, final_relu)
    acts = [a.astype(np.float64) for a in acts]
    B = acts[0].shape[0]
    L = len(params) // 2
    gq = np.array(gq, np.float32).reshape(B, -1).astype(np.float64)
    assert np.isfinite(gq).all() and all(np.isfinite(a).all() for a in acts) and np.isfinite(q).all(), "outside the pinned domain"
    if drop_row is not None:
        gq[drop_row] = 0.0
    d = gq * (q > 0) if final_relu else gq
    D = np.abs(d)
    c = float(B)
    grads, bounds = [None] * (2 * L), [None] * (2 * L)
    ones = np.ones((B, 1))
    for l in range(L, 0, -1):
        w = params[2 * (l - 1)].astype(np.float64)
        a = acts[l - 1]
        if exact:
            _assert_sums_exact(d.T, a, "gW%d" % l)
            _assert_sums_exact(d.T, ones, "gb%d" % l)
        grads[2 * (l - 1)], grads[2 * (l - 1) + 1] = d.T @ a, d.sum(0)
        bounds[2 * (l - 1)], bounds[2 * (l - 1) + 1] = c * U * (D.T @ np.abs(a)), c * U * D.sum(0)
        if l > 1:
            if exact:
                _assert_sums_exact(d, w, "W%d^T d%d" % (l, l))
            c += w.shape[0]
            d, D = (d @ w) * (a > 0), (D @ np.abs(w)) * (a > 0)
    if exact:
        for g in grads:
            assert np.array_equal(g.astype(np.float32).astype(np.float64), g), "a gradient is not an fp32 value"
    if clamp:
        grads = [np.clip(g, -clamp, clamp) for g in grads]
    return grads, bounds


def roundings(kind_sizes, B):
    """c of each layer's gradients for the layer widths (59, h1[, h2], OUT), last layer first: B, B + OUT, B + OUT + h2"""
    out, c = [], B
    for n in kind_sizes[:0:-1]:
        out.append(c)
        c += n
    return out
