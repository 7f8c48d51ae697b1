"""Host model of the agents/DQN Q network's backward pass (DqnQNet.with_grad, include/evg_dqn_grad.h): the contract in numpy, as
tests/qnet_grad_model.py states it for the two small networks.

  chain(x, params, final_relu)            -> ([x, a1], q): the activations and the output of the exact fp32 fmaf chain (tests/dqn_model.py, whose
                                             layers are tests/qnet_model.layer), computed once per distinct row of x
  backward(x, params, final_relu, gq)     -> (grads, E): the parameter gradients in float64, in the order of params (w1, b1, w2, b2), and the
                                             per-element bound on |device - model|

The backward is done in float64 on the chain's activations:

    d2  = gq * (final_relu ? q > 0 : 1)     gb2 = sum_r d2[r]     gW2 = sum_r d2[r] (x) a1[r]
    d1  = (W2^T d2) * (a1 > 0)              gb1 = sum_r d1[r]     gW1 = sum_r d1[r] (x) x[r]

The bound.  E = c * 2^-24 * M, elementwise.  M is the same sums over absolute values (|gq|, |W2|, |a1|, |x|, the same masks).  c counts the fp32
roundings on the longest path from the operands to a gradient element, whatever the order of the sums and whether or not products are fused into the
additions: a row sum of B terms rounds each product once and passes it through at most B - 1 additions (B); W2^T d2 above gW1 / gb1 has 132 terms
(one product, at most 131 additions: 132).  So c = B for gW2 / gb2 and B + 132 for gW1 / gb1.  The masks multiply by exact 0 or 1; gq * mask is
exact.  c is counted, not measured: nothing here looks at a device result.  (The first-order form c u M holds without a second-order term for
recursive sums and dot products: Jeannerod and Rump, 2013.)

exact=True asserts, with qnet_grad_model's predicate, that no sum of the backward can round in fp32 in ANY order, so that the float64 result IS the
fp32 result.  drop_row=r leaves row r's contribution out (its gq row is zeroed)."""
import numpy as np

import dqn_model
from qnet_model import layer
from qnet_grad_model import U, _assert_sums_exact

IN, OUT = dqn_model.IN, dqn_model.OUT


def chain(x, params, final_relu):
    x = np.ascontiguousarray(x, np.float32).reshape(-1, IN)
    ux, inv = np.unique(x, axis=0, return_inverse=True)
    inv = np.ravel(inv)
    w1, b1, w2, b2 = params
    a1 = layer(ux, w1, b1, True)
    q = layer(a1, w2, b2, bool(final_relu))
    return [ux[inv], a1[inv]], q[inv]


def roundings(B):
    """c of (gW2 / gb2, gW1 / gb1)"""
    return B, B + OUT


def backward(x, params, final_relu, gq, exact=False, drop_row=None, clamp=0.0):
    params = [np.asarray(p, np.float32) for p in params]
    (x0, a1), q = chain(x, params, final_relu)
    x0, a1 = x0.astype(np.float64), a1.astype(np.float64)
    B = x0.shape[0]
    gq = np.array(gq, np.float32).reshape(B, OUT).astype(np.float64)
    assert np.isfinite(gq).all() and np.isfinite(x0).all() and np.isfinite(a1).all() and np.isfinite(q).all(), "outside the pinned domain"
    if drop_row is not None:
        gq[drop_row] = 0.0
    w2 = params[2].astype(np.float64)
    d2 = gq * (q > 0) if final_relu else gq
    D2 = np.abs(d2)
    d1, D1 = (d2 @ w2) * (a1 > 0), (D2 @ np.abs(w2)) * (a1 > 0)
    c2, c1 = roundings(B)
    if exact:
        ones = np.ones((B, 1))
        _assert_sums_exact(d2.T, a1, "gW2")
        _assert_sums_exact(d2.T, ones, "gb2")
        _assert_sums_exact(d2, w2, "W2^T d2")
        _assert_sums_exact(d1.T, x0, "gW1")
        _assert_sums_exact(d1.T, ones, "gb1")
    grads = [d1.T @ x0, d1.sum(0), d2.T @ a1, d2.sum(0)]
    bounds = [c1 * U * (D1.T @ np.abs(x0)), c1 * U * D1.sum(0), c2 * U * (D2.T @ a1), c2 * U * D2.sum(0)]
    if exact:
        for g in grads:
            assert np.array_equal(g.astype(np.float32).astype(np.float64), g), "a gradient is not an fp32 value"
    if clamp:
        grads = [np.clip(g, -clamp, clamp) for g in grads]
    return grads, bounds
