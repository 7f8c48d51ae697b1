"""Host model of the Q networks' bf16 forward (everglades_amd.SmartQNetBf16 / MinimizedQNetBf16, include/evg_qnet_bf16.h): the numeric contract in numpy.

  bf16_rne(x)        float32 -> the nearest bfloat16 (ties to even) as float32, on the bit pattern: overflow gives +-Inf, a NaN stays a NaN.
  forward(...)       expanded rows x [..., 59] -> (Q, E);  forward_compact(...)  shared [N, 34], swarm [N, 12, 13] -> (Q, E) of shape [N, 12, out].
                     params are (w1, b1, w2, b2, w3, b3) (Smart_State, 5 outputs) or (w1, b1, w2, b2) (Minimized, 11 outputs).

The forward is computed in float64 on the rounded operands (inputs and weights bf16_rne, biases as they are), hidden activations
bf16_rne(relu(pre)) with relu(p) = p < 0 ? 0 : p (a NaN stays), the output layer unrounded (through the same ReLU with final_relu).  The model has no
padded units.  Q is returned as float32 (the float64 value rounded once), E as float64.

E bounds |device Q - model Q| per output when the device accumulates in fp32 in ANY order with one rounding (to nearest or truncating) per addition;
u = 2^-24.  For a layer of K terms whose inputs h carry an error of at most e_in (zero for layer 1):

    e_pre = sum_k |w~_k| e_in,k  +  ALLOW (K + 1) u (|b| + sum_k |w~_k| (|h_k| + e_in,k))        ALLOW = 2 roundings' worth per addition
    e_h   = e_pre + 2^-8 (relu(p) + e_pre)

The first line: K + 1 additions, each off by at most 2u relative to a partial sum that the bracket bounds.  The second: two RNE roundings to bf16 of
values e_pre apart differ by at most e_pre plus two half-ulps, an ulp of bf16 being at most 2^-7 of the value.  E is e_pre of the last layer.  Where
a pre-activation is not finite (an Inf or NaN operand: the device holds the same Inf or NaN) its error is zero.

exact=True is for the test families whose device result must be bit-equal: it asserts that no accumulation can round -- every pre-activation has at
most one non-zero term (bias included), or all its terms are integers, and |b| + sum |w~ h| stays below 2^24 -- so that the float64 value IS the fp32
value whatever the order.  With rounds=False it also asserts that every bf16 rounding (inputs, weights, hidden activations) was the identity; the
`rounding` family, whose point is those roundings, passes rounds=True.

defect=(row, j): the largest |w~ h| term of output j of (flattened) row `row` is left out of the last layer -- what a wrong operand map does to an
output; the CPU tests show that the bound sees it."""
import numpy as np

U = 2.0 ** -24
ALLOW = 2.0          # roundings' worth (u each) allowed per addition


def bf16_rne(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u | 0x00400000) & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def _relu(p):
    return np.where(p < 0, 0.0, p)            # a NaN compares false: it stays


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _layer(h, e_in, w, b, exact, rounds, defect=None):
    """h [R, K] float64 (already rounded), e_in [R, K] -> (p, e_pre) [R, H] in float64"""
    w32 = np.asarray(w, np.float32)
    wt = bf16_rne(w32).astype(np.float64)
    if exact and not rounds:
        assert _same(wt, w32.astype(np.float64)), "a weight is not a bfloat16 value"
    b = np.asarray(b, np.float32).astype(np.float64)
    K = wt.shape[1]
    with np.errstate(all="ignore"):
        p = b[None, :] + h @ wt.T
        if defect is not None:
            row, j = defect
            t = wt[j] * h[row]
            k = int(np.nanargmax(np.abs(t)))
            p[row, j] = b[j] + np.delete(t, k).sum()
        mag = np.abs(b)[None, :] + (np.abs(h) + e_in) @ np.abs(wt).T
        e_pre = e_in @ np.abs(wt).T + ALLOW * (K + 1) * U * mag
        e_pre = np.where(np.isfinite(p), e_pre, 0.0)
        if exact:
            terms = h[:, None, :] * wt[None, :, :]                                  # [R, H, K], each product exact in float64
            finite = np.isfinite(terms).all(2) & np.isfinite(b)[None, :]
            count = (terms != 0).sum(2) + (b != 0)[None, :]
            integers = (terms == np.rint(terms)).all(2) & (b == np.rint(b))[None, :]
            a = np.abs(b)[None, :] + np.abs(terms).sum(2)
            ok = ~finite | (((count <= 1) | integers) & (a < 2.0 ** 24))
            assert ok.all(), "an accumulation of this case may round in fp32"
    return p, e_pre


def _hidden(p, e_pre, exact, rounds):
    with np.errstate(all="ignore"):
        r = _relu(p)
        h32 = r.astype(np.float32)
        if exact:
            assert _same(h32.astype(np.float64), r), "a hidden pre-activation is not an fp32 value"
        h = bf16_rne(h32).astype(np.float64)
        if exact and not rounds:
            assert _same(h, r), "a hidden activation is not a bfloat16 value"
        e_h = e_pre + 2.0 ** -8 * (np.where(np.isfinite(r), r, 0.0) + e_pre)
        e_h = np.where(np.isfinite(p), e_h, 0.0)
    return h, e_h


def forward(x, params, final_relu, exact=False, rounds=True, defect=None):
    """Expanded rows x [..., 59] -> (Q float32 [..., out], E float64 [..., out])."""
    x = np.asarray(x, np.float32)
    lead = x.shape[:-1]
    x = x.reshape(-1, 59)
    h = bf16_rne(x).astype(np.float64)
    if exact and not rounds:
        assert _same(h, x.astype(np.float64)), "an input is not a bfloat16 value"
    e = np.zeros_like(h)
    layers = [(params[i], params[i + 1]) for i in range(0, len(params), 2)]
    for i, (w, b) in enumerate(layers):
        last = i == len(layers) - 1
        p, e_pre = _layer(h, e, w, b, exact, rounds, defect if last else None)
        if last:
            break
        h, e = _hidden(p, e_pre, exact, rounds)
    with np.errstate(all="ignore"):
        q = _relu(p) if final_relu else p
        q32 = q.astype(np.float32)
    if exact:
        assert _same(q32.astype(np.float64), q), "an output is not an fp32 value"
    out = q.shape[1]
    return q32.reshape(lead + (out,)), e_pre.reshape(lead + (out,))


def expand(shared, swarm):
    """[N, 12, 59] = cat(shared, swarm[s], onehot(s))."""
    shared, swarm = np.asarray(shared, np.float32), np.asarray(swarm, np.float32)
    N = shared.shape[0]
    x = np.zeros((N, 12, 59), np.float32)
    x[:, :, :34] = shared[:, None, :]
    x[:, :, 34:47] = swarm
    x[:, np.arange(12), 47 + np.arange(12)] = 1.0
    return x


def forward_compact(shared, swarm, params, final_relu, exact=False, rounds=True, defect=None):
    """Compact features shared [N, 34], swarm [N, 12, 13] -> (Q, E) [N, 12, out]: the expanded forward of expand(shared, swarm) (contract item 3)."""
    return forward(expand(shared, swarm), params, final_relu, exact, rounds, defect)


def forward_layout(layout, params, inputs, final_relu, exact=False, rounds=True):
    """layout "expanded": inputs x;  "compact": (shared, swarm);  "seats": ([N, 2, 34], [N, 2, 12, 13]) with params = (set of seat 0, set of seat 1)"""
    if layout == "expanded":
        return forward(inputs, params, final_relu, exact, rounds)
    shared, swarm = inputs
    if layout == "compact":
        return forward_compact(shared, swarm, params, final_relu, exact, rounds)
    qs = [forward_compact(shared[:, p], swarm[:, p], params[p], final_relu, exact, rounds) for p in range(2)]
    return np.stack([q for q, _ in qs], 1), np.stack([e for _, e in qs], 1)
