"""CPU tests (no GPU needed) of the host model of the device Q network (tests/qnet_model.py): its exact fp32 fma against libm's fmaf, its forward
pass against the reference's QNetwork (tests/golden/smart_qnet.npz, tools/gen_qnet_golden.py), and its compact and expanded forms against each other."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from conftest import load_golden
from qnet_model import expand, fmaf32, forward, forward_compact

NETS = ["a", "b", "c"]
RTOL, ATOL = 1e-5, 1e-5            # torch CPU's GEMM does not add in the chain's order (|Q| ~ 1: cancellation leaves ~1e-6 absolute)


def _libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    f = libm.fmaf
    f.argtypes, f.restype = [ctypes.c_float] * 3, ctypes.c_float
    return f


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def test_fma_emulation_equals_libm_fmaf_on_random_triples():
    rng = np.random.default_rng(7)
    n = 100000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    c[: n // 4] = -(a[: n // 4].astype(np.float64) * b[: n // 4]).astype(np.float32)     # heavy cancellation
    f = _libm_fmaf()
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(_bits(fmaf32(a, b, c)), _bits(want))


def test_fma_emulation_settles_halfway_cases_by_the_exact_sum():
    # c + a*b where the float64 sum lies exactly midway between two fp32 values and the rest of a*b decides the rounding
    f = _libm_fmaf()
    cases = []
    for e in (0, 3, -5, 20):
        c = np.float32(2.0 ** e)
        half = 2.0 ** (e - 24)                      # half an fp32 ulp of c
        for sgn in (1.0, -1.0):
            for tiny in (2.0 ** -30, -2.0 ** -30, 0.0):
                # a * b = sgn * (half + tiny * half): exact in float64, not in fp32 -> the float64 sum may round to the midpoint
                a = np.float32(1.0 + tiny) if tiny else np.float32(1.0)
                b = np.float32(sgn * half)
                cases.append((a, b, c))
                cases.append((np.float32(1.0 + 2.0 ** -23), np.float32(sgn * half * (1.0 - 2.0 ** -24)), c))
                cases.append((np.float32(3.0), np.float32(sgn * half / 3.0), np.float32(c * (1 + 2.0 ** -23))))
    a, b, c = (np.array(v, np.float32) for v in zip(*cases))
    s = a.astype(np.float64) * b + c
    r = s.astype(np.float32).astype(np.float64)
    assert len(cases) >= 48
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in cases], np.float32)
    assert np.array_equal(_bits(fmaf32(a, b, c)), _bits(want))
    assert (s != r).any()                           # the set reaches inexact sums


def test_fma_emulation_on_constructed_ties():
    # s = c + a*b with c = 1 and a*b = 2^-24 + 2^-60 * k: the float64 sum 1 + 2^-24 is a tie, the TwoSum error decides
    f = _libm_fmaf()
    a = np.full(6, 2.0 ** -12, np.float32)
    b = np.array([2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -24), 2.0 ** -12, -2.0 ** -12 * (1 + 2.0 ** -23),
                  -2.0 ** -12 * (1 - 2.0 ** -24), -2.0 ** -12], np.float32)
    c = np.array([1.0, 1.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23], np.float32)
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(_bits(fmaf32(a, b, c)), _bits(want))


def _class_triples(name, n, rng):
    """n random fp32 triples (a, b, c) of one exponent class of a * b + c"""
    def val(lo, hi):
        return (rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n)) * np.exp2(rng.integers(lo, hi, n))).astype(np.float32)
    if name == "normal":
        return val(-30, 30), val(-30, 30), val(-60, 60)
    if name == "subnormal product, subnormal addend":
        return val(-80, -60), val(-89, -66), val(-149, -126)
    if name == "subnormal x normal":
        return val(-149, -126), val(-8, 8), val(-149, -120)
    if name == "overflow":
        return val(60, 127), val(0, 68), val(100, 128)
    return val(-149, 128), val(-149, 128), val(-149, 128)                    # the full range


CLASSES = ["normal", "subnormal product, subnormal addend", "subnormal x normal", "overflow", "full range"]


def _same(got, want):
    """equal NaN masks, equal bits elsewhere (a NaN's sign and payload are not part of the contract)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


@pytest.mark.parametrize("name", CLASSES)
def test_fma_emulation_equals_libm_fmaf_in_every_exponent_class(name):
    """The emulation holds over the whole of fp32 -- subnormal operands and results, overflow to Inf -- not only where product and sum stay normal."""
    rng = np.random.default_rng(CLASSES.index(name) + 11)
    a, b, c = _class_triples(name, 4000, rng)
    f = _libm_fmaf()
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    with np.errstate(all="ignore"):
        got = fmaf32(a, b, c)
    assert _same(got, want)
    tiny = np.finfo(np.float32).tiny
    if "subnormal" in name:                                                  # the class reaches what it names
        assert ((np.abs(want) < tiny) & (want != 0)).mean() > 0.2
    if name == "overflow":
        assert 0.2 < np.isinf(want).mean() < 0.999
    if name == "full range":
        assert np.isinf(want).any() and (np.abs(want) < tiny).any() and np.isfinite(want).mean() > 0.3


def test_fma_emulation_on_non_finite_operands_and_signed_zeros():
    inf, nan, big = np.inf, np.nan, 3.0e38
    cases = [(nan, 1, 1), (1, nan, 1), (1, 1, nan), (inf, 2, 1), (-inf, 2, 1), (2, inf, -1), (1, 1, inf), (1, 1, -inf), (inf, 0, 1), (0, -inf, 1),
             (inf, 0, nan), (inf, 1, -inf), (-inf, 1, inf), (inf, -1, inf), (inf, 1, inf), (-inf, -1, -inf), (big, 2, -inf), (big, big, -big),
             (big, -big, big), (big, 2, -big), (0.0, 1, 0.0), (-0.0, 1, 0.0), (-0.0, 1, -0.0), (0.0, -1, -0.0), (1, 1, -1), (-1, 1, 1), (0.0, 5, -0.0),
             (1e-30, 1e-30, 0.0), (1e-30, -1e-30, 0.0), (1e-30, -1e-30, -0.0), (1e-45, 0.5, 0.0), (1e-45, 0.5, 1e-45)]
    a, b, c = (np.array(v, np.float32) for v in zip(*cases))
    f = _libm_fmaf()
    want = np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    with np.errstate(all="ignore"):
        got = fmaf32(a, b, c)
    assert _same(got, want)
    assert np.isnan(want).sum() >= 8 and np.isinf(want).sum() >= 8


def _params(d, v):
    return tuple(d[v + "_" + k] for k in ("w1", "b1", "w2", "b2", "w3", "b3"))


@pytest.mark.parametrize("v", NETS)
def test_host_model_reproduces_the_reference_qnetwork(v):
    d = load_golden("smart_qnet.npz")
    x = load_golden("smart_state.npz")["features"].astype(np.float32)
    q = forward(x, _params(d, v), final_relu=True)
    assert q.dtype == np.float32 and q.shape == d[v + "_q"].shape
    np.testing.assert_allclose(q, d[v + "_q"], rtol=RTOL, atol=ATOL)
    assert not np.allclose(forward(x, _params(d, v), final_relu=False), d[v + "_q"], rtol=RTOL, atol=ATOL)   # the final ReLU is pinned


@pytest.mark.parametrize("v", NETS)
@pytest.mark.parametrize("final_relu", [False, True])
def test_host_model_compact_and_expanded_forms_agree_exactly(v, final_relu):
    d = load_golden("smart_qnet.npz")
    x = load_golden("smart_state.npz")["features"].astype(np.float32).reshape(-1, 12, 59)
    shared, swarm = x[:, 0, :34], x[:, :, 34:47]
    assert np.array_equal(expand(shared, swarm), x)
    p = _params(d, v)
    assert np.array_equal(forward_compact(shared, swarm, p, final_relu), forward(x, p, final_relu))
