"""CPU tests (no GPU needed) of the Q networks' bf16 forward: the host model (tests/qnet_bf16_model.py) against torch's bfloat16 on the CPU, the
error bound's power to see a defect, the exact-tier families of tests/qnet_bf16_cases.py, and the agreement of header / export list / binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import learner_edge_cases as edge
import qnet_bf16_cases as cases
import qnet_bf16_model as model

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = {"evg_smart_qnet_bf16": "evg_smart_qnet", "evg_minimized_qnet_bf16": "evg_minimized_qnet"}
NET_IDS = ["%s-%s" % (k, "x".join(map(str, h))) for k, h in cases.NETS]

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _torch_bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


# ---------------------------------------------------------------------- 1. bf16_rne
def test_bf16_rne_equals_torch_on_bit_patterns_ties_and_specials():
    rng = np.random.default_rng(16)
    u = rng.integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
    hi = rng.integers(0, 1 << 16, 1 << 14, dtype=np.uint64).astype(np.uint32) << np.uint32(16)
    ties = np.concatenate([hi | np.uint32(0x8000), hi | np.uint32(0x8001), hi | np.uint32(0x7FFF), hi])      # every tie, just above, just below, exact
    every_hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    specials = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, np.inf, -np.inf, np.nan, 0.0, -0.0, 1 + 2.0 ** -8,
                         1 + 2.0 ** -7 + 2.0 ** -8], np.float32).view(np.uint32)
    x = np.concatenate([u, ties, every_hi | np.uint32(0x8000), every_hi, specials]).view(np.float32)
    got, want = model.bf16_rne(x), _torch_bf16(x)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)                       # a NaN stays a NaN
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    assert (_bits(got) & 0xFFFF == 0).all()
    f = np.float32
    assert model.bf16_rne(f(np.finfo(np.float32).max)) == np.inf and model.bf16_rne(f(-np.finfo(np.float32).max)) == -np.inf
    assert model.bf16_rne(f(1 + 2.0 ** -8)) == 1.0 and model.bf16_rne(f(1 + 2.0 ** -7 + 2.0 ** -8)) == f(1 + 2.0 ** -6)
    assert model.bf16_rne(f(1 + 2.0 ** -8 + 2.0 ** -20)) == f(1 + 2.0 ** -7)


# ---------------------------------------------------------------------- 2. the model against torch's bfloat16 forward, within E
def _torch_forward(x, params, final_relu):
    """fp32 torch on the CPU over operands rounded by torch to bfloat16: another accumulation order, the same contract"""
    import torch
    h = torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(-1, 59).to(torch.bfloat16).to(torch.float32)
    layers = [(params[i], params[i + 1]) for i in range(0, len(params), 2)]
    for i, (w, b) in enumerate(layers):
        w = torch.from_numpy(w).to(torch.bfloat16).to(torch.float32)
        p = h @ w.T + torch.from_numpy(b)
        if i < len(layers) - 1:
            h = torch.relu(p).to(torch.bfloat16).to(torch.float32)
    return (torch.relu(p) if final_relu else p).numpy()


def _random_case(kind, hidden, family, layout):
    params, inputs = edge.case(kind, hidden, family, layout)
    return params, inputs


@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=NET_IDS)
def test_model_agrees_with_a_torch_bfloat16_forward_within_the_bound(kind, hidden, family):
    params, x = _random_case(kind, hidden, family, "expanded")
    for final_relu in (False, True):
        q, e = model.forward(x, params, final_relu)
        ok, worst = cases.within_bound(_torch_forward(x, params, final_relu), q, e)
        print("%s %s %s final_relu=%d: worst |torch - model| / E = %.3f" % (kind, hidden, family, final_relu, worst))
        assert ok, worst
    # the compact form is the expanded form of the expanded features
    params, (shared, swarm) = _random_case(kind, hidden, family, "compact")
    qc, ec = model.forward_compact(shared, swarm, params, False)
    qx, ex = model.forward(model.expand(shared, swarm), params, False)
    assert cases.same_values(qc, qx) and np.array_equal(ec, ex)


# ---------------------------------------------------------------------- 3. the bound can see a defect
@pytest.mark.parametrize("layout", ["expanded", "compact"])
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=NET_IDS)
def test_the_bound_sees_one_dropped_term(kind, hidden, family, layout):
    """One term of one output left out of the last layer -- the largest |w~ h| of that output -- moves it by more than the output's E, in every
    random-tier case: a wrong operand map cannot hide inside the tolerance.  The output is the one of an undamaged row whose largest term is the
    largest of all (a hidden layer of one unit can be all zeros in a given row)."""
    params, inputs = _random_case(kind, hidden, family, layout)
    x = inputs if layout == "expanded" else model.expand(*inputs).reshape(-1, 59)
    q, e = model.forward(x, params, False)
    clean = np.isfinite(x).all(1)
    best, where = 0.0, None
    for row in np.flatnonzero(clean)[:64]:
        for j in range(q.shape[1]):
            qd, _ = model.forward(x[row:row + 1], params, False, defect=(0, j))
            d = abs(float(qd[0, j]) - float(q[row, j]))
            if d > best:
                best, where = d, (row, j)
    assert where is not None
    row, j = where
    print("%s %s %s %s: dropping the largest term of output %s moves it by %.3g, E = %.3g" % (kind, hidden, family, layout, where, best, e[row, j]))
    assert best > e[row, j] > 0


# ---------------------------------------------------------------------- 4. the exact tier is exact
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden,family", cases.EXACT_CASES, ids=cases.EXACT_IDS)
def test_exact_tier_families_pass_the_models_exact_mode(kind, hidden, family, layout):
    params, inputs = cases.case(kind, hidden, family, layout)
    q, _ = model.forward_layout(layout, params, inputs, False, exact=True, rounds=family == "rounding")
    assert q.dtype == np.float32
    if family == "integer":
        assert np.isfinite(q).all() and (q == np.rint(q)).all() and np.abs(q).max() > 4
    if family == "permutation":
        assert np.isfinite(q).all() and (q != 0).mean() > (0.02 if min(hidden) == 1 else 0.2)
    if family == "rounding":                                  # the roundings it is about do happen: inputs, weights, an overflow to Inf
        flat = np.concatenate([np.ravel(a) for a in (inputs if isinstance(inputs, tuple) else (inputs,))])
        assert (model.bf16_rne(flat) != flat).mean() > 0.5 and np.isinf(model.bf16_rne(flat)).any() and np.isfinite(flat).all()
        sets = params if layout == "seats" else (params,)
        assert all((model.bf16_rne(p[0]) != p[0]).any() for p in sets)
    if family == "nonfinite":
        assert np.isnan(q).any() and np.isinf(q).any() and np.isfinite(q).mean() > 0.2


def test_exact_mode_refuses_what_may_round():
    params, x = edge.case("smart", (60, 60), "signed", "expanded")
    with pytest.raises(AssertionError):
        model.forward(x[:4], params, False, exact=True)
    params, x = cases.case("smart", (60, 60), "rounding", "expanded")
    with pytest.raises(AssertionError):
        model.forward(x[:4], params, False, exact=True, rounds=False)


# ---------------------------------------------------------------------- 5. header, export list and binding agree
def _prototype_args(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototypes_ctypes_argtypes_and_exports_agree():
    """The two entry points live in include/evg_qnet_bf16.h and libevg_bf16.so (the product's sources with -DEVG_BF16), with the argument lists of
    the fp32 entry points; libevg.so and include/evg.h keep exactly the entry points they had."""
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_qnet_bf16.h")).read()
    main_header = open(os.path.join(ROOT, "include", "evg.h")).read()
    assert _lib.BF16_EXPORTS == list(ENTRY_POINTS) and not set(ENTRY_POINTS) & set(_lib.EXPORTS)
    assert set(re.findall(r"EVG_API \w+ (evg_[a-z0-9_]+)\s*\(", header)) == set(ENTRY_POINTS)
    assert not any(name + "(" in main_header for name in ENTRY_POINTS)
    lib = _lib.load_bf16()
    assert lib.evg_abi_version() == _lib.ABI_VERSION
    for name, fp32 in ENTRY_POINTS.items():
        assert _prototype_args(header, name) == _prototype_args(main_header, fp32), name
        assert list(getattr(lib, name).argtypes) == list(getattr(lib, fp32).argtypes), name

    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert exported(_lib.BF16_LIB_PATH) == set(_lib.EXPORTS) | set(ENTRY_POINTS)
    assert exported(_lib.LIB_PATH) == set(_lib.EXPORTS)
    assert issubclass(everglades_amd.SmartQNetBf16, everglades_amd.SmartQNet) and issubclass(everglades_amd.MinimizedQNetBf16, everglades_amd.MinimizedQNet)
    assert not issubclass(everglades_amd.SmartQNetBf16, everglades_amd.MinimizedQNet)
    for cls, base in ((everglades_amd.SmartQNetBf16, everglades_amd.SmartQNet), (everglades_amd.MinimizedQNetBf16, everglades_amd.MinimizedQNet)):
        for name in ("__call__", "expanded", "_params", "_descriptor", "_run", "_input", "__init__"):
            assert getattr(cls, name) is getattr(base, name), (cls, name)                  # only the launch differs
        assert cls._launch is not base._launch


def test_an_unknown_precision_is_a_value_error():
    import everglades_amd
    env = object.__new__(everglades_amd.EvergladesVecEnv)             # the precision is checked before anything of the env is touched
    for make in (everglades_amd.EvergladesVecEnv.smart_qnet, everglades_amd.EvergladesVecEnv.minimized_qnet):
        with pytest.raises(ValueError, match="precision"):
            make(env, None, precision="int8")
        with pytest.raises(ValueError, match="precision"):
            make(env, None, precision=None)


# ---------------------------------------------------------------------- 6. the new kernels' static resources
def test_bf16_kernels_have_no_scratch_and_no_vgpr_spills():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "FLAGS_EXTRA=-DEVG_BF16"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    names = [n for n in usage if re.search(r"evg_(mini_)?qnet_bf16_kernel", n)]
    assert len(names) == 4, names
    for n in names:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0", (n, u)
