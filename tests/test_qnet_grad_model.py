"""CPU tests (no GPU needed) of the Q networks' backward pass: the host model (tests/qnet_grad_model.py) against torch.autograd in float64, the error
bound's power to see a dropped row, the exact-tier families of tests/qnet_grad_cases.py at the sizes the device runs them, the condition on the random
families, and the agreement of header / export list / binding / static resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import qnet_grad_cases as cases
import qnet_grad_model as model

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = ["evg_smart_qnet_backward", "evg_minimized_qnet_backward"]
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


# ---------------------------------------------------------------------- 1. the model against torch.autograd in float64
def _torch_grads(x, params, final_relu, gq):
    """torch.autograd in float64 over the model's own activations and masks: a hidden layer's value is the chain's a (so that the outer products and
    the masks are the contract's), its derivative the mask's"""
    import torch
    acts, q = model.chain(x, params, final_relu)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float64))
    ps = [t(p).requires_grad_() for p in params]
    h = t(x)
    layers = len(ps) // 2
    for l in range(layers):
        z = h @ ps[2 * l].T + ps[2 * l + 1]
        if l < layers - 1:
            a = t(acts[l + 1])
            m = (a > 0).double()
            h = z * m + (a - z * m).detach()
        else:
            out = z * t(q > 0) if final_relu else z
    out.backward(t(gq))
    return [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_model_agrees_with_torch_autograd_in_float64(kind, hidden, family, final_relu):
    params, x, gq = cases.case(kind, hidden, family, cases.RANDOM_ROWS)
    grads, bounds = model.backward(x, params, final_relu, gq)
    want = _torch_grads(x, params, final_relu, gq)
    cs = model.roundings(cases.sizes(kind, hidden), x.shape[0])[::-1]
    for i, (g, e, w) in enumerate(zip(grads, bounds, want)):
        M = e / (cs[i // 2] * model.U)                                  # the sums over absolute values
        assert g.shape == w.shape == tuple(params[i].shape)
        assert (np.abs(g - w) <= 1e-12 * M).all(), (NAMES[i], float(np.abs(g - w).max()))
        assert np.abs(g).max() > 0 or hidden in ((1, 1), (1,))


def test_the_count_of_roundings_is_the_headers():
    assert model.roundings((59, 60, 60, 5), 256) == [256, 256 + 5, 256 + 5 + 60]
    assert model.roundings((59, 80, 11), 1024) == [1024, 1024 + 11]
    params, x, gq = cases.case("smart", (3, 64), "dense", 17)
    _, bounds = model.backward(x, params, False, gq)
    acts, _ = model.chain(x, params, False)
    assert np.allclose(bounds[5], 17 * model.U * np.abs(gq).sum(0), rtol=1e-12)
    assert np.allclose(bounds[4], 17 * model.U * np.abs(gq.astype(np.float64)).T @ np.abs(acts[2].astype(np.float64)), rtol=1e-12)


# ---------------------------------------------------------------------- 2. the bound can see a dropped row
@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_the_bound_sees_one_dropped_row(kind, hidden, family, final_relu):
    """Leaving one row's contribution out moves some gradient element by more than that element's E, whichever row (of 9 spread over the batch) it
    is whose upstream gradient reaches a parameter at all: a skipped row cannot hide inside the tolerance."""
    params, x, gq = cases.case(kind, hidden, family, cases.RANDOM_ROWS)
    grads, bounds = model.backward(x, params, final_relu, gq)
    seen = 0
    for row in range(0, cases.RANDOM_ROWS, 31):
        dropped, _ = model.backward(x, params, final_relu, gq, drop_row=row)
        moved = max(float((np.abs(d - g) - e).max()) for d, g, e in zip(dropped, grads, bounds))
        reaches = any((d != g).any() for d, g in zip(dropped, grads))
        assert moved > 0 or not reaches, (row, moved)
        seen += reaches
    assert seen >= 1                              # (a row whose one gq entry sits on a clipped output reaches nothing)


# ---------------------------------------------------------------------- 3. the exact tier is exact at the sizes the device runs it
@pytest.mark.parametrize("final_relu", [False, True])
@pytest.mark.parametrize("family", cases.EXACT_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_exact_tier_families_pass_the_models_exact_mode(kind, hidden, family, final_relu):
    for rows in (1, 17, cases.ROWS[-1]):
        params, x, gq = cases.case(kind, hidden, family, rows)
        grads, _ = model.backward(x, params, final_relu, gq, exact=True)
        if family == "pow2dup":                                       # B equal rows: B times the one-row gradient
            one, _ = model.backward(x[:1], params, final_relu, gq[:1], exact=True)
            assert all(np.array_equal(g, rows * o) for g, o in zip(grads, one))
    assert any(np.abs(g).max() > 0 for g in grads)
    if family == "integer":
        assert all((g == np.rint(g)).all() for g in grads) and max(np.abs(g).max() for g in grads) > 4


@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_the_integer_family_is_exact_over_two_sweeps_of_the_capped_grid(kind, hidden):
    import everglades_amd
    rows = cases.sweep_rows(everglades_amd._lib.QNET_GRAD_MAX_BLOCKS)
    assert rows == 65555
    params, x, gq = cases.case(kind, hidden, "integer", rows)
    for final_relu in (False, True):
        grads, _ = model.backward(x, params, final_relu, gq, exact=True)
        assert max(np.abs(g).max() for g in grads) > 1000


def test_exact_mode_refuses_what_may_round():
    for family in cases.RANDOM_FAMILIES:
        params, x, gq = cases.case("smart", (60, 60), family, 17)
        with pytest.raises(AssertionError):
            model.backward(x, params, False, gq, exact=True)
    params, x, gq = cases.case("mini", (80,), "integer", 17)          # integers, but one row sum of 2^24 + 1
    gq[:, 0] = 0
    gq[0, 0], gq[1, 0] = 2.0 ** 24, 1.0
    with pytest.raises(AssertionError):
        model.backward(x, params, False, gq, exact=True)


# ---------------------------------------------------------------------- 4. both sides of every mask are exercised
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_random_families_exercise_both_sides_of_the_masks(kind, hidden, family):
    """Between 20 % and 80 % of the hidden units are active over the batch, and at least one unit is dead in every row.  A network with one or two
    hidden units in all cannot meet both (one unit dead in every row leaves at most half active, none of a single unit): there the units must be
    active in some rows and dead in others."""
    params, x, gq = cases.case(kind, hidden, family, cases.RANDOM_ROWS)
    acts, q = model.chain(x, params, True)
    active = np.concatenate([a > 0 for a in acts[1:]], 1)
    assert 0.2 <= active.mean() <= 0.8, active.mean()
    if cases.has_dead_unit(hidden):
        assert not active[:, cases.DEAD_UNIT].any() and (~active).any(1).all()
    else:
        assert active.any(0).all() and (~active).any(0).all()
    assert 0.1 <= (q > 0).mean() <= 0.9


# ---------------------------------------------------------------------- 5. header, export list and binding agree
def _prototype_args(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototypes_ctypes_argtypes_and_exports_agree():
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_qnet_grad.h")).read()
    main_header = open(os.path.join(ROOT, "include", "evg.h")).read()
    assert _lib.GRAD_EXPORTS == ENTRY_POINTS and not set(ENTRY_POINTS) & set(_lib.EXPORTS)
    assert set(re.findall(r"EVG_API \w+ (evg_[a-z0-9_]+)\s*\(", header)) == set(ENTRY_POINTS)
    assert not any(name + "(" in main_header for name in ENTRY_POINTS)
    for macro, value in (("EVG_QNET_GRAD_MAX_BLOCKS", _lib.QNET_GRAD_MAX_BLOCKS), ("EVG_SMART_QNET_GRAD_PARTIAL", _lib.SMART_QNET_GRAD_PARTIAL),
                         ("EVG_MINI_QNET_GRAD_PARTIAL", _lib.MINI_QNET_GRAD_PARTIAL)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert _lib.SMART_QNET_GRAD_PARTIAL == 2 * 64 * 64 + 16 * 64 + 64 + 64 + 16 and _lib.MINI_QNET_GRAD_PARTIAL == 128 * 64 + 16 * 128 + 128 + 16
    lib = _lib.load_grad()
    assert lib.evg_abi_version() == _lib.ABI_VERSION
    kinds = {"evg_handle* h": C.c_void_p, "int64_t rows": C.c_int64, "const float* x": C.c_void_p, "const float* gq": C.c_void_p,
             "void* workspace": C.c_void_p, "int64_t workspace_bytes": C.c_int64, "float clamp": C.c_float, "void* stream": C.c_void_p,
             "const evg_qnet* net": C.POINTER(_lib.EvgQnet), "const evg_mini_qnet* net": C.POINTER(_lib.EvgMiniQnet),
             "const evg_qnet_grads* grads": C.POINTER(_lib.EvgQnetGrads), "const evg_mini_qnet_grads* grads": C.POINTER(_lib.EvgMiniQnetGrads)}
    for name in ENTRY_POINTS:
        assert [kinds[a] for a in _prototype_args(header, name)] == list(getattr(lib, name).argtypes), name
    for struct, fields in ((_lib.EvgQnetGrads, NAMES), (_lib.EvgMiniQnetGrads, NAMES[:4])):
        assert [n for n, _ in struct._fields_] == ["struct_size", "reserved"] + list(fields) and C.sizeof(struct) == 8 + 8 * len(fields)
        body = re.search(r"typedef struct (\w+) \{([^}]*)\} \1;", header[header.index("typedef struct evg_%sqnet_grads" % ("" if len(fields) == 6 else "mini_")):])
        assert re.findall(r"(?:uint32_t|float\*) (\w+);", body.group(2)) == ["struct_size", "reserved"] + list(fields)

    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert len(_lib.EXPORTS) == 70
    assert exported(_lib.GRAD_LIB_PATH) == set(_lib.EXPORTS) | set(ENTRY_POINTS)
    assert exported(_lib.LIB_PATH) == set(_lib.EXPORTS)


def test_with_grad_is_refused_by_the_bf16_classes_before_anything_is_touched():
    import everglades_amd
    for cls in (everglades_amd.SmartQNetBf16, everglades_amd.MinimizedQNetBf16):
        with pytest.raises(ValueError, match="fp32 chain"):
            cls.with_grad(object.__new__(cls), None)
    assert everglades_amd.MinimizedQNet.with_grad is everglades_amd.SmartQNet.with_grad


# ---------------------------------------------------------------------- 6. the new kernels' static resources
def test_grad_kernels_have_no_scratch_and_no_vgpr_spills():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "FLAGS_EXTRA=-DEVG_GRAD"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    names = [n for n in usage if re.search(r"evg_(mini_)?qnet_grad_(reduce_)?kernel", n)]
    assert len(names) == 3, names
    for n in names:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
        assert int(u["LDS Size [bytes/block]"]) <= 65536
