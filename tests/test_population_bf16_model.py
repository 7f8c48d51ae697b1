"""CPU tests of the populations' grouped bf16 forward (include/evg_pop_bf16.h, everglades_amd.QPopulationBf16 / SmartQPopulationBf16): the composed host
model (tests/population_bf16_cases.py) against its two parts, header / binding / export agreement of libevg_popbf16.so, the six older libraries' export
sets, the four new kernels' static resources, and the Python surface's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import population_bf16_cases as pcases
import population_edge_cases as pedge
import qnet_bf16_cases as cases
import qnet_bf16_model as model

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
ENTRY_POINTS = ["evg_population_qnet_bf16", "evg_smart_population_qnet_bf16"]


# ---------------------------------------------------------------------- 1. the model is its two parts
@pytest.mark.parametrize("layout", pcases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden", [("smart", (17, 64)), ("mini", (80,))], ids=["smart", "mini"])
def test_a_team_of_one_is_the_plain_bf16_model(kind, hidden, layout):
    inputs = pcases.case_inputs("integer", layout)
    rows = pcases.num_rows(layout, inputs)
    if layout == "seats":
        teams = [pcases.team(kind, hidden, "integer", 1, p) for p in range(2)]
        ids, plain = np.zeros((rows, 2), np.uint8), (teams[0][0], teams[1][0])
    else:
        teams = pcases.team(kind, hidden, "integer", 1)
        ids, plain = np.zeros(rows, np.uint8), teams[0]
    got, E = pcases.forward(kind, layout, teams, inputs, ids, True)
    want, wE = model.forward_layout({"seat": "compact"}.get(layout, layout), plain, inputs, True)
    assert np.array_equal(got, want) and np.array_equal(E, wE) and np.abs(want).sum() > 0


def test_one_rows_id_changes_that_row_alone_and_nobody_gets_zeros():
    kind, hidden, K, rows = "smart", (60, 60), 4, 37
    teams = pcases.team(kind, hidden, "integer", K)
    x = pcases.case_inputs("integer", "expanded", rows)
    ids = pcases.ids("round_robin", rows, K)
    base, _ = pcases.forward(kind, "expanded", teams, x, ids, False)
    for r, new in ((0, 3), (16, 2), (36, 1)):
        other = ids.copy()
        other[r] = new
        got, _ = pcases.forward(kind, "expanded", teams, x, other, False)
        changed = np.flatnonzero((got != base).any(1))
        assert changed.tolist() == [r], (r, changed)
        assert np.array_equal(got[r], model.forward(x[r:r + 1], teams[new], False)[0][0])
    bad = pcases.ids("bad", rows, K)
    got, E = pcases.forward(kind, "expanded", teams, x, bad, False)
    nobody = bad >= K
    assert nobody.sum() >= 8 and not got[nobody].any() and not E[nobody].any() and got[~nobody].any(1).all()
    assert set(bad[nobody].tolist()) == set(pedge.BAD_IDS)


@pytest.mark.parametrize("pattern", pcases.PATTERNS)
def test_the_id_patterns_are_what_their_names_say(pattern):
    for K in pcases.TEAM_SIZES:
        for rows in cases.ROWS:
            ids = pcases.ids(pattern, rows, K)
            count = np.bincount(ids[ids < K], minlength=K)
            assert ids.shape == (rows,) and ids.dtype == np.uint8
            if pattern == "one":
                assert (count > 0).sum() == 1 and count.sum() == rows
            elif pattern == "round_robin":
                assert count.max() - count.min() <= 1 and (rows < 2 or K < 2 or ids[0] != ids[1])
            elif pattern == "blocks":
                assert (np.diff(ids.astype(int)) >= 0).all() and count.sum() == rows
            elif pattern == "empty":
                assert count[0] == 0
            elif pattern.startswith("exact"):
                assert count[0] == min(int(pattern[5:]), rows)
            else:
                assert (ids >= K).any()


@pytest.mark.parametrize("layout", pcases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden,family", cases.EXACT_CASES, ids=cases.EXACT_IDS)
def test_exact_families_pass_the_models_exact_check_for_every_member_on_every_row(kind, hidden, family, layout):
    """the exact tier's weight sets, seeded per member (16 of team 0; two seats: 5 of either team), keep every accumulation free of rounding on every
    row of the case, whichever member an id pattern sends the row to: the device result must be bit-equal"""
    inputs = pcases.case_inputs(family, layout)
    lay = pcases.model_layout(layout)
    seats = [(p, (inputs[0][:, p], inputs[1][:, p]), 5) for p in range(2)] if layout == "seats" else [(0, inputs, 16)]
    for p, x, K in seats:
        for m, params in enumerate(pcases.team(kind, hidden, family, K, p)):
            q, _ = model.forward_layout(lay, params, x, False, exact=True, rounds=family == "rounding")
            assert q.shape[0] == cases.MAX_ROWS
            if family == "nonfinite":                          # the damaged weight sets sit on members 1 and 3: the NaN column is theirs alone
                clean = np.arange(cases.MAX_ROWS) % 7 == 0
                assert np.isnan(q).any() if m in pcases.DAMAGED_MEMBERS else not np.isnan(q[clean]).any()


# ---------------------------------------------------------------------- 2. header, export lists and binding agree
def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_prototypes_argtypes_and_exports_agree():
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_pop_bf16.h")).read()
    assert _lib.POPBF16_EXPORTS == ENTRY_POINTS
    assert not set(ENTRY_POINTS) & set(_lib.EXPORTS + _lib.BF16_EXPORTS + _lib.GRAD_EXPORTS + _lib.LEARN_EXPORTS + _lib.POPLEARN_EXPORTS + _lib.PRIORITY_EXPORTS)
    assert re.findall(r"EVG_API \w+ (evg_[a-z0-9_]+)\s*\(", header) == ENTRY_POINTS
    for other in ("evg.h", "evg_qnet_bf16.h", "evg_pop_learn.h"):                  # the new entry points are declared in the new header alone
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(name + "(" in text for name in ENTRY_POINTS), other
    evg_h = open(os.path.join(ROOT, "include", "evg.h")).read()
    args = lambda text, name: re.sub(r"\s+", " ", re.search(r"EVG_API int %s\s*\((.*?)\);" % name, text, re.S).group(1)).strip()
    strip = lambda a: re.sub(r"/\*.*?\*/", "", a).replace(" ,", ",").strip()
    for new, old in (("evg_population_qnet_bf16", "evg_population_qnet"), ("evg_smart_population_qnet_bf16", "evg_smart_population_qnet")):
        assert strip(args(header, new)) == strip(args(evg_h, old)), new           # the argument list is the fp32 entry point's
    lib = _lib.load_popbf16()
    assert lib.evg_abi_version() == _lib.ABI_VERSION
    vp = C.c_void_p
    assert list(lib.evg_population_qnet_bf16.argtypes) == list(lib.evg_population_qnet.argtypes) == \
        [vp, C.POINTER(_lib.EvgPopulation), C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
    assert list(lib.evg_smart_population_qnet_bf16.argtypes) == list(lib.evg_smart_population_qnet.argtypes) == \
        [vp, C.POINTER(_lib.EvgSmartPopulation), C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
    assert len(_lib.EXPORTS) == 70
    assert _exported(_lib.POPBF16_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.BF16_EXPORTS) | set(ENTRY_POINTS)


def test_the_six_older_libraries_export_what_they_did():
    import everglades_amd
    _lib = everglades_amd._lib
    assert _lib.BF16_EXPORTS == ["evg_smart_qnet_bf16", "evg_minimized_qnet_bf16"]
    learn = set(_lib.EXPORTS) | set(_lib.GRAD_EXPORTS) | set(_lib.LEARN_EXPORTS)
    for path, want in ((_lib.LIB_PATH, set(_lib.EXPORTS)), (_lib.PRIORITY_LIB_PATH, set(_lib.EXPORTS) | set(_lib.PRIORITY_EXPORTS)),
                       (_lib.BF16_LIB_PATH, set(_lib.EXPORTS) | set(_lib.BF16_EXPORTS)), (_lib.GRAD_LIB_PATH, set(_lib.EXPORTS) | set(_lib.GRAD_EXPORTS)),
                       (_lib.LEARN_LIB_PATH, learn), (_lib.POPLEARN_LIB_PATH, learn | set(_lib.POPLEARN_EXPORTS))):
        got = _exported(path)
        assert got == want, path
        assert not any(n.endswith("population_qnet_bf16") for n in got), path


def test_null_descriptors_are_refused_without_a_device_with_the_fp32_text():
    import everglades_amd
    lib = everglades_amd._lib.load_popbf16()
    for new, old in ((lib.evg_population_qnet_bf16, lib.evg_population_qnet), (lib.evg_smart_population_qnet_bf16, lib.evg_smart_population_qnet)):
        assert new(None, None, 0, 1, 0, None, None, None, None, None) == -1
        text = lib.evg_last_error()
        assert old(None, None, 0, 1, 0, None, None, None, None, None) == -1 and lib.evg_last_error() == text and b"null handle" in text


# ---------------------------------------------------------------------- 3. the Python surface's refusals, by text, before anything is touched
def test_precision_and_target_precision_are_refused_by_their_text():
    import torch
    import everglades_amd
    from everglades_amd import population
    for fp32_cls, bf16_cls in ((population.QPopulation, population.QPopulationBf16), (population.SmartQPopulation, population.SmartQPopulationBf16)):
        assert issubclass(bf16_cls, fp32_cls) and [n for n in vars(bf16_cls) if not n.startswith("__")] == []     # _launch alone, from the mixin
        with pytest.raises(ValueError, match=r'precision must be "fp32" or "bf16" \(got \'int8\'\)'):
            population.make(None, [], None, None, None, "int8", fp32_cls, bf16_cls)
    assert [n for n in vars(population._Bf16Forward) if not n.startswith("__")] == ["_launch"]
    net = tuple(torch.zeros(s) for s in ((3, 59), (3,), (3, 3), (3,), (5, 3), (5,)))
    with pytest.raises(ValueError, match='target_precision must be "fp32" or "bf16" or "bf16_grouped"'):
        everglades_amd.PopulationLearner(None, "smart", [net], [net], target_precision="bf16_group")


# ---------------------------------------------------------------------- 4. the new kernels' static resources
def test_grouped_bf16_kernels_have_no_scratch_and_no_spills():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    csrc = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "resource-usage", "FLAGS_EXTRA=-DEVG_BF16 -DEVG_POP_BF16"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    names = sorted(n for n in usage if "pop_bf16_kernel" in n)
    assert len(names) == 4, names                                                   # two families x (expanded, compact)
    for n in names:
        u = usage[n]
        print(n, u)
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
        assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 256 and int(u["Occupancy [waves/SIMD]"]) >= 2, (n, u)     # two wavefronts per SIMD
