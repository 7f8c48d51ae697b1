"""CPU tests (no GPU needed) of the Minimized agents' entry points: the prototypes include/evg.h declares, the ctypes binding and the export list agree,
the descriptor has the C layout, the ABI stays 7, and the new kernels and step-kernel forms meet their resource conditions in the static build."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = {"evg_minimized_get_action": 8, "evg_step_vs_policy_minimized_q": 17, "evg_step_vs_league_minimized_q": 16, "evg_minimized_qnet": 8}


def _prototype_arity(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_prototypes_ctypes_argtypes_and_exports_agree():
    import everglades_amd
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    lib = everglades_amd.load_library()
    assert everglades_amd._lib.ABI_VERSION == 7 and "#define EVG_ABI_VERSION 7" in header and lib.evg_abi_version() == 7
    for name, arity in ENTRY_POINTS.items():
        assert name in everglades_amd._lib.EXPORTS, name
        assert _prototype_arity(header, name) == len(getattr(lib, name).argtypes) == arity, name
    # the fused forms take the argument lists of their Smart_State counterparts without directions_out
    assert _prototype_arity(header, "evg_step_vs_policy_minimized_q") == _prototype_arity(header, "evg_step_vs_policy_smart_q") - 1
    assert _prototype_arity(header, "evg_step_vs_league_minimized_q") == _prototype_arity(header, "evg_step_vs_league_q") - 1
    for name in ("evg_step_vs_policy_minimized_q", "evg_step_vs_league_minimized_q"):
        assert "directions_out" not in re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header).group(1)
    # the version script exports every evg_* symbol and nothing else
    assert "global: evg_*;" in open(os.path.join(CSRC, "evg.map")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", everglades_amd._lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported and exported == set(everglades_amd._lib.EXPORTS)
    assert "#define EVG_MINI_QNET_MAX_HIDDEN 128" in header and everglades_amd._lib.MINI_QNET_MAX_HIDDEN == 128


def test_descriptor_layout_matches_the_header():
    from everglades_amd import _lib
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    d = _lib.EvgMiniQnet
    assert C.sizeof(d) == 16 + 8 * 8                  # 4 x 4 bytes, then 8 pointers
    assert d.w1.offset == 16 and d.b2.offset == 16 + 6 * 8
    names = [f[0] for f in d._fields_]
    assert names == ["struct_size", "h1", "final_relu", "num_sets", "w1", "b1", "w2", "b2"]
    body = re.search(r"typedef struct evg_mini_qnet \{(.*?)\} evg_mini_qnet;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"\[\d+\]", "", part.split()[-1].lstrip("*")) for part in body.split(";") if part.strip()]
    assert declared == names


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage"], capture_output=True, text=True, check=True)
    u = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        u[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    return u


def _clean(u):
    return u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0"


def test_step_kernel_forms_keep_the_lds_budget_and_two_waves_per_simd(usage):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import _prof
    for form in ("seat_q_min", "seat_q_min_league"):
        for dt in ("float32", "float64", "int16"):
            u = usage[_prof.step_kernel_symbol(form, dt)]
            assert _clean(u), (form, dt, u)
            assert int(u["LDS Size [bytes/block]"]) <= 20208 and int(u["Occupancy [waves/SIMD]"]) == 2, (form, dt, u)
    # ... and the forms there were keep their names
    for form in ("seat_q", "seat_q_league", "two_seat_q", "seat", "single_turn", "persistent"):
        assert _prof.step_kernel_symbol(form) in usage, form


def test_qnet_and_action_kernels_have_no_scratch_and_no_spills(usage):
    for expanded in "01":
        u = usage["_ZN3evg20evg_mini_qnet_kernelILb%sEEEvNS_12MiniQnetArgsE" % expanded]
        assert _clean(u), (expanded, u)
        assert int(u["LDS Size [bytes/block]"]) <= 65536 and int(u["Occupancy [waves/SIMD]"]) >= 2, (expanded, u)
    names = [n for n in usage if "evg_minimized_actions_kernel" in n]
    assert len(names) == 2
    for n in names:
        assert _clean(usage[n]), (n, usage[n])
