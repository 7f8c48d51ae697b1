"""CPU tests (no GPU needed) of the opponent league's entry points: the prototypes include/evg.h declares and the ctypes binding agree, and the two league
forms of the one-seat step kernel fit the budget of the forms they derive from (no scratch, no spills, the same LDS, 2 waves per SIMD)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = {"evg_league_clear": 3, "evg_league_assign": 4, "evg_league_importance": 4, "evg_step_vs_league": 13, "evg_step_vs_league_q": 17}


def _step_kernel_symbol(form, obs_dtype):
    spec = importlib.util.spec_from_file_location("evg_prof", os.path.join(ROOT, "tools", "_prof.py"))
    prof = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(prof)
    return prof.step_kernel_symbol(form, obs_dtype)


def _prototype_arity(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_prototypes_and_ctypes_argtypes_have_the_same_arity():
    import everglades_amd
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    lib = everglades_amd.load_library()
    assert everglades_amd._lib.ABI_VERSION == 7 and "#define EVG_ABI_VERSION 7" in header
    for name, arity in ENTRY_POINTS.items():
        assert name in everglades_amd._lib.EXPORTS, name
        assert _prototype_arity(header, name) == len(getattr(lib, name).argtypes) == arity, name
    # the league forms take the argument lists of the seat forms with the descriptor where opponent_policy stands and no seat
    assert _prototype_arity(header, "evg_step_vs_league") == _prototype_arity(header, "evg_step_vs_policy_smart") - 1
    assert _prototype_arity(header, "evg_step_vs_league_q") == _prototype_arity(header, "evg_step_vs_policy_smart_q") - 1
    # the descriptor: 19 int32, then five pointers (8-byte aligned)
    assert C.sizeof(everglades_amd._lib.EvgLeague) == 80 + 5 * 8
    assert everglades_amd._lib.EvgLeague.weights.offset == 80
    assert everglades_amd.OpponentLeague is not None


def _resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = block.split()[0]
        usage[name] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    return usage


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_league_forms_of_the_seat_kernel_fit_the_seat_kernel_budget():
    usage = _resource_usage()
    for ot in ("float32", "float64", "int16"):
        for base, form in (("seat", "seat_league"), ("seat_q", "seat_q_league")):
            b, f = usage[_step_kernel_symbol(base, ot)], usage[_step_kernel_symbol(form, ot)]
            print(ot, form, f)
            assert f["ScratchSize [bytes/lane]"] == "0" and f["VGPRs Spill"] == "0" and f["SGPRs Spill"] == "0", (ot, form, f)
            assert int(f["LDS Size [bytes/block]"]) <= 20480 and f["LDS Size [bytes/block]"] == b["LDS Size [bytes/block]"], (ot, form, f)
            assert f["Occupancy [waves/SIMD]"] == b["Occupancy [waves/SIMD]"] == "2", (ot, form, f, b)
