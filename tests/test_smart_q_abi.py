"""CPU tests (no GPU needed) of evg_step_vs_policy_smart_q, the Smart_State learner's turn from its Q values: the prototype include/evg.h declares and the
ctypes binding agree, and the kernel instantiation it launches fits the budget of the one-seat kernel it is a form of (no scratch, the same LDS and occupancy)."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")


def _step_kernel_symbol(form, obs_dtype):
    """tools/_prof.py knows the symbol of a step-kernel form"""
    spec = importlib.util.spec_from_file_location("evg_prof", os.path.join(ROOT, "tools", "_prof.py"))
    prof = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(prof)
    return prof.step_kernel_symbol(form, obs_dtype)


def _prototype_arity(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_prototype_and_ctypes_argtypes_have_the_same_arity():
    import everglades_amd
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    lib = everglades_amd.load_library()
    assert "evg_step_vs_policy_smart_q" in everglades_amd._lib.EXPORTS
    assert everglades_amd._lib.ABI_VERSION == 7 and "#define EVG_ABI_VERSION 7" in header
    assert _prototype_arity(header, "evg_step_vs_policy_smart_q") == len(lib.evg_step_vs_policy_smart_q.argtypes) == 18
    for name in ("evg_step_vs_policy_smart", "evg_smart_get_action", "evg_step_vs_policy"):
        assert _prototype_arity(header, name) == len(getattr(lib, name).argtypes), name


def _resource_usage():
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = block.split()[0]
        usage[name] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    return usage


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_q_form_of_the_seat_kernel_fits_the_seat_kernel_budget():
    usage = _resource_usage()
    for ot in ("float32", "float64", "int16"):
        seat = usage[_step_kernel_symbol("seat", ot)]
        qform = usage[_step_kernel_symbol("seat_q", ot)]
        assert qform["ScratchSize [bytes/lane]"] == "0" and qform["VGPRs Spill"] == "0" and qform["SGPRs Spill"] == "0", (ot, qform)
        assert int(qform["LDS Size [bytes/block]"]) <= 20480 and qform["LDS Size [bytes/block]"] == seat["LDS Size [bytes/block]"], (ot, qform)
        assert qform["Occupancy [waves/SIMD]"] == seat["Occupancy [waves/SIMD]"] == "2", (ot, qform, seat)
