"""CPU tests (no GPU needed) of self-royale's entry points: the prototypes include/evg.h declares, the ctypes binding and the export list agree, the
descriptor has the C layout, the ABI stays 7, the grouped kernels meet the resource bounds of the Minimized kernels they share a body with, and those
keep their names."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = {"evg_population_clear": 3, "evg_population_assign": 6, "evg_population_qnet": 10}


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
    assert "global: evg_*;" in open(os.path.join(CSRC, "evg.map")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", everglades_amd._lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported and exported == set(everglades_amd._lib.EXPORTS)
    _lib = everglades_amd._lib
    assert "#define EVG_POP_MAX_MEMBERS 16" in header and _lib.POP_MAX_MEMBERS == 16
    assert "#define EVG_POP_MAX_ROWS (1 << 24)" in header and _lib.POP_MAX_ROWS == 1 << 24
    assert "enum { EVG_POP_S_BAD_MEMBER = 1 };" in header and _lib.POP_S_BAD_MEMBER == 1
    assert hasattr(everglades_amd, "QPopulation") and hasattr(everglades_amd.EvergladesVecEnv, "q_population")
    # RNG domain 6 is the population's, on the device and in the host statement
    rng = open(os.path.join(CSRC, "evg_rng.h")).read()
    assert "RNG_POPULATION = 6" in rng


def test_descriptor_layout_matches_the_header():
    from everglades_amd import _lib
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    d = _lib.EvgPopulation
    assert C.sizeof(d) == 24 + 4 * 2 * 16 * 8 + 7 * 8 + 8          # 6 x 4 bytes, four [2][16] pointer tables, 7 pointers, scratch_rows
    assert d.num_members.offset == 12 and d.w1.offset == 24 and d.b2.offset == 24 + 3 * 256 and d.member.offset == 24 + 1024
    assert d.scratch_rows.offset == C.sizeof(d) - 8
    names = [f[0] for f in d._fields_]
    assert names == ["struct_size", "h1", "final_relu", "num_members", "reserved", "w1", "b1", "w2", "b2", "member", "counts", "ctl", "index", "first",
                     "count", "hist", "scratch_rows"]
    body = re.search(r"typedef struct evg_population \{(.*?)\} evg_population;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"\[\w+\]", "", part.split()[-1].lstrip("*")) for part in body.split(";") if part.strip()]
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


def test_grouped_kernels_meet_the_bounds_of_the_minimized_kernels(usage):
    for expanded in "01":
        u = usage["_ZN3evg24evg_mini_qnet_pop_kernelILb%sEEEvNS_11MiniPopArgsE" % expanded]
        assert _clean(u), (expanded, u)
        assert int(u["LDS Size [bytes/block]"]) <= 65536 and int(u["Occupancy [waves/SIMD]"]) >= 2, (expanded, u)
    # ... and the two kernels there were keep their names
    for expanded in "01":
        assert "_ZN3evg20evg_mini_qnet_kernelILb%sEEEvNS_12MiniQnetArgsE" % expanded in usage


def test_side_kernels_have_no_scratch_and_no_spills(usage):
    names = [n for n in usage if "evg_population_" in n]
    assert len(names) == 5, names
    for n in names:
        assert _clean(usage[n]), (n, usage[n])
