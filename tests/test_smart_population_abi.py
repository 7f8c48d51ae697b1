"""CPU tests (no GPU needed) of Smart_State self-royale's entry points: the prototypes include/evg.h declares, the ctypes binding and the export list
agree, the descriptor has the C layout, the ABI stays 7, and the refusals that need no device (a NULL handle, a NULL descriptor) are refusals.  The
refusals that need a handle are in tests/test_gpu_smart_population.py."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = {"evg_smart_population_clear": 3, "evg_smart_population_assign": 6, "evg_smart_population_qnet": 10}
FIELDS = ["struct_size", "h1", "h2", "final_relu", "num_members", "w1", "b1", "w2", "b2", "w3", "b3", "member", "counts", "ctl", "index", "first",
          "count", "hist", "scratch_rows"]


def _prototype_arity(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_prototypes_ctypes_argtypes_and_exports_agree():
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    lib = everglades_amd.load_library()
    assert _lib.ABI_VERSION == 7 and "#define EVG_ABI_VERSION 7" in header and lib.evg_abi_version() == 7
    for name, arity in ENTRY_POINTS.items():
        assert name in _lib.EXPORTS, name
        assert _prototype_arity(header, name) == len(getattr(lib, name).argtypes) == arity, name
    # the Smart_State entry points take their arguments in the order of the Minimized ones
    for name in ENTRY_POINTS:
        twin = name.replace("smart_", "")
        assert [t for t in getattr(lib, name).argtypes[2:]] == [t for t in getattr(lib, twin).argtypes[2:]], name
    assert "global: evg_*;" in open(os.path.join(CSRC, "evg.map")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported and exported == set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == 70
    assert hasattr(everglades_amd, "SmartQPopulation") and hasattr(everglades_amd.EvergladesVecEnv, "smart_q_population")
    assert issubclass(everglades_amd.SmartQPopulation, everglades_amd.QPopulation) and everglades_amd.SmartQPopulation.OUT == 5
    assert everglades_amd.QPopulation.OUT == 11 and everglades_amd.QPopulation._DESC is _lib.EvgPopulation
    # the header says what two populations on one handle draw
    assert "TWO\n * POPULATIONS ON ONE HANDLE DRAW THE SAME MEMBERS" in header


def test_descriptor_layout_matches_the_header():
    from everglades_amd import _lib
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    d = _lib.EvgSmartPopulation
    assert C.sizeof(d) == 24 + 6 * 2 * 16 * 8 + 7 * 8 + 8           # 6 x 4 bytes, six [2][16] pointer tables, 7 pointers, scratch_rows
    assert d.h1.offset == 4 and d.h2.offset == 8 and d.final_relu.offset == 12 and d.num_members.offset == 16
    for i, name in enumerate(("w1", "b1", "w2", "b2", "w3", "b3")):
        assert getattr(d, name).offset == 24 + 256 * i and getattr(d, name).size == 256, name
    for i, name in enumerate(("member", "counts", "ctl", "index", "first", "count", "hist", "scratch_rows")):
        assert getattr(d, name).offset == 24 + 6 * 256 + 8 * i, name
    assert d.scratch_rows.offset == C.sizeof(d) - 8
    names = [f[0] for f in d._fields_]
    assert names == FIELDS
    body = re.search(r"typedef struct evg_smart_population \{(.*?)\} evg_smart_population;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for part in body.split(";"):
        if part.strip():                                           # "int32_t h1, h2" declares two fields
            first, *more = part.split(",")
            declared.append(re.sub(r"\[\w+\]", "", first.split()[-1].lstrip("*")))
            declared += [re.sub(r"\[\w+\]", "", m.strip().lstrip("*")) for m in more]
    assert declared == names
    # the part the assignment kernels read lies where a shared struct would put it: the same fields, in evg_population's order, after the weights
    mini = [f[0] for f in _lib.EvgPopulation._fields_]
    assert names[names.index("member"):] == mini[mini.index("member"):]
    assert "#define EVG_QNET_MAX_HIDDEN 64" in header and _lib.QNET_MAX_HIDDEN == 64


def test_refusals_that_need_no_device():
    import everglades_amd
    _lib = everglades_amd._lib
    lib = everglades_amd.load_library()
    d = _lib.EvgSmartPopulation()
    d.struct_size = C.sizeof(d)
    d.h1 = d.h2 = 60
    d.num_members[0] = d.num_members[1] = 4
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # a NULL handle, whatever else is passed
    assert lib.evg_smart_population_clear(None, C.byref(d), None) == _lib.ERR_ARG
    assert b"null handle" in lib.evg_last_error()
    assert lib.evg_smart_population_assign(None, C.byref(d), None, None, None, None) == _lib.ERR_ARG
    for layout in (_lib.QNET_COMPACT, _lib.QNET_COMPACT_SEATS, _lib.QNET_EXPANDED):
        assert lib.evg_smart_population_qnet(None, C.byref(d), layout, 1, 0, p, p, p, p, None) == _lib.ERR_ARG
    assert lib.evg_smart_population_qnet(None, None, _lib.QNET_EXPANDED, 1, 0, p, p, None, p, None) == _lib.ERR_ARG
    assert lib.evg_smart_population_clear(None, None, None) == _lib.ERR_ARG
    assert lib.evg_smart_population_assign(None, None, None, None, None, None) == _lib.ERR_ARG
