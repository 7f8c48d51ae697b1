"""CPU tests (no GPU needed) of the agents/DQN entry points' interface: include/evg_dqn.h against the ctypes binding and the export list of libevg_dqn.so,
the descriptor's layout, the unchanged product library, the new kernels' static resources, and the host-side refusals of everglades_amd/dqn.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = ["evg_dqn_qnet", "evg_dqn_actions", "evg_dqn_get_action"]
C_TYPES = {"evg_handle*": C.c_void_p, "const evg_dqn_net*": "net", "int": C.c_int, "int64_t": C.c_int64, "const void*": C.c_void_p, "float*": C.c_void_p,
           "void*": C.c_void_p, "const float*": C.c_void_p, "int32_t*": C.c_void_p, "float": C.c_float, "uint8_t*": C.c_void_p}


def _prototype_args(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototypes_ctypes_argtypes_and_exports_agree():
    """The three entry points live in include/evg_dqn.h and libevg_dqn.so (the product's sources with -DEVG_DQN); libevg.so and include/evg.h keep
    exactly the entry points they had, and the ABI is still 7."""
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_dqn.h")).read()
    main_header = open(os.path.join(ROOT, "include", "evg.h")).read()
    assert _lib.DQN_EXPORTS == ENTRY_POINTS and not set(ENTRY_POINTS) & set(_lib.EXPORTS)
    assert set(re.findall(r"EVG_API \w+ (evg_[a-z0-9_]+)\s*\(", header)) == set(ENTRY_POINTS)
    assert "evg_dqn" not in main_header and "#define EVG_ABI_VERSION 7" in main_header and _lib.ABI_VERSION == 7
    lib = _lib.load_dqn()
    assert lib.evg_abi_version() == 7
    for name in ENTRY_POINTS:
        args = _prototype_args(header, name)
        types = [a.rsplit(" ", 1)[0] for a in args]
        want = [C.POINTER(_lib.EvgDqnNet) if C_TYPES[t] == "net" else C_TYPES[t] for t in types]
        assert list(getattr(lib, name).argtypes) == want, (name, args)
    # evg_dqn_get_action takes evg_minimized_get_action's argument list
    assert _prototype_args(header, "evg_dqn_get_action") == _prototype_args(main_header, "evg_minimized_get_action")
    assert list(lib.evg_dqn_get_action.argtypes) == list(lib.evg_minimized_get_action.argtypes)

    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert exported(_lib.DQN_LIB_PATH) == set(_lib.EXPORTS) | set(ENTRY_POINTS)
    assert exported(_lib.LIB_PATH) == set(_lib.EXPORTS)
    for name, value in (("EVG_DQN_IN", _lib.DQN_IN), ("EVG_DQN_OUT", _lib.DQN_OUT), ("EVG_DQN_MAX_HIDDEN", _lib.DQN_MAX_HIDDEN), ("EVG_DQN_CHUNK", _lib.DQN_CHUNK),
                        ("EVG_DQN_TINY_ROWS", _lib.DQN_TINY_ROWS), ("EVG_DQN_SMALL_ROWS", _lib.DQN_SMALL_ROWS), ("EVG_DQN_MAX_BLOCKS", _lib.DQN_MAX_BLOCKS), ("EVG_DQN_ROWS", _lib.DQN_ROWS),
                        ("EVG_DQN_OBS_SEAT", _lib.DQN_OBS_SEAT), ("EVG_DQN_OBS", _lib.DQN_OBS)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (_lib.DQN_IN, _lib.DQN_OUT, _lib.DQN_MAX_HIDDEN) == (105, 132, 528)
    assert hasattr(everglades_amd, "DqnQNet") and all(hasattr(everglades_amd.EvergladesVecEnv, n) for n in ("dqn_qnet", "dqn_actions", "dqn_get_action"))


def test_descriptor_layout_matches_the_compiler(tmp_path):
    from everglades_amd import _lib
    src = tmp_path / "layout.c"
    fields = ["struct_size", "h1", "final_relu", "reserved", "w1", "b1", "w2", "b2"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evg_dqn.h"\nint main(void) { printf("%%zu %s\\n", sizeof(evg_dqn_net), %s); return 0; }\n' % (
        " ".join(["%zu"] * len(fields)), ", ".join("offsetof(evg_dqn_net, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    d = _lib.EvgDqnNet
    assert [f[0] for f in d._fields_] == fields
    assert got == [C.sizeof(d)] + [getattr(d, f).offset for f in fields] and C.sizeof(d) == 48


def test_dqn_kernels_have_no_scratch_and_no_spills_and_the_lds_design_states():
    """make resource-usage FLAGS_EXTRA=-DEVG_DQN: the two network kernels per observation type and the two decode kernels -- no scratch, no VGPR and no
    SGPR spills, and the LDS sizes and occupancies DESIGN.md section 3 states."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "FLAGS_EXTRA=-DEVG_DQN"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    nets = sorted(n for n in usage if "evg_dqn_qnet_kernel" in n or "evg_dqn_qnet_rows16_kernel" in n)
    heads = sorted(n for n in usage if "evg_dqn_actions_kernel" in n)
    assert len(nets) == 9 and len(heads) == 2, (nets, heads)        # float, double, int16 x (16-row, one group, four groups); greedy, exploring
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in nets + heads:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
        if n in heads:
            lds = 35360
        else:
            lds, occupancy = (53312, 3) if "rows16" in n else (62912, 2) if "Li1EEE" in n else (101312, 1)
            assert int(u["Occupancy [waves/SIMD]"]) == occupancy, (n, u)
            assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 512 // occupancy, (n, u)
            assert "%d wavefront%s per SIMD" % (occupancy, "s" if occupancy > 1 else "") in design
        assert int(u["LDS Size [bytes/block]"]) == lds, (n, u)
        assert "{:,}".format(lds).replace(",", " ") in design, lds


def test_host_side_refusals_need_no_device():
    import torch
    from everglades_amd import dqn
    w1, b1, w2, b2 = torch.zeros(48, 105), torch.zeros(48), torch.zeros(132, 48), torch.zeros(132)
    assert dqn.check_shapes([t.shape for t in (w1, b1, w2, b2)]) == 48
    assert dqn.check_shapes([(528, 105), (528,), (132, 528), (132,)]) == 528
    for bad in ([(529, 105), (529,), (132, 529), (132,)], [(0, 105), (0,), (132, 0), (132,)], [(48, 59), (48,), (132, 48), (132,)],
                [(48, 105), (48,), (11, 48), (11,)], [(48, 105), (47,), (132, 48), (132,)], [(48, 105), (48,), (132, 47), (132,)]):
        with pytest.raises(ValueError):
            dqn.check_shapes(bad)
    with pytest.raises(ValueError, match="hidden|h1"):                          # the wrong hidden size, before anything of the env is touched
        dqn.DqnQNet(None, (torch.zeros(529, 105), torch.zeros(529), torch.zeros(132, 529), b2), final_relu=True)
    with pytest.raises(ValueError, match="4 tensors"):                           # the wrong tuple length
        dqn.DqnQNet(None, (w1, b1, w2), final_relu=True)
    with pytest.raises(ValueError, match="4 tensors"):
        dqn.DqnQNet(None, (w1, b1, w2, b2, w2, b2), final_relu=True)
    with pytest.raises(ValueError, match="final_relu"):
        dqn.DqnQNet(None, (w1, b1, w2, b2))
    seq = torch.nn.Sequential(torch.nn.Linear(105, 16), torch.nn.ReLU(), torch.nn.Linear(16, 132))
    with pytest.raises(ValueError, match="contradicts"):
        dqn.DqnQNet(None, seq, final_relu=True)
    with pytest.raises(ValueError):
        dqn.DqnQNet(None, torch.nn.Sequential(torch.nn.Linear(105, 16), torch.nn.Linear(16, 132)))
    src, final_relu = dqn._param_source(seq, None)
    assert final_relu is False and [tuple(t.shape) for t in src()] == [(16, 105), (16,), (132, 16), (132,)]

    class Ref(torch.nn.Module):                                                  # the reference's QNetwork: fc1 / fc2, final ReLU on
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2 = torch.nn.Linear(105, 528), torch.nn.Linear(528, 132)

    src, final_relu = dqn._param_source(Ref(), None)
    assert final_relu is True and dqn.check_shapes([t.shape for t in src()]) == 528
    assert np.dtype(np.float32).itemsize * (105 * 528 + 528 * 132) == 500544       # the 501 KB that fit neither LDS nor registers
