"""CPU tests (no GPU needed) of the interface of the agents/DQN family's learner step: include/evg_dqn_learn.h against the ctypes binding and the export
list of libevg_dqnlearn.so, the descriptor's layout, the unchanged neighbour libraries, the refusals of both entry points through the ABI, the new
kernels' static resources, the host-side argument checks of DqnFamilyLearner, and the measured tolerance of the reference fixture."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import dqn_learn_cases as cases
import dqn_learn_fixture as fixture

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = ["evg_dqn_td_head", "evg_adam_step_wide"]


def test_prototypes_ctypes_argtypes_macros_and_exports_agree():
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_dqn_learn.h")).read()
    assert _lib.DQN_LEARN_EXPORTS == ENTRY_POINTS
    assert not set(ENTRY_POINTS) & (set(_lib.EXPORTS) | set(_lib.DQN_EXPORTS) | set(_lib.DQN_GRAD_EXPORTS) | set(_lib.LEARN_EXPORTS))
    assert set(re.findall(r"EVG_API \w+ (evg_[a-z0-9_]+)\s*\(", header)) == set(ENTRY_POINTS)
    for other in ("evg.h", "evg_dqn.h", "evg_dqn_grad.h", "evg_learn.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "evg_dqn_td_head" not in text and "evg_adam_step_wide" not in text
    lib = _lib.load_dqn_learn()
    assert lib.evg_abi_version() == 7
    assert list(lib.evg_dqn_td_head.argtypes) == [C.c_void_p, C.POINTER(_lib.EvgDqnTdHeadArgs), C.c_void_p]
    assert list(lib.evg_adam_step_wide.argtypes) == [C.c_void_p, C.POINTER(_lib.EvgAdamArgs), C.c_void_p]
    for macro, value in (("EVG_DQN_TD_HUBER", _lib.DQN_TD_MODES["huber"]), ("EVG_DQN_TD_SQUARED", _lib.DQN_TD_MODES["squared"]),
                         ("EVG_DQN_TD_ACTIONS", _lib.DQN_TD_ACTIONS), ("EVG_DQN_TD_MAX_BLOCKS", _lib.DQN_TD_MAX_BLOCKS),
                         ("EVG_ADAM_WIDE_MAX_BLOCKS", _lib.ADAM_WIDE_MAX_BLOCKS)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert re.search(r"#define EVG_DQN_TD_MAX_BATCH \(1 << 20\)", header) and _lib.DQN_TD_MAX_BATCH == 1 << 20
    assert re.search(r"#define EVG_DQN_TD_WORKSPACE_BYTES \(4LL \* EVG_DQN_TD_MAX_BLOCKS\)", header) and _lib.DQN_TD_WORKSPACE_BYTES == 4 * _lib.DQN_TD_MAX_BLOCKS

    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert exported(_lib.DQN_LEARN_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.DQN_EXPORTS) | set(_lib.DQN_GRAD_EXPORTS) | set(ENTRY_POINTS)
    assert exported(_lib.DQN_GRAD_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.DQN_EXPORTS) | set(_lib.DQN_GRAD_EXPORTS)
    assert exported(_lib.LEARN_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.GRAD_EXPORTS) | set(_lib.LEARN_EXPORTS)
    assert exported(_lib.LIB_PATH) == set(_lib.EXPORTS)
    assert everglades_amd.DqnFamilyLearner.__name__ == "DqnFamilyLearner" and hasattr(everglades_amd.EvergladesVecEnv, "dqn_learner")


def test_descriptor_layout_matches_the_compiler(tmp_path):
    from everglades_amd import _lib
    fields = [f[0] for f in _lib.EvgDqnTdHeadArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evg_dqn_learn.h"\nint main(void) {\n printf("%%zu %%zu %s\\n", sizeof(evg_dqn_td_head_args), sizeof(evg_adam_args), %s);\n return 0; }\n' % (
        " ".join(["%zu"] * len(fields)), ", ".join("offsetof(evg_dqn_td_head_args, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    d = _lib.EvgDqnTdHeadArgs
    assert got == [C.sizeof(d), C.sizeof(_lib.EvgAdamArgs)] + [getattr(d, f).offset for f in fields] and C.sizeof(d) == 112


def test_refusals_of_both_entry_points_through_the_abi():
    """every refusal is decided before the handle or a pointer is used: a non-NULL handle and an aligned address that nothing dereferences"""
    from everglades_amd import _lib
    G = _lib.load_dqn_learn()
    handle = C.create_string_buffer(1 << 16)
    block = C.create_string_buffer(4096 + 64)
    address = (C.addressof(block) + 63) // 64 * 64
    cases.check_td_refusals(_lib, G, C.addressof(handle), address)
    cases.check_adam_refusals(_lib, G, C.addressof(handle), address)


def test_dqn_learn_kernels_have_no_scratch_and_no_spills():
    """make resource-usage FLAGS_EXTRA="-DEVG_DQN -DEVG_DQN_GRAD -DEVG_DQN_LEARN": the TD head's two kernels and the wide Adam's two -- no scratch, no
    VGPR and no SGPR spills, and the figures DESIGN.md states"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "FLAGS_EXTRA=-DEVG_DQN -DEVG_DQN_GRAD -DEVG_DQN_LEARN"], capture_output=True, text=True,
                         check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    names = sorted(n for n in usage if re.search(r"evg_dqn_td_(head|loss)_kernel|evg_adam_wide_(ctl_)?kernel", n))
    assert len(names) == 4, names
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in names:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
        assert int(u["VGPRs"]) <= 128, (n, u)                          # four wavefronts per SIMD at the least
    td = usage[[n for n in names if "td_head" in n][0]]
    assert int(td["LDS Size [bytes/block]"]) == 64
    assert "%s VGPRs" % td["VGPRs"] in design and "64 bytes of LDS" in design


def test_learner_refuses_bad_arguments_before_anything_is_touched():
    from everglades_amd import dqn_learner, _lib
    ok = dict(mode="huber", clamp=1.0, lr=1e-4, gamma=0.99, betas=(0.9, 0.999), eps=1e-8)
    assert dqn_learner.check_options(**ok) == (0, 1.0)
    assert dqn_learner.check_options(**dict(ok, mode="squared", clamp=None)) == (1, 0.0)
    for key, bad in (("mode", "max_mean"), ("mode", None), ("clamp", 0), ("clamp", -1.0), ("clamp", float("inf")), ("clamp", True), ("clamp", "1"),
                     ("lr", float("nan")), ("lr", "x"), ("gamma", float("inf")), ("eps", 0.0), ("eps", -1e-8), ("betas", (0.9,)), ("betas", (0.9, 1.0)),
                     ("betas", (-0.1, 0.5))):
        with pytest.raises(ValueError, match=key):
            dqn_learner.check_options(**dict(ok, **{key: bad}))
    for B in (0, -1, _lib.DQN_GRAD_MAX_ROWS + 1):
        with pytest.raises(ValueError, match="batch size"):
            dqn_learner.check_batch_size(B)
    assert dqn_learner.check_batch_size(1) == 1 and dqn_learner.check_batch_size(_lib.DQN_GRAD_MAX_ROWS) == 1 << 16


def test_fixture_tolerance_is_twice_the_fp32_host_models_deviation():
    """the figures of tests/dqn_learn_fixture.py are what the fp32 host model measures against tests/golden/dqn_learn.npz, the GPU test's bounds twice
    that, and the fixture leaves out at most 1 % of the elements"""
    fx = fixture.load_fixture()
    worst_p = worst_l = 0.0
    for k, (params, loss) in enumerate(fixture.host_steps(fx)):
        dev_lr, dev_ulps, left_out = fixture.fixture_compare(fx, k, params, loss)
        print("step %d: parameters %.6g lr, loss %.4f ulps, left out %.3f %%" % (k, dev_lr, dev_ulps, 100 * left_out))
        assert left_out <= 0.01
        worst_p, worst_l = max(worst_p, dev_lr), max(worst_l, dev_ulps)
    assert np.isclose(worst_p, fixture.FIXTURE_PARAM_DEV_LR, rtol=1e-6) and np.isclose(worst_l, fixture.FIXTURE_LOSS_DEV_ULPS, rtol=1e-6)
    assert fixture.FIXTURE_PARAM_BOUND_LR == 2 * fixture.FIXTURE_PARAM_DEV_LR and fixture.FIXTURE_LOSS_BOUND_ULPS == 2 * fixture.FIXTURE_LOSS_DEV_ULPS
    z = np.load(os.path.join(ROOT, "tests", "golden", "dqn_learn.npz"))
    assert all(z[k].dtype.kind in "fib" for k in z.files) and os.path.getsize(os.path.join(ROOT, "tests", "golden", "dqn_learn.npz")) < (1 << 20)
