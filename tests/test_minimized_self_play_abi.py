"""CPU tests (no GPU needed) of the Minimized self-play entry points evg_step_minimized_q / evg_step_league_minimized_q: the prototypes include/evg.h
declares, the ctypes binding and the export list agree, the ABI stays 7, the two new step-kernel forms meet the seat forms' resource conditions in the
static build -- and the host model shows that the league the GPU test of the second entry point plays does what that test relies on."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import league_model as lm
import minimized_self_play_cases as cases
from conftest import ROOT

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
ENTRY_POINTS = {"evg_step_minimized_q": 16, "evg_step_league_minimized_q": 18}


def _prototype(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_prototypes_ctypes_argtypes_and_exports_agree():
    import everglades_amd
    header = open(os.path.join(ROOT, "include", "evg.h")).read()
    lib = everglades_amd.load_library()
    assert everglades_amd._lib.ABI_VERSION == 7 and "#define EVG_ABI_VERSION 7" in header and lib.evg_abi_version() == 7
    for name, arity in ENTRY_POINTS.items():
        assert name in everglades_amd._lib.EXPORTS, name
        assert len(_prototype(header, name)) == len(getattr(lib, name).argtypes) == arity, name
    # the two-seat turn takes evg_step_smart_q's argument list without directions_out, in its order
    smart = [re.sub(r"\s+", " ", a) for a in _prototype(header, "evg_step_smart_q")]
    mini = [re.sub(r"\s+", " ", a) for a in _prototype(header, "evg_step_minimized_q")]
    assert "int32_t* directions_out" in smart and mini == [a for a in smart if a != "int32_t* directions_out"]
    # ... and its league form adds the descriptor and the network member in front of the outputs
    lg = [re.sub(r"\s+", " ", a) for a in _prototype(header, "evg_step_league_minimized_q")]
    assert lg == mini[:5] + ["const evg_league* lg", "int q_member"] + mini[5:]
    out = subprocess.check_output(["nm", "-D", "--defined-only", everglades_amd._lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRY_POINTS) <= exported and exported == set(everglades_amd._lib.EXPORTS)
    assert len(everglades_amd._lib.EXPORTS) == len(set(everglades_amd._lib.EXPORTS))


@pytest.fixture(scope="module")
def usage():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage"], capture_output=True, text=True, check=True)
    u = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        u[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    return u


def test_two_seat_forms_keep_the_lds_budget_and_two_waves_per_simd(usage):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import _prof
    for form in ("two_seat_q_min", "two_seat_q_min_league"):
        for dt in ("float32", "float64", "int16"):
            u = usage[_prof.step_kernel_symbol(form, dt)]
            assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (form, dt, u)
            assert int(u["LDS Size [bytes/block]"]) <= 20208 and int(u["Occupancy [waves/SIMD]"]) == 2, (form, dt, u)
    # ... and every form name there was still resolves to a kernel of the build
    for form in ("single_turn", "persistent", "chunked", "stock_entropy", "seat", "seat_q", "two_seat_q", "seat_league", "seat_q_league", "seat_q_min",
                 "seat_q_min_league"):
        for dt in ("float32", "float64", "int16"):
            assert _prof.step_kernel_symbol(form, dt) in usage, (form, dt)


# ---------------------------------------------------------------------------------------------- the league of the GPU test, on the host model alone
@pytest.mark.parametrize("N", cases.SIZES)
@pytest.mark.parametrize("seat", [0, 1])
def test_the_gpu_test_league_uses_every_member_and_returns_to_the_network(N, seat):
    """What tests/test_gpu_minimized_self_play.py relies on, so that it cannot pass vacuously: with its seed and weights every member of non-zero weight is
    played (the network member "q" among them), the zero-weight member never, and within the episodes the test plays (at least cases.EPISODES per env: its
    turn count over the longest game) some env leaves "q" for a bot and comes back to it."""
    h = cases.model_histories(N, seat)
    q = cases.MEMBERS.index("q")
    zero = [m for m, w in enumerate(cases.WEIGHTS) if w == 0.0]
    assert len(zero) == 1 and all(zero[0] not in a for a in h)
    assert {x for a in h for x in a} == set(range(len(cases.MEMBERS))) - set(zero)
    assert all(len(a) == cases.EPISODES for a in h)
    back = [a for a in h if any(a[i] == q and a[j] != q and a[k] == q for i in range(len(a)) for j in range(i + 1, len(a)) for k in range(j + 1, len(a)))]
    assert back, "no env leaves the network member and returns to it"
    # the repeated bot id is two members: both are played
    rep = [m for m, name in enumerate(cases.MEMBERS) if cases.MEMBERS.count(name) > 1]
    assert len(rep) == 2 and all(any(m in a for a in h) for m in rep)


def test_the_league_class_accepts_one_network_member():
    """OpponentLeague's bookkeeping of "q" (no device needed: the constructor's checks run before anything is allocated)"""
    import everglades_amd
    from everglades_amd import _lib

    class _Env(object):
        POLICIES = everglades_amd.EvergladesVecEnv.POLICIES
        num_envs = 4
    with pytest.raises(ValueError):
        everglades_amd.OpponentLeague(_Env(), ["q", "swarm_agent", "q"])
    assert _lib.POLICY_NAMES[12] == "no_action" and "EVG_POLICY_NO_ACTION = 12" in open(os.path.join(ROOT, "include", "evg.h")).read()
