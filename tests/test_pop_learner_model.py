"""CPU tests of the population learner (tests/pop_learner_model.py, include/evg_pop_learn.h, everglades_amd.PopulationLearner): the composed model
against the plain ones, header / binding / export agreement of libevg_poplearn.so, the three older libraries' export sets, the new kernels' static
resources, and the constructor's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import learner_cases as cases
import learner_model as model
import pop_learner_cases as pcases
import pop_learner_model as pmodel
import qnet_grad_cases as gcases
import qnet_grad_model

ENTRY_POINTS = ["evg_pop_learn_expand_ids", "evg_pop_learn_take_rows", "evg_td_head_grouped", "evg_smart_population_backward", "evg_population_backward", "evg_adam_step_grouped"]


# ---------------------------------------------------------------------- 1. the model is the plain models, per member
@pytest.mark.parametrize("mode", model.MODES)
def test_one_member_batch_is_the_plain_td_head(mode):
    c = cases.td_random(259, 5, mode, True)
    ids = np.zeros(259, np.uint8)
    got, E = pmodel.td_head(c, ids, 1)
    want, wE = model.td_head(**c)
    for k in ("gq", "priorities", "estimated"):
        assert np.array_equal(got[k], want[k]) and np.array_equal(E[k], wE[k])
    assert got["loss"][0] == want["loss"] and E["loss"][0] == wE["loss"]
    got32, want32 = pmodel.td_head32(c, ids, 1), model.td_head32(**c)
    assert all(cases.same_bits(got32[k], want32[k]) for k in ("gq", "priorities", "estimated")) and cases.same_bits(got32["loss"][0], want32["loss"])


def test_members_get_the_plain_models_on_their_gathered_rows_and_nobody_gets_zeros():
    B, K = 259, 4
    c = cases.td_random(B, 11, "double_mean", True)
    ids = pcases.ids(B, K, nobody=0.2)
    assert (ids >= K).any() and all(len(R) for R in pmodel.rows_of(ids, K))
    got, E = pmodel.td_head(c, ids, K)
    got32 = pmodel.td_head32(c, ids, K)
    for m, R in enumerate(pmodel.rows_of(ids, K)):
        want, _ = model.td_head(**pmodel.take(c, R))
        assert np.array_equal(got["gq"][R], want["gq"]) and got["loss"][m] == want["loss"]
        assert np.abs(want["gq"]).sum() > 0                                         # ... divided by c_m, not by B
        ok, ratio = cases.within(got32["loss"][m], got["loss"][m], E["loss"][m])
        assert ok, ratio
    nobody = ids >= K
    for k in ("gq", "priorities", "estimated"):
        assert not got[k][nobody].any() and not got32[k][nobody].any() and not E[k][nobody].any()
    # the loss of a member is the sum over its rows: deleting the rows of nobody changes nothing, bit for bit
    keep = np.flatnonzero(~nobody)
    alone = pmodel.td_head32(pmodel.take(c, keep), ids[keep], K)
    assert cases.same_bits(alone["loss"], got32["loss"]) and cases.same_bits(alone["gq"], got32["gq"][keep])


@pytest.mark.parametrize("kind", ["smart", "mini"])
def test_backward_per_member_is_the_plain_backward_and_an_empty_member_gets_zeros(kind):
    hidden = pcases.HIDDEN[kind][1]
    B, K = 65, 4
    team = pcases.random_team(kind, hidden, K)
    x, gq = gcases.inputs(kind, hidden, "dense", B)
    ids = pcases.ids(B, K - 1)                                                      # member K - 1 has no row
    grads, bounds = pmodel.backward(x, team, pcases.final_relu(kind), gq, ids, clamp=1.0)
    for m, R in enumerate(pmodel.rows_of(ids, K)):
        if m == K - 1:
            assert all(not g.any() and not e.any() and g.shape == p.shape for g, e, p in zip(grads[m], bounds[m], team[m]))
            continue
        want, wE = qnet_grad_model.backward(x[R], team[m], pcases.final_relu(kind), gq[R], clamp=1.0)
        assert all(np.array_equal(g, w.reshape(g.shape)) and np.array_equal(e, b.reshape(e.shape)) for g, w, e, b in zip(grads[m], want, bounds[m], wE))
    assert pmodel.roundings(gcases.sizes(kind, hidden), ids, K)[K - 1] is None
    assert pmodel.roundings(gcases.sizes(kind, hidden), ids, K)[0][0] == len(pmodel.rows_of(ids, K)[0])


@pytest.mark.parametrize("kind", ["smart", "mini"])
@pytest.mark.parametrize("B,K", pcases.SHAPES)
def test_exact_tier_operands_cannot_round_for_any_member(kind, B, K):
    """what the GPU exact tier runs: the model's exact mode accepts every member's rows"""
    hidden = pcases.HIDDEN[kind][0 if B != 257 else 1]
    ids = pcases.ids(B, K, nobody=0.1 if B > 16 else 0.0)
    x, gq = gcases.inputs(kind, hidden, "integer", B)
    pmodel.backward(x, pcases.exact_team(kind, hidden, K), pcases.final_relu(kind), gq, ids, exact=True)
    pmodel.td_head(cases.td_exact(B, gcases.OUT[kind], "max_mean", True), ids, K, exact=True)


def test_adam_leaves_a_member_without_rows_alone():
    params, grads = cases.adam_case("smart", (3, 3))
    z = [np.zeros_like(p) for p in params]
    ctl = (7, 0.9 ** 7, 0.999 ** 7)
    out = pmodel.adam([params, params], [grads(0), grads(0)], [z, z], [z, z], [ctl, ctl], [5, 0], lr=1e-3)
    (p0, _, _, c0), _ = out[0]
    (p1, m1, v1, c1), (E1, _, _) = out[1]
    assert c0[0] == 8 and c1 == ctl and all(np.array_equal(a, b) for a, b in zip(p1, params)) and not any(e.any() for e in E1)
    assert any(not np.array_equal(a, b) for a, b in zip(p0, params)) and not any(a.any() for a in m1 + v1)


# ---------------------------------------------------------------------- 2. header, export lists and binding agree
def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_prototypes_structs_macros_and_exports_agree():
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_pop_learn.h")).read()
    assert _lib.POPLEARN_EXPORTS == ENTRY_POINTS and not set(ENTRY_POINTS) & set(_lib.EXPORTS + _lib.GRAD_EXPORTS + _lib.LEARN_EXPORTS)
    assert set(re.findall(r"EVG_API \w+ (evg_[a-z0-9_]+)\s*\(", header)) == set(ENTRY_POINTS)
    for other in ("evg.h", "evg_learn.h", "evg_qnet_grad.h"):                       # the new entry points are declared in the new header alone
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(name + "(" in text for name in ENTRY_POINTS), other
    assert "#define EVG_POP_LEARN_MAX_PARTIALS (EVG_QNET_GRAD_MAX_BLOCKS + EVG_POP_MAX_MEMBERS)" in header
    assert _lib.POP_LEARN_MAX_PARTIALS == _lib.QNET_GRAD_MAX_BLOCKS + _lib.POP_MAX_MEMBERS
    assert "#define EVG_TD_HEAD_GROUPED_WORKSPACE_BYTES (4LL * EVG_TD_HEAD_MAX_BLOCKS * EVG_POP_MAX_MEMBERS)" in header
    assert _lib.TD_HEAD_GROUPED_WORKSPACE_BYTES == _lib.TD_HEAD_WORKSPACE_BYTES * _lib.POP_MAX_MEMBERS
    assert int(re.search(r"#define EVG_POP_LEARN_MAX_TENSORS (\d+)", header).group(1)) == _lib.POP_LEARN_MAX_TENSORS == _lib.ADAM_MAX_TENSORS
    for struct, name in ((_lib.EvgPopLists, "evg_pop_lists"), (_lib.EvgTdHeadGroupedArgs, "evg_td_head_grouped_args"),
                         (_lib.EvgPopBackwardArgs, "evg_pop_backward_args"), (_lib.EvgAdamGroupedArgs, "evg_adam_grouped_args")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)(?:\[\w+\])*\s*(?:,|$)", decl.strip().replace("*", " "))]
        assert fields == [n for n, _ in struct._fields_], (name, fields)
    assert C.sizeof(_lib.EvgPopLists) == 32 and C.sizeof(_lib.EvgTdHeadGroupedArgs) == 8 + 128 + 32
    assert C.sizeof(_lib.EvgPopBackwardArgs) == 24 + 32 + 16 + 2 * 6 * 16 * 8 + 16
    assert C.sizeof(_lib.EvgAdamGroupedArgs) == 40 + 16 + 48 + 4 * 6 * 16 * 8 < 4096  # (it is a kernel argument's worth of pointers)
    lib = _lib.load_poplearn()
    assert lib.evg_abi_version() == _lib.ABI_VERSION
    assert list(lib.evg_td_head_grouped.argtypes) == [C.c_void_p, C.POINTER(_lib.EvgTdHeadGroupedArgs), C.c_void_p]
    assert list(lib.evg_smart_population_backward.argtypes) == list(lib.evg_population_backward.argtypes) == \
        [C.c_void_p, C.POINTER(_lib.EvgPopBackwardArgs), C.c_void_p]
    assert list(lib.evg_adam_step_grouped.argtypes) == [C.c_void_p, C.POINTER(_lib.EvgAdamGroupedArgs), C.c_void_p]
    assert list(lib.evg_pop_learn_expand_ids.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    assert list(lib.evg_pop_learn_take_rows.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p,
                                                          C.c_void_p]
    assert _exported(_lib.POPLEARN_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.GRAD_EXPORTS) | set(_lib.LEARN_EXPORTS) | set(ENTRY_POINTS)


def test_the_three_older_libraries_export_what_they_did():
    import everglades_amd
    _lib = everglades_amd._lib
    assert _lib.GRAD_EXPORTS == ["evg_smart_qnet_backward", "evg_minimized_qnet_backward"] and _lib.LEARN_EXPORTS == ["evg_td_head", "evg_adam_step"]
    assert _exported(_lib.LIB_PATH) == set(_lib.EXPORTS)
    assert _exported(_lib.GRAD_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.GRAD_EXPORTS)
    assert _exported(_lib.LEARN_LIB_PATH) == set(_lib.EXPORTS) | set(_lib.GRAD_EXPORTS) | set(_lib.LEARN_EXPORTS)
    assert not any("pop_learn" in n or "grouped" in n or n.endswith("population_backward") for n in _exported(_lib.LEARN_LIB_PATH))


def test_null_and_malformed_descriptors_are_refused_without_a_device():
    import everglades_amd
    _lib = everglades_amd._lib
    lib = _lib.load_poplearn()
    assert lib.evg_td_head_grouped(None, None, None) != 0 and b"null handle" in lib.evg_last_error()
    assert lib.evg_smart_population_backward(None, None, None) != 0 and lib.evg_population_backward(None, None, None) != 0
    assert lib.evg_adam_step_grouped(None, None, None) != 0 and b"null handle" in lib.evg_last_error()
    assert lib.evg_pop_learn_expand_ids(None, None, 1, 12, None, None) != 0
    assert lib.evg_pop_learn_take_rows(None, None, None, 0, 1, 12, 5, None, None) != 0 and b"take rows: null handle" in lib.evg_last_error()


# ---------------------------------------------------------------------- 3. the constructor's refusals, by text, before anything is touched
def test_population_learner_refuses_bad_arguments_before_anything_is_touched():
    import torch
    import everglades_amd
    PL = everglades_amd.PopulationLearner
    net = lambda h1, h2: tuple(torch.zeros(s) for s in ((h1, 59), (h1,), (h2, h1), (h2,), (5, h2), (5,)))
    with pytest.raises(ValueError, match="kind must be"):
        PL(None, "blind", [net(3, 3)], [net(3, 3)])
    with pytest.raises(ValueError, match="mode must be one of"):
        PL(None, "smart", [net(3, 3)], [net(3, 3)], mode="mean_max")
    with pytest.raises(ValueError, match=r"a team has 1\.\.16 members"):
        PL(None, "smart", [], [])
    with pytest.raises(ValueError, match=r"a team has 1\.\.16 members"):
        PL(None, "smart", [net(3, 3)] * 17, [net(3, 3)] * 17)
    with pytest.raises(ValueError, match="as many targets as policies"):
        PL(None, "smart", [net(3, 3)] * 2, [net(3, 3)])
    with pytest.raises(ValueError, match="one network, not a pair"):
        PL(None, "smart", [(net(3, 3), net(3, 3))], [net(3, 3)])
    with pytest.raises(ValueError, match="all members share the hidden size"):
        PL(None, "smart", [net(3, 3), net(3, 4)], [net(3, 3), net(3, 3)])
    with pytest.raises(ValueError, match="all members share the hidden size"):
        PL(None, "minimized", [net(3, 3)[:4], net(4, 3)[:4]], [net(3, 3)[:4]] * 2)
    with pytest.raises(ValueError, match="lists of networks"):
        PL(None, "smart", net(3, 3)[0], [net(3, 3)])
    with pytest.raises(ValueError, match='target_precision must be "fp32" or "bf16"'):
        PL(None, "smart", [net(3, 3)], [net(3, 3)], target_precision="fp16")
    with pytest.raises(ValueError, match="n_step must be"):
        PL(None, "smart", [net(3, 3)], [net(3, 3)], n_step=0)


# ---------------------------------------------------------------------- 4. the new kernels' static resources
def test_population_learner_kernels_have_no_scratch_and_no_spills():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    csrc = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "resource-usage", "FLAGS_EXTRA=-DEVG_GRAD -DEVG_LEARN -DEVG_POP_LEARN"], capture_output=True,
                         text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    names = [n for n in usage if "evg_poplearn_" in n]
    # expand ids, take rows, the TD head for OUT 5 and 11, its loss reduction, the two backwards, their reduction, Adam
    assert len(names) == 9, names
    assert len([n for n in usage if "evg_learn_" in n]) == 4                       # (the plain learner's four are still there, as they were)
    for n in names:
        u = usage[n]
        print(n, u)
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
        if "qnet_grad" in n:
            assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 512, (n, u)
