"""CPU tests (no GPU needed) of prioritized sampling over the replay memory: the host model (tests/replay_priority_model.py) against the reference's own
agents/DQN/PrioritizedMemory.py where the reference tree is present, the model's properties, the agreement of header / export list / binding, and the
static resources of the new kernels."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rng_spec
from replay_priority_model import PriorityModel, S_BAD_HANDLE, S_BAD_PRIORITY, philox_words01, quantise, stamp, weight

CSRC = os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc")
REF = os.environ.get("EVG_REFERENCE", "/root/reference")
ENTRY_POINTS = {"evg_replay_priority_clear": 4, "evg_replay_update_priorities": 7, "evg_replay_sample_prioritized": 14}


class Base(object):
    """What PriorityModel needs of a ReplayModel: M records on one slot, record i holding counts[i] transitions (rows 0 .. c - 1, swarm = row)."""

    def __init__(self, counts, slots=1):
        counts = np.asarray(counts, np.int64).reshape(slots, -1)
        self.slots, self.N, self.S = slots, counts.shape[1], 1
        self.dirs = np.zeros((slots, self.N, 1, 7, 2), np.int32)
        self.dirs[..., 0] = -1
        for r in range(7):
            on = (counts > r)[:, :, None]
            self.dirs[..., r, 0] = np.where(on, r, -1)
            self.dirs[..., r, 1] = np.where(on, 1 + r % 4, 0)
        self.count = counts.astype(np.uint8)[:, :, None]
        self.meta = np.zeros((slots, self.N, 1, 4), np.int32)
        self.meta[..., 0] = np.arange(self.N)[None, :, None] % 150
        self.meta[..., 1] = np.arange(self.N)[None, :, None] // 150


def all_handles(model):
    k, e, s, r, _ = model.transitions()
    return np.stack([k, e, s, r], 1).astype(np.int32)


def log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)


# ---------------------------------------------------------------------- 1. against the live reference class
@pytest.fixture(scope="module")
def reference_class():
    path = os.path.join(REF, "agents", "DQN", "PrioritizedMemory.py")
    if not os.path.exists(path):
        pytest.skip("needs the reference tree (EVG_REFERENCE)")
    spec = importlib.util.spec_from_file_location("reference_prioritized_memory", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PrioritizedMemory


@pytest.mark.parametrize("M", [37, 400, 3000])
@pytest.mark.parametrize("alpha,beta", [(0.6, 0.4), (1.0, 1.0), (0.0, 0.4), (0.3, 0.7)])
def test_model_probabilities_and_weights_match_the_reference_class(reference_class, monkeypatch, M, alpha, beta):
    rng = np.random.default_rng(M * 7 + int(alpha * 10))
    state = np.zeros(3, np.float32)

    def run(prios):
        ref = reference_class(M, prob_alpha=alpha)
        for i in range(M):
            ref.push(state, 0, 0.0, state, False)
        ref.update_priorities(range(M), prios)
        seen = {}
        real_choice = np.random.choice

        def choice(a, size=None, replace=True, p=None):
            seen["p"] = np.array(p, np.float64)
            return real_choice(a, size, replace, p)

        monkeypatch.setattr(np.random, "choice", choice)
        out = ref.sample(256, beta=beta)
        monkeypatch.undo()
        model = PriorityModel(Base(np.ones(M)), alpha)
        model.update(all_handles(model), prios)
        assert model.status == 0
        return seen["p"], out[5], out[6], model

    # the p= handed to np.random.choice against q / Q: 1e-5 p for the reference's float32 `prios ** alpha` and normalisation, 2^-31 for one unit of
    # the quantisation over Q >= 2^31
    p, idx, w_ref, model = run(log_uniform(rng, M, 1e-5, 50.0))
    got = model.probabilities()
    err = np.abs(got - p) - (1e-5 * p + 2.0 ** -31)
    assert (err <= 0).all(), (float(np.abs(got - p).max()), float((np.abs(got - p) / p).max()))
    # importance weights, for priorities within a range of 2^10 (a q of at least 2^21 units: the quantisation is below 1e-6 relative)
    p, idx, w_ref, model = run(log_uniform(rng, M, 50.0 / 1024, 50.0))
    w = model.weights(np.asarray(idx), beta)
    assert np.allclose(w, w_ref.astype(np.float64), rtol=1e-5, atol=0), float(np.abs(w / w_ref - 1).max())


# ---------------------------------------------------------------------- 2. properties of the model
def test_vector_philox_equals_the_rng_statement():
    w0, w1 = philox_words01(50, (3 << 32) | 9, 0x1234567890ABCDEF)
    key = rng_spec._key(0x1234567890ABCDEF)
    for i in (0, 1, 17, 49):
        want = rng_spec.philox4x32_10((i, 9, 3, 7), key)
        assert (int(w0[i]), int(w1[i])) == want[:2]


def test_stamp_and_weight_conventions():
    assert int(stamp(0, 0)) == 0x80000000 and int(stamp(149, 3)) == 0x80000000 | (3 << 8) | 149
    assert int(stamp(256 + 5, (1 << 23) + 2)) == 0x80000000 | (2 << 8) | 5
    p = np.array([1e-30, 0.3, 1.0, 7.5, 3e38], np.float32)
    assert np.array_equal(weight(p, 1.0), p) and np.array_equal(weight(p, 0.0), np.ones(5, np.float32))
    assert float(weight(np.float32(1e-45), 1.0)) == float(np.float32(1.17549435e-38))         # a subnormal result is raised to FLT_MIN
    w = weight(p, 0.6).astype(np.float64)
    assert np.allclose(w, p.astype(np.float64) ** float(np.float32(0.6)), rtol=2.0 ** -23, atol=0)      # alpha is a float32 of the descriptor


def test_alpha_zero_gives_every_transition_two_to_the_31():
    model = PriorityModel(Base([3, 0, 7, 1, 2]), 0.0)
    h = all_handles(model)
    model.update(h[::2], log_uniform(np.random.default_rng(0), len(h[::2]), 1e-5, 50.0))
    q = model.q()
    assert len(q) == 13 and (q == 2 ** 31).all() and float(model.wmax) == 1.0


def test_a_weight_below_the_quantum_gets_one_unit():
    model = PriorityModel(Base(np.ones(6)), 1.0)
    h = all_handles(model)
    model.update(h[:4], np.array([1024.0, 1024.0 * 2.0 ** -32, 1024.0 * 2.0 ** -33, 1e-30], np.float32))
    q = model.q()
    # frexp(1024) = (0.5, 11): the heaviest holds 2^31 units, 2^-32 of it half a unit -> floored to 0 -> raised to 1; the never-updated two weigh wmax
    assert [int(x) for x in q] == [2 ** 31, 1, 1, 1, 2 ** 31, 2 ** 31]
    assert int(quantise(np.float32(1024.0 * 2.0 ** -31), np.float32(1024.0))) == 1
    assert int(quantise(np.float32(1024.0 * 2.0 ** -30), np.float32(1024.0))) == 2
    # wmax just below a power of two: the heaviest holds almost 2^32 units and stays below it
    m = np.nextafter(np.float32(2.0), np.float32(0.0))
    assert 2 ** 32 - 512 <= int(quantise(m, m)) < 2 ** 32


def test_duplicate_handles_keep_the_largest_priority_in_any_order():
    base = Base([2, 3])
    pr = np.array([0.5, 9.0, 2.0, 0.1, 4.0], np.float32)
    h = np.array([[0, 1, 0, 1]] * 5, np.int32)
    planes = []
    for order in (np.arange(5), np.arange(5)[::-1], np.array([1, 0, 4, 2, 3])):
        model = PriorityModel(base, 0.6)
        model.update(h[order], pr[order])
        planes.append(model.plane.copy())
        assert model.plane[0, 1, 0, 1] == weight(np.float32(9.0), 0.6) and float(model.wmax) == float(weight(np.float32(9.0), 0.6))
    assert np.array_equal(planes[0], planes[1]) and np.array_equal(planes[0], planes[2])
    # a later update with a SMALLER priority replaces the entry (the reset launch comes first); wmax stays
    model.update(h[:1], pr[3:4])
    assert model.plane[0, 1, 0, 1] == weight(np.float32(0.1), 0.6) and float(model.wmax) == float(weight(np.float32(9.0), 0.6))


def test_a_stale_stamp_reverts_the_whole_record_to_wmax():
    base = Base([3, 2])
    model = PriorityModel(base, 1.0)
    h = all_handles(model)
    model.update(h, np.array([0.25, 0.5, 4.0, 0.125, 2.0], np.float32))
    assert [float(x) for x in model.effective()] == [0.25, 0.5, 4.0, 0.125, 2.0]
    base.meta[0, 0, 0, 0] += 1                                     # the slot now holds another record: same rows, a later turn
    assert [float(x) for x in model.effective()] == [4.0, 4.0, 4.0, 0.125, 2.0]
    # the first update of the new occupant resets the other entries of the row and takes the new stamp
    model.update(h[1:2], np.array([0.75], np.float32))
    assert [float(x) for x in model.plane[0, 0, 0, :7]] == [0.0, 0.75, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert int(model.plane.view(np.uint32)[0, 0, 0, 7]) == int(stamp(1, 0))
    assert [float(x) for x in model.effective()] == [4.0, 0.75, 4.0, 0.125, 2.0]


def test_wmax_applies_as_of_the_draw_not_of_the_update():
    model = PriorityModel(Base(np.ones(3)), 1.0)
    h = all_handles(model)
    model.update(h[:1], np.array([2.0], np.float32))
    assert [float(x) for x in model.effective()] == [2.0, 2.0, 2.0]
    model.update(h[1:2], np.array([8.0], np.float32))                # the never-updated third follows the new maximum
    assert [float(x) for x in model.effective()] == [2.0, 8.0, 8.0]
    assert [int(x) for x in model.q()] == [2 ** 29, 2 ** 31, 2 ** 31]


def test_bad_priorities_and_handles_leave_the_plane_untouched():
    model = PriorityModel(Base([2, 0, 1]), 0.6)
    h = all_handles(model)
    model.update(h, np.array([0.5, 1.5, 2.5], np.float32))
    before, wmax = model.plane.copy(), model.wmax
    model.update(np.repeat(h[:1], 4, 0), np.array([np.nan, 0.0, -1.0, np.inf], np.float32))
    assert np.array_equal(model.plane, before) and model.wmax == wmax and model.status == S_BAD_PRIORITY
    model.status = 0
    bad = np.array([[0, 1, 0, 0], [0, 0, 0, 2], [1, 0, 0, 0], [0, 3, 0, 0], [0, 0, 1, 0], [0, 0, 0, 7], [-1, -1, -1, -1]], np.int32)
    model.update(bad, np.full(len(bad), 99.0, np.float32))
    assert np.array_equal(model.plane, before) and model.wmax == wmax and model.status == S_BAD_HANDLE


def test_model_draws_follow_q_over_Q():
    """65 536 draws; priorities log-uniform over [0.01, 10] at alpha 0.6 keep the weights within a factor of 63, so the rarest of at most 400
    transitions still expects about 8 draws and the normal bound is meaningful (a binomial count, sigma^2 = n p (1 - p))."""
    rng = np.random.default_rng(5)
    model = PriorityModel(Base(rng.integers(0, 8, 60)), 0.6)
    h = all_handles(model)
    assert 20 <= len(h) <= 400
    pick = rng.random(len(h)) < 0.7
    model.update(h[pick], log_uniform(rng, int(pick.sum()), 0.01, 10.0))
    p = model.probabilities()
    n = 65536
    handles, idx = model.draw(seed=77, call=3, batch=n)
    assert np.array_equal(handles, h[idx])
    counts = np.bincount(idx, minlength=len(h))
    sigma = np.sqrt(n * p * (1 - p))
    assert (np.abs(counts - n * p) < 5 * sigma).all(), float((np.abs(counts - n * p) / sigma).max())
    # another call index draws others; the same one repeats
    assert not np.array_equal(model.draw(77, 4, 512)[1], idx[:512]) and np.array_equal(model.draw(77, 3, 512)[1], idx[:512])


# ---------------------------------------------------------------------- 3. header, export list and binding agree
def _prototype_arity(header, name):
    m = re.search(r"EVG_API int %s\(([^;]*)\)\s*;" % name, header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_prototypes_ctypes_argtypes_and_exports_agree():
    """The three entry points live in include/evg_replay_priority.h and libevg_priority.so (the product's sources with -DEVG_PRIORITY); libevg.so and
    include/evg.h keep exactly the entry points they had."""
    import everglades_amd
    _lib = everglades_amd._lib
    header = open(os.path.join(ROOT, "include", "evg_replay_priority.h")).read()
    main_header = open(os.path.join(ROOT, "include", "evg.h")).read()
    assert _lib.PRIORITY_EXPORTS == list(ENTRY_POINTS) and not set(ENTRY_POINTS) & set(_lib.EXPORTS)
    assert set(re.findall(r"EVG_API \w+ (evg_[a-z_]+)\s*\(", header)) == set(ENTRY_POINTS)
    assert not any(name + "(" in main_header for name in ENTRY_POINTS)
    lib = _lib.load_priority()
    assert _lib.ABI_VERSION == 7 and "#define EVG_ABI_VERSION 7" in main_header and lib.evg_abi_version() == 7
    for name, arity in ENTRY_POINTS.items():
        assert _prototype_arity(header, name) == len(getattr(lib, name).argtypes) == arity, name
    assert _prototype_arity(header, "evg_replay_sample_prioritized") == _prototype_arity(main_header, "evg_replay_sample") + 3
    assert "global: evg_*;" in open(os.path.join(CSRC, "evg.map")).read()

    def exported(path):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        return {line.split()[-1] for line in out.splitlines() if line.strip()}

    assert exported(_lib.PRIORITY_LIB_PATH) == set(_lib.EXPORTS) | set(ENTRY_POINTS)
    assert exported(_lib.LIB_PATH) == set(_lib.EXPORTS)
    assert "enum { EVG_REPLAY_S_BAD_PRIORITY = 4 };" in header and _lib.REPLAY_S_BAD_PRIORITY == 4 == S_BAD_PRIORITY
    assert (_lib.REPLAY_S_EMPTY, _lib.REPLAY_S_BAD_HANDLE) == (1, 2) and S_BAD_HANDLE == 2
    assert hasattr(everglades_amd, "PrioritizedSmartReplay") and hasattr(everglades_amd.EvergladesVecEnv, "prioritized_replay")
    assert issubclass(everglades_amd.PrioritizedSmartReplay, everglades_amd.SmartReplay)
    assert "RP_PDRAW_DOMAIN = 7" in open(os.path.join(CSRC, "replay_priority_kernels.inc")).read()


def test_descriptor_layout_matches_the_compiler(tmp_path):
    from everglades_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evg_replay_priority.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %lld %lld\\n", '
                   'sizeof(evg_replay_priority), offsetof(evg_replay_priority, alpha), offsetof(evg_replay_priority, plane), '
                   'offsetof(evg_replay_priority, pscan), offsetof(evg_replay_priority, pctl), (long long)EVG_REPLAY_PSCAN_WORDS(5, 1031, 2), '
                   '(long long)EVG_REPLAY_PSCAN_WORDS(9, 65536, 1)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    d = _lib.EvgReplayPriority
    R1, R2 = 5 * 1031 * 2, 9 * 65536
    assert got == [C.sizeof(d), d.alpha.offset, d.plane.offset, d.pscan.offset, d.pctl.offset, (R1 + 3) // 4 + 2 * ((R1 + 1023) // 1024),
                   (R2 + 3) // 4 + 2 * ((R2 + 1023) // 1024)]
    assert [f[0] for f in d._fields_] == ["alpha", "plane", "pscan", "pctl"] and C.sizeof(d) == 32


# ---------------------------------------------------------------------- 4. the new kernels' static resources
def test_priority_kernels_have_no_scratch_and_no_spills():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage", "FLAGS_EXTRA=-DEVG_PRIORITY"], capture_output=True, text=True, check=True)
    usage = {}
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        usage[block.split()[0]] = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
    names = [n for n in usage if re.search(r"evg_prio_(clear|update|scan|top|draw|weights)_kernel", n)]
    assert len(names) == 6, names
    for n in names:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == "0" and u["VGPRs Spill"] == "0" and u["SGPRs Spill"] == "0", (n, u)
