"""GPU tests of evg_smart_qnet_bf16 / evg_minimized_qnet_bf16 (env.smart_qnet / env.minimized_qnet with precision="bf16"; include/evg_qnet_bf16.h)
against the host model of the numeric contract (tests/qnet_bf16_model.py), in the three layouts, with different weights per seat in the two-seat one:

  exact tier    the families of tests/qnet_bf16_cases.py (integer, permutation, rounding, nonfinite): bit-equal values, equal NaN masks
  random tier   the families signed, absorbed and zero_column of tests/learner_edge_cases.py: |Q^ - Q| <= E elementwise, E the model's derived bound
  shapes        Smart (60, 60), (17, 64), (1, 1), (64, 64), Minimized 80, 128, 17, 1; 1, 15, 16, 17 and 37 rows; one full sweep of the capped grid
                plus a group and a row; both final_relu values
  boundaries    a captured call replays to the same values; refusals; the fp32 evaluators are what they were with the new library loaded"""
import ctypes as C

import numpy as np
import pytest

import learner_edge_cases as edge
import qnet_bf16_cases as cases
import qnet_bf16_model as model
import qnet_model
import minimized_model

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


@pytest.fixture(scope="module")
def env(evg):
    e = evg.EvergladesVecEnv(64, seed=5)
    yield e
    e.close()


def _dev(env, a):
    import torch
    if isinstance(a, tuple):
        return tuple(_dev(env, x) for x in a)
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _evaluator(env, kind, params, final_relu, precision="bf16"):
    """the device network of one case; params are one set, or the two sets of the two-seat layout"""
    make = env.smart_qnet if kind == "smart" else env.minimized_qnet
    return make(_dev(env, params), final_relu=final_relu, precision=precision)


def _run(net, layout, dev_inputs, out=None):
    if layout == "expanded":
        return net.expanded(dev_inputs, out=out)
    return net(dev_inputs[0], dev_inputs[1], out=out)


def _relu(q):
    return np.where(q < 0, np.float32(0), q)             # a NaN stays


def test_precision_argument_selects_the_class(evg, env):
    p = cases.net_params("smart", (60, 60), "integer")
    assert type(env.smart_qnet(_dev(env, p), final_relu=False)) is evg.SmartQNet
    assert type(env.smart_qnet(_dev(env, p), final_relu=False, precision="fp32")) is evg.SmartQNet
    assert type(env.smart_qnet(_dev(env, p), final_relu=False, precision="bf16")) is evg.SmartQNetBf16
    m = cases.net_params("mini", (80,), "integer")
    assert type(env.minimized_qnet(_dev(env, m), final_relu=False)) is evg.MinimizedQNet
    assert type(env.minimized_qnet(_dev(env, m), final_relu=False, precision="bf16")) is evg.MinimizedQNetBf16
    with pytest.raises(ValueError):
        env.smart_qnet(_dev(env, p), final_relu=False, precision="int8")


# ---------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("kind,hidden,family", cases.EXACT_CASES, ids=cases.EXACT_IDS)
def test_exact_tier_is_bit_equal_to_the_host_model(env, kind, hidden, family, layout):
    params, inputs = cases.case(kind, hidden, family, layout)
    raw, _ = model.forward_layout(layout, params, inputs, False, exact=True, rounds=family == "rounding")
    for final_relu in (False, True):
        want = _relu(raw) if final_relu else raw
        net = _evaluator(env, kind, params, final_relu)
        for rows in cases.ROWS:
            got = _run(net, layout, _dev(env, cases.first_rows(layout, inputs, rows))).cpu().numpy()
            w = want[:rows]
            differ = int((~((got == w) | (np.isnan(got) & np.isnan(w)))).sum())
            print("%s %s %s %s final_relu=%d rows=%d: %d values, NaN %d (model %d), Inf %d, differ at %d" % (
                kind, hidden, family, layout, final_relu, rows, got.size, np.isnan(got).sum(), np.isnan(w).sum(), np.isinf(got).sum(), differ))
            assert cases.same_values(got, w), (kind, hidden, family, layout, final_relu, rows)


# ---------------------------------------------------------------------- random tier
WORST = {}


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("family", cases.RANDOM_FAMILIES)
@pytest.mark.parametrize("kind,hidden", cases.NETS, ids=cases.NET_IDS)
def test_random_tier_stays_within_the_derived_bound(env, kind, hidden, family, layout):
    params, inputs = edge.case(kind, hidden, family, layout)
    raw, bound = model.forward_layout(layout, params, inputs, False)
    full = raw.shape[0]
    worst = 0.0
    for final_relu in (False, True):
        want = _relu(raw) if final_relu else raw
        net = _evaluator(env, kind, params, final_relu)
        for rows in cases.ROWS + [full]:
            got = _run(net, layout, _dev(env, cases.first_rows(layout, inputs, rows))).cpu().numpy()
            ok, ratio = cases.within_bound(got, want[:rows], bound[:rows])
            worst = max(worst, ratio)
            assert ok, (kind, hidden, family, layout, final_relu, rows, ratio)
            if family == "absorbed":
                assert np.isfinite(got).all()                  # a padded unit's NaN accumulator reaches no output
            if family == "zero_column" and rows == full:
                assert np.isnan(got).any() and np.isfinite(got).mean() > 0.5
    WORST[(kind, hidden, family, layout)] = worst
    print("%s %s %s %s: worst |Q^ - Q| / E = %.4f (so far, all cases: %.4f)" % (kind, hidden, family, layout, worst, max(WORST.values())))


# ---------------------------------------------------------------------- the second sweep of the capped grid
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("family", ["integer", "permutation"])
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_second_sweep_of_the_capped_grid(env, kind, hidden, family, layout):
    """rows = one full sweep of the launch's grid (2 workgroups per CU x 4 wavefronts x 16 rows) + one group + one row: the grid-stride loop takes its
    back edge in the first wavefronts, and the last group holds one row.  A row the kernel skips keeps the -7 the output was filled with."""
    import torch
    cus = torch.cuda.get_device_properties(env.device).multi_processor_count
    rows = cases.sweep_rows(cus)
    params, inputs = cases.case(kind, hidden, family, layout, rows)
    pick = cases.sweep_checked_rows(rows, cus)
    want, _ = model.forward_layout(layout, params, cases.pick_rows(layout, inputs, pick), True)
    net = _evaluator(env, kind, params, True)
    lead = {"expanded": (rows,), "compact": (rows, 12), "seats": (rows, 2, 12)}[layout]
    out = torch.full(lead + (cases.OUT[kind],), -7.0, dtype=torch.float32, device=env.device)
    got = _run(net, layout, _dev(env, inputs), out=out).cpu().numpy()
    assert (got >= 0).all()                                    # final ReLU on: every row was written
    assert cases.same_values(got[pick], want)


# ---------------------------------------------------------------------- boundaries
@pytest.mark.parametrize("kind,hidden", [("smart", (60, 60)), ("mini", (80,))], ids=["smart", "mini"])
def test_captured_call_replays_to_the_same_values(env, kind, hidden):
    import torch
    params, inputs = edge.case(kind, hidden, "signed", "seats")
    net = _evaluator(env, kind, params, False)
    shared, swarm = _dev(env, inputs)
    out = torch.empty(shared.shape[:2] + (12, cases.OUT[kind]), dtype=torch.float32, device=env.device)
    s = torch.cuda.Stream(env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(s):
        net(shared, swarm, out=out)                            # warm-up outside the capture
    torch.cuda.current_stream(env.device).wait_stream(s)
    eager = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net(shared, swarm, out=out)
    out.fill_(-7.0)
    g.replay()
    assert torch.equal(out, eager)
    shared.mul_(2.0)                                           # the replay reads the tensors as they are now
    g.replay()
    want = net(shared, swarm)
    assert torch.equal(out, want) and not torch.equal(out, eager)


def test_refusals_are_those_of_the_fp32_entry_points(evg, env):
    """A misaligned pointer, h1 = 65 (Smart) and h1 = 129 (Minimized): EVG_ERR_INVALID from both precisions' entry points, nothing launched."""
    import torch
    _lib = evg._lib
    B = _lib.load_bf16()
    N = 37
    for kind, hidden, entry, fp32_entry, too_wide in (("smart", (60, 60), B.evg_smart_qnet_bf16, B.evg_smart_qnet, 65),
                                                     ("mini", (80,), B.evg_minimized_qnet_bf16, B.evg_minimized_qnet, 129)):
        params, inputs = edge.case(kind, hidden, "signed", "compact")
        net = _evaluator(env, kind, params, False)
        shared, swarm = _dev(env, cases.first_rows("compact", inputs, N))
        out = torch.full((N, 12, cases.OUT[kind]), 7.0, dtype=torch.float32, device=env.device)

        def call(fn, d, in0=None, q=None):
            return fn(env._h, C.byref(d), _lib.QNET_COMPACT, N, C.c_void_p(shared.data_ptr() if in0 is None else in0), C.c_void_p(swarm.data_ptr()),
                      C.c_void_p(out.data_ptr() if q is None else q), None)

        for fn in (entry, fp32_entry):
            d = net._descriptor(1)
            assert call(fn, d, in0=shared.data_ptr() + 4) == -1 and call(fn, d, q=out.data_ptr() + 8) == -1         # EVG_ERR_INVALID
            d.b1[0] = d.b1[0] + 4
            assert call(fn, d) == -1
            d = net._descriptor(1)
            d.h1 = too_wide
            assert call(fn, d) == -1
            d.h1 = 0
            assert call(fn, d) == -1
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                        # nothing was launched
        assert "hidden size" in B.evg_last_error().decode()
        assert call(entry, net._descriptor(1)) == 0
        torch.cuda.synchronize()
        assert bool((out != 7.0).any())
    with pytest.raises(ValueError):                            # the Python surface's own checks are shared: they refuse first
        env.smart_qnet(_dev(env, edge.net_params("smart", (65, 60), "signed")), final_relu=False, precision="bf16")
    with pytest.raises(ValueError):
        env.minimized_qnet(_dev(env, edge.net_params("mini", (129,), "signed")), final_relu=False, precision="bf16")


def test_fp32_evaluators_are_unchanged_with_the_bf16_library_loaded(evg, env):
    """The fp32 evaluators give the host model's fmaf chain bit for bit before and after libevg_bf16.so is loaded and used."""
    outs = {}
    for stage in ("before", "after"):
        for kind, hidden, host in (("smart", (60, 60), qnet_model), ("mini", (80,), minimized_model)):
            params, inputs = edge.case(kind, hidden, "signed", "compact")
            got = _run(_evaluator(env, kind, params, True, precision="fp32"), "compact", _dev(env, inputs)).cpu().numpy()
            outs[(stage, kind)] = got
            assert edge.same_values(got, host.forward_compact(inputs[0], inputs[1], params, True))
        evg._lib.load_bf16()
        params, inputs = edge.case("smart", (60, 60), "signed", "compact")
        _run(_evaluator(env, "smart", params, True), "compact", _dev(env, inputs))
    for kind in ("smart", "mini"):
        assert np.array_equal(outs[("before", kind)].view(np.uint32), outs[("after", kind)].view(np.uint32))
