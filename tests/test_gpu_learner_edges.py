"""GPU tests of the learner-side kernels at their numeric and shape edges (the cases of tests/learner_edge_cases.py, shown on the CPU by
tests/test_learner_edge_cases.py to reach what they name), each against its host model on the same arrays:

  B  evg_smart_qnet / evg_minimized_qnet in the three layouts, with and without the final ReLU, at every hidden size of the case module: signed inputs,
     subnormal hidden units and Q, overflow inside the chain (NaN, +-Inf and finite Q), non-finite inputs (whose rows alone may be damaged: the padded
     hidden units must not leak them), non-finite and zero weights (seat 0 of the two-seat layout stays finite), a -Inf input that the ReLU
     absorbs in every real unit (Q finite, while a padded unit's accumulator is NaN) -- compared by value with equal NaN masks,
     the contract of include/evg.h: torch's ReLU keeps a NaN;
     the Minimized kernel's second sweep of its capped grid: one full sweep, one group and one row, against the model and against fresh 4 096-row calls;
  C  evg_replay_*: a synthetic driver (random features, directions, rewards, done, custom rewards; no stepping) over the shaping x ring x seat grid, frozen
     envs with n = 4, and a ring past 256 scan blocks with runs of empty blocks -- metadata record for record, size(), a gather of every transition, and
     sample() handle for handle against ReplayModel.draw."""
import numpy as np
import pytest

import learner_edge_cases as cases
from test_gpu_replay import check_gather, model_handles

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]     # (numpy's warnings of the overflow the cases are about)

NETS = [("smart", h) for h in cases.SMART_HIDDEN] + [("mini", h) for h in cases.MINI_HIDDEN]


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


def _evaluator(env, kind, layout, params, final_relu):
    """the device network of one case; params are one set, or the two sets of the two-seat layout"""
    make = env.smart_qnet if kind == "smart" else env.minimized_qnet
    return make(_dev(env, params), final_relu=final_relu)


def _run(net, layout, dev_inputs, out=None):
    if layout == "expanded":
        return net.expanded(dev_inputs, out=out)
    return net(dev_inputs[0], dev_inputs[1], out=out)


def _report(tag, got, want):
    """the figures of a comparison, printed before it is asserted"""
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    both = ~nan_g & ~nan_w
    print("%s: %d values, NaN %d (model %d), Inf %d (model %d), subnormal %d (model %d), NaN masks differ at %d, values differ at %d" % (
        tag, got.size, nan_g.sum(), nan_w.sum(), np.isinf(got).sum(), np.isinf(want).sum(), cases.is_subnormal(got).sum(),
        cases.is_subnormal(want).sum(), (nan_g != nan_w).sum(), (got[both] != want[both]).sum()))


_MODEL_Q = {}


def _model_q(kind, hidden, family, layout):
    """the host model's Q without the final ReLU, computed once per case (with it: the model's own np.maximum on top, as qnet_model.layer applies it)"""
    key = (kind, hidden, family, layout)
    if key not in _MODEL_Q:
        params, inputs = cases.case(kind, hidden, family, layout)
        _MODEL_Q[key] = cases.model_q(kind, layout, params, inputs, False)
        _MODEL_Q[key].setflags(write=False)
    return _MODEL_Q[key]


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("kind,hidden", NETS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_q_networks_equal_the_host_model_at_the_numeric_edges(env, kind, hidden, family, layout):
    params, inputs = cases.case(kind, hidden, family, layout)
    dev_inputs = _dev(env, inputs)
    raw = _model_q(kind, hidden, family, layout)
    for final_relu in (False, True):
        want = np.maximum(raw, np.float32(0)) if final_relu else raw
        got = _run(_evaluator(env, kind, layout, params, final_relu), layout, dev_inputs).cpu().numpy()
        _report("%s %s %s %s final_relu=%d" % (kind, hidden, family, layout, final_relu), got, want)
        assert cases.same_values(got, want), (kind, hidden, family, layout, final_relu)
        # what a damaged row or weight set must not reach, said of the device output itself
        if family == "absorbed":
            assert np.isfinite(got).all()                                                  # a padded unit's NaN accumulator reaches no output
        if family in ("nonfinite", "zero_column"):
            if layout == "seats":
                shared, swarm = inputs
                clean = np.isfinite(shared).all(2) & np.isfinite(swarm).all((2, 3))        # [N, 2]
            else:
                clean = ~cases.damaged_rows(family, got.shape[0])
            assert clean.sum() * 7 >= clean.size * 4 and np.isfinite(got[clean]).all()
            assert not np.isfinite(got[~clean]).all()
        if layout == "seats" and family in cases.WEIGHT_DAMAGE:
            assert np.isfinite(got[:, 0]).all()
        if family == "overflow" and min(hidden) >= 16:
            assert np.isnan(got).mean() >= 0.10                                            # also with the final ReLU on: it keeps a NaN


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("family", ["signed", "nonfinite"])
@pytest.mark.parametrize("h1", [80, 128])
def test_minimized_second_sweep_equals_the_model_and_fresh_calls(env, h1, family, layout):
    """rows = one full sweep of the capped grid (2 workgroups per CU x 4 wavefronts x 16 rows) + one group + one row: the grid-stride loop takes its back
    edge, the per-wavefront LDS tile is reused behind the wavefront barrier, and the last group holds one row."""
    import torch
    cus = torch.cuda.get_device_properties(env.device).multi_processor_count
    rows = cases.sweep_rows(cus)
    final_relu = family == "nonfinite"
    seats = 2 if layout == "seats" else 1
    if layout == "expanded":
        params, inputs = cases.net_params("mini", (h1,), family), cases.expanded_inputs(family, rows)
        pick_inputs = lambda idx: inputs[idx]                                               # noqa: E731
        shape = (rows, 11)
    else:
        params = cases.seat_params("mini", (h1,), family) if seats == 2 else cases.net_params("mini", (h1,), family)
        inputs = cases.compact_inputs(family, rows, seats)
        pick_inputs = lambda idx: (inputs[0][idx], inputs[1][idx])                          # noqa: E731
        shape = (rows, 2, 12, 11) if seats == 2 else (rows, 12, 11)
    net = _evaluator(env, "mini", layout, params, final_relu)
    dev_inputs = _dev(env, inputs)
    out = torch.full(shape, -7.0, dtype=torch.float32, device=env.device)                  # a row the kernel skips keeps its -7
    got = _run(net, layout, dev_inputs, out=out).cpu().numpy()
    pick = cases.sweep_checked_rows(rows, cus)
    want = cases.model_q("mini", layout, params, pick_inputs(pick), False)
    if final_relu:
        want = np.maximum(want, np.float32(0))
    _report("sweep %d rows (%d CUs) h1=%d %s %s" % (rows, cus, h1, family, layout), got[pick], want)
    assert cases.same_values(got[pick], want)
    # batch invariance: the same rows as fresh 4 096-row calls (every row of them inside a first sweep) give the same values
    for lo in range(0, rows, 4096):
        idx = np.arange(lo, min(lo + 4096, rows))
        part = _run(net, layout, _dev(env, pick_inputs(idx))).cpu().numpy()
        assert cases.same_values(part, got[idx]), (lo, int((~np.isclose(part, got[idx], rtol=0, atol=0, equal_nan=True)).sum()))
    if family == "nonfinite":
        clean = ~cases.damaged_rows(family, rows)
        if seats == 2:
            clean = np.isfinite(inputs[0]).all(2) & np.isfinite(inputs[1]).all((2, 3))
        assert np.isfinite(got[clean]).all() and not np.isfinite(got[~clean]).all()


# ------------------------------------------------------------------------------------------------------------------ replay memory
def _compare_metadata(mem, model, t):
    assert np.array_equal(mem.meta.cpu().numpy(), model.meta), "meta at turn %d" % t
    assert np.array_equal(mem.counts.cpu().numpy(), model.count), "counts at turn %d" % t
    assert np.array_equal(mem.rewards.cpu().numpy().view(np.uint64), model.rew.view(np.uint64)), "rewards (float64 bits) at turn %d" % t
    assert np.array_equal(mem.env_state.cpu().numpy(), model.ctr), "env counters at turn %d" % t


def _drive(evg, case):
    """the synthetic loop of a case on the device and in the host model, compared as the docstring of this file says"""
    import torch
    env = evg.EvergladesVecEnv(case.N, seed=7, auto_reset=case.auto_reset)
    env.reset()
    dev = env.device
    mem = env.smart_replay(case.H, n_step=case.n, gamma=case.gamma, shaping=case.shaping, seats=case.seats, episode_base=0)
    model = case.model()
    put = lambda views, arrays: [v.copy_(torch.from_numpy(a).to(dev)) for v, a in zip(views, arrays)]     # noqa: E731
    put(mem.slot_features(0), case.features(0))
    checked = 0
    for t in range(case.turns):
        put(mem.slot_features(t + 1), case.features(t + 1))
        dirs, reward, done, custom = case.turn(t)
        mem.slot_directions(t).copy_(torch.from_numpy(dirs).to(dev))
        shaped = torch.from_numpy(custom).to(dev) if case.shaping == "custom" else None
        mem.record(torch.from_numpy(reward).to(dev), torch.from_numpy(done).to(dev), shaped=shaped)
        model.record(dirs, reward, done, custom if case.shaping == "custom" else None)
        if case.per_turn or t in case.checks:
            _compare_metadata(mem, model, t)
        if t in case.checks:
            total = model.size()
            print("%s turn %d: %d transitions in %d records" % (case.name, t, total, model.count.size))
            assert int(mem.size().item()) == total and total > 0
            h = model_handles(model, dev)
            assert h.shape[0] == total
            for lo in range(0, total, 65536):
                check_gather(mem, model, h[lo:lo + 65536].contiguous())
            for B in cases.SAMPLE_SIZES:
                call = int(mem.sample_calls.item())
                out = [x.clone() for x in mem.sample(B, seed=cases.SEED, return_handles=True)]
                want = model.draw(cases.SEED, call, B)
                got = out[5].cpu().numpy()
                assert np.array_equal(got, want), "draw %d of sample(%d) at turn %d" % (int(np.flatnonzero((got != want).any(1))[0]), B, t)
                for a, b in zip(out[:5], mem.gather(out[5])):
                    assert torch.equal(a, b)
            checked += 1
    assert checked == 3
    assert int(mem.size().item()) == model.size()
    mem.check()
    return env, mem, model


@pytest.mark.parametrize("case", cases.REPLAY_GRID, ids=repr)
def test_record_and_draw_over_the_configuration_grid(evg, case):
    env, mem, model = _drive(evg, case)
    env.close()


@pytest.mark.parametrize("case", cases.REPLAY_FROZEN, ids=repr)
def test_frozen_envs_record_nothing_more_with_a_long_n_step(evg, case):
    env, mem, model = _drive(evg, case)
    assert (model.ctr[:, 3] == 1).all() and bool((mem.env_state[:, 3] == 1).all())
    env.close()


def test_ring_past_256_scan_blocks_with_runs_of_empty_blocks(evg):
    env, mem, model = _drive(evg, cases.REPLAY_BIG)
    env.close()
