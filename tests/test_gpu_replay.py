"""GPU tests of the Smart_State replay memory on the device (everglades_amd.SmartReplay, include/evg.h evg_replay_*):
  - the reference's own memory (tests/golden/smart_replay.npz) rebuilt by the record kernel from the fixture's inputs, gather of every transition;
  - end to end with step_vs_q (both seats), step_q and auto_reset=False over 400 turns of a wrapping ring, against the host model (tests/replay_model.py)
    fed the same step outputs;
  - sample: valid handles, outputs equal to gather, uniform frequencies, repeatable draws;
  - refusals and the device status word."""
import numpy as np
import pytest

from conftest import load_golden
from replay_model import ReplayModel
from test_replay_model import variant_shaping

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def evg():
    import everglades_amd
    return everglades_amd


def expected_batch(mem, handles, model):
    """optimize_model's operands for handles int32 [B, 4], expanded with torch from the ring's own feature buffers and the model's metadata."""
    import torch
    h = handles.long()
    slot, env, seat, row = h[:, 0], h[:, 1], h[:, 2], h[:, 3]
    if mem.S == 2:
        sh, sw_all = mem.shared[slot, env, seat], mem.swarm[slot, env, seat]
        dirs = mem.directions[slot, env, seat]
    else:
        sh, sw_all = mem.shared[slot, env], mem.swarm[slot, env]
        dirs = mem.directions[slot, env]
    B = h.shape[0]
    ar = torch.arange(B, device=h.device)
    swarm = dirs[ar, row, 0].long()
    eye = torch.eye(12, device=h.device)
    obs = torch.cat([sh, sw_all[ar, swarm], eye[swarm]], 1)
    hn = handles.cpu().numpy()
    nd = (model.meta[hn[:, 0], hn[:, 1], hn[:, 2], 2] & 1) != 0
    nslot = (slot + mem.n_step) % mem.slots
    if mem.S == 2:
        nsh, nsw = mem.shared[nslot, env, seat], mem.swarm[nslot, env, seat]
    else:
        nsh, nsw = mem.shared[nslot, env], mem.swarm[nslot, env]
    nxt = torch.cat([nsh[:, None, :].expand(-1, 12, -1), nsw, eye.expand(B, -1, -1)], 2)
    ndt = torch.as_tensor(nd, device=h.device)
    nxt = torch.where(ndt[:, None, None], nxt, torch.zeros_like(nxt))
    action = (dirs[ar, row, 1] - 1).long()
    reward = torch.as_tensor(model.rew[hn[:, 0], hn[:, 1], hn[:, 2], 1].astype(np.float32), device=h.device)
    return obs, action, nxt, reward, ndt


def check_gather(mem, model, handles):
    import torch
    got = [t.clone() for t in mem.gather(handles)]
    want = expected_batch(mem, handles, model)
    names = ["swarm_obs", "action", "next_state", "reward", "not_done"]
    for g, w, name in zip(got, want, names):
        assert torch.equal(g, w.to(g.dtype)), name


def model_handles(model, device, limit=None, seed=0):
    import torch
    tr = model.transitions()
    h = np.stack([tr["slot"], tr["env"], tr["seat"], tr["row"]], 1).astype(np.int32)
    if limit is not None and len(h) > limit:
        h = h[np.random.default_rng(seed).choice(len(h), limit, replace=False)]
    return torch.as_tensor(h, device=device)


@pytest.mark.parametrize("v", ["a", "b", "c"])
def test_record_kernel_rebuilds_the_reference_memory(evg, v):
    import torch
    d = load_golden("smart_replay.npz")
    n, gamma, shaping, base = variant_shaping(d[v + "_params"])
    T = len(d[v + "_done"])
    env = evg.EvergladesVecEnv(1, seed=1)
    env.reset()
    mem = env.smart_replay(T + 1, n_step=n, gamma=gamma, shaping=shaping, seats=0, episode_base=base)
    dev = env.device
    model = ReplayModel(1, 1, T + 1, n, gamma, shaping, episode_base=base)
    rew = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    done = torch.zeros((1,), dtype=torch.uint8, device=dev)
    for t in range(T):
        for k in (t, t + 1):                                                   # record t's features (and t + 1's, as the step would write them)
            if k < T:
                mem.slot_features(k)[0].copy_(torch.as_tensor(d[v + "_shared"][k][None], device=dev))
                mem.slot_features(k)[1].copy_(torch.as_tensor(d[v + "_swarm"][k][None], device=dev))
        mem.slot_directions(t).copy_(torch.as_tensor(d[v + "_dirs"][t][None], device=dev))
        rew.copy_(torch.as_tensor(d[v + "_reward"][t][None].astype(np.float32), device=dev))
        done.fill_(int(d[v + "_done"][t]))
        mem.record(rew, done)
        model.record(d[v + "_dirs"][t][None], d[v + "_reward"][t][None].astype(np.float32), d[v + "_done"][t][None])
    assert np.array_equal(mem.meta.cpu().numpy(), model.meta) and np.array_equal(mem.counts.cpu().numpy(), model.count)
    assert np.array_equal(mem.rewards.cpu().numpy(), model.rew)
    assert int(mem.size().item()) == len(d[v + "_tr"])
    # gather every transition of the fixture: {record, swarm} -> handle {slot = record, 0, 0, row of that swarm}
    tr, trr = d[v + "_tr"], d[v + "_tr_reward"]
    rows = np.array([int(np.flatnonzero(d[v + "_dirs"][r][:, 0] == sw)[0]) for r, sw in tr[:, :2]], np.int32)
    handles = torch.as_tensor(np.stack([tr[:, 0], np.zeros_like(rows), np.zeros_like(rows), rows], 1).astype(np.int32), device=dev)
    obs, action, nxt, reward, nd = [t.cpu().numpy() for t in mem.gather(handles)]
    feats = np.concatenate([np.broadcast_to(d[v + "_shared"][:, None, :], (T, 12, 34)), d[v + "_swarm"], np.broadcast_to(np.eye(12, dtype=np.float32),
                                                                                                                       (T, 12, 12))], 2)
    assert np.array_equal(obs, feats[tr[:, 0], tr[:, 1]])
    assert np.array_equal(action, tr[:, 2].astype(np.int64))
    want_next = np.where((tr[:, 3] >= 0)[:, None, None], feats[np.maximum(tr[:, 3], 0)], 0.0).astype(np.float32)
    assert np.array_equal(nxt, want_next)
    assert np.array_equal(nd.astype(np.int32), tr[:, 4])
    assert np.allclose(reward.astype(np.float64), trr, rtol=1e-6, atol=1e-7)
    mem.check()
    env.close()


def run_loop(evg, N, form, seat=0, auto_reset=True, turns=400, H=8, n=2, shaping="reward_short_games", gather_at=(60, 250, 399), gather_limit=None):
    import torch
    env = evg.EvergladesVecEnv(N, seed=11 + N, auto_reset=auto_reset)
    obs = env.reset()
    dev = env.device
    S = 2 if form == "step_q" else 1
    mem = env.smart_replay(H, n_step=n, gamma=0.9, shaping=shaping, seats=(0, 1) if S == 2 else seat, episode_base=0)
    st = env.get_state()["env"]
    model = ReplayModel(N, S, H, n, 0.9, shaping, seat=seat, auto_reset=auto_reset, turn0=st[:, 0], episode0=st[:, 2])
    if S == 2:
        for p in range(2):
            s_, w_ = env.smart_state_compact(p, obs)
            mem.slot_features(0)[0][:, p].copy_(s_)
            mem.slot_features(0)[1][:, p].copy_(w_)
    else:
        env.smart_state_compact(-1, env.observe_seat(seat), *mem.slot_features(0))
    g = torch.Generator(device="cpu").manual_seed(N)
    checked = 0
    for t in range(turns):
        qshape = (N, 2, 12, 5) if S == 2 else (N, 12, 5)
        q = (torch.randn(qshape, generator=g) * 2.0).round().to(dev)
        if S == 2:
            env.step_q(q, (0.3, 0.1), features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        else:
            env.step_vs_q("swarm", q, 0.3, seat=seat, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        mem.record()
        model.record(mem.slot_directions(t).cpu().numpy(), env.reward.cpu().numpy(), env.done.cpu().numpy())
        assert np.array_equal(mem.meta.cpu().numpy(), model.meta), "meta at turn %d" % t
        assert np.array_equal(mem.counts.cpu().numpy(), model.count), "counts at turn %d" % t
        assert np.array_equal(mem.rewards.cpu().numpy(), model.rew), "rewards at turn %d" % t
        assert np.array_equal(mem.env_state.cpu().numpy(), model.ctr), "env counters at turn %d" % t
        if t in gather_at:
            assert int(mem.size().item()) == model.size()
            h = model_handles(model, dev, gather_limit, seed=t)
            for lo in range(0, h.shape[0], 65536):
                check_gather(mem, model, h[lo:lo + 65536].contiguous())
            checked += h.shape[0]
    mem.check()
    assert checked > 0
    return env, mem, model


@pytest.mark.parametrize("N,seat", [(4096, 0), (4096, 1), (65536, 0)])
def test_step_vs_q_loop_matches_the_host_model(evg, N, seat):
    env, mem, model = run_loop(evg, N, "step_vs_q", seat=seat, gather_limit=None if N <= 4096 else 200000)
    env.close()


@pytest.mark.parametrize("N", [4096, 65536])
def test_step_q_loop_matches_the_host_model(evg, N):
    env, mem, model = run_loop(evg, N, "step_q", shaping=("transition", "normalized_score", "reward_short_games", 3),
                               gather_limit=None if N <= 4096 else 200000)
    env.close()


def test_frozen_envs_record_nothing_after_their_last_turn(evg):
    env, mem, model = run_loop(evg, 4096, "step_vs_q", auto_reset=False, turns=200, shaping="penalize_long_games", gather_at=(150, 199))
    assert (model.ctr[:, 3] == 1).all()                                        # every game ended by turn 150 and froze
    env.close()


def test_sample_draws_valid_handles_and_equals_gather(evg):
    import torch
    env, mem, model = run_loop(evg, 4096, "step_vs_q", turns=30, gather_at=(29,))
    valid = set(map(tuple, model_handles(model, "cpu").numpy().tolist()))
    for B in (1, 3, 1024, 4099):
        out = [t.clone() for t in mem.sample(B, seed=5, return_handles=True)]
        hs = out[5]
        assert set(map(tuple, hs.cpu().numpy().tolist())) <= valid
        again = mem.gather(hs)
        for a, b in zip(out[:5], again):
            assert torch.equal(a, b)
    # the same seed and call index draw the same handles; the next call draws others
    mem.sample_calls.fill_(7)
    h1 = mem.sample(4096, seed=9, return_handles=True)[5].clone()
    assert int(mem.sample_calls.item()) == 8
    h2 = mem.sample(4096, seed=9, return_handles=True)[5].clone()
    mem.sample_calls.fill_(7)
    h3 = mem.sample(4096, seed=9, return_handles=True)[5].clone()
    assert torch.equal(h1, h3) and not torch.equal(h1, h2)
    mem.check()
    env.close()


def test_sample_is_uniform_over_transitions(evg):
    import torch
    env, mem, model = run_loop(evg, 8, "step_vs_q", turns=12, H=5, n=1, gather_at=(11,))
    tr = model.transitions()
    M = len(tr["slot"])
    assert 20 <= M <= 400
    index = {h: i for i, h in enumerate(zip(tr["slot"].tolist(), tr["env"].tolist(), tr["seat"].tolist(), tr["row"].tolist()))}
    counts = np.zeros(M, np.int64)
    draws = 0
    for call in range(16):
        h = mem.sample(65536, seed=123, return_handles=True)[5].cpu().numpy()
        counts += np.bincount([index[tuple(x)] for x in h.tolist()], minlength=M)
        draws += len(h)
    assert draws >= 10 ** 6
    p = 1.0 / M
    sigma = np.sqrt(draws * p * (1 - p))
    assert np.abs(counts - draws * p).max() < 5 * sigma, (counts.min(), counts.max(), draws * p, sigma)
    env.close()


def test_refusals_and_status(evg):
    import ctypes as C
    import torch
    env = evg.EvergladesVecEnv(256, seed=3)
    env.reset()
    with pytest.raises(ValueError):
        env.smart_replay(3, n_step=3)                                            # capacity must exceed n
    with pytest.raises(ValueError):
        env.smart_replay(4, seats=(1, 0))
    with pytest.raises(ValueError):
        env.smart_replay(4, shaping="no_such_shaping")
    mem = env.smart_replay(4, n_step=1)
    with pytest.raises(ValueError):
        mem.sample(0, seed=1)
    # a one-seat memory's views do not fit the two-seat step
    q = torch.zeros((256, 2, 12, 5), device=env.device)
    with pytest.raises(ValueError):
        env.step_q(q, 0.1, features=mem.slot_features(1), directions=mem.slot_directions(0))
    # the ABI refuses a misaligned buffer and too few slots
    L, d = env.L, mem._d
    bad = evg._lib.EvgReplay.from_buffer_copy(d)
    bad.meta = d.meta + 4
    with pytest.raises(evg.EvgError):
        evg._lib.check(L.evg_replay_record(env._h, C.byref(bad), 0, C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), None, None), L)
    bad = evg._lib.EvgReplay.from_buffer_copy(d)
    bad.slots = 2
    with pytest.raises(evg.EvgError):
        evg._lib.check(L.evg_replay_clear(env._h, C.byref(bad), None), L)
    # an empty memory: zeros and the EMPTY bit, not a host refusal
    obs, action, nxt, reward, nd = mem.sample(64, seed=1)
    assert not obs.any() and not action.any() and not nxt.any() and not reward.any() and not nd.any()
    assert mem.status() == evg._lib.REPLAY_S_EMPTY
    with pytest.raises(evg.EvgError):
        mem.check()
    mem.clear()
    assert mem.status() == 0
    # a handle that names no transition: zeros and the BAD_HANDLE bit
    h = torch.tensor([[0, 0, 0, 0], [99, 0, 0, 0], [0, 999, 0, 0], [0, 0, 1, 0], [0, 0, 0, 7]], dtype=torch.int32, device=env.device)
    obs, action, nxt, reward, nd = mem.gather(h)
    assert not obs.any() and not nxt.any() and not nd.any()
    assert mem.status() == evg._lib.REPLAY_S_BAD_HANDLE
    env.close()


def test_training_example_runs_with_a_finite_loss():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import torch
    import smart_state_training
    losses = smart_state_training.main(2048, 60, 256)
    assert len(losses) > 50 and bool(torch.isfinite(losses).all())
