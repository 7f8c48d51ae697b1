"""GPU tests of the agents/DQN family's replay memory on the device (everglades_amd.DqnReplay, include/evg_dqn_replay.h, libevg_dqnreplay.so) against
the host model (tests/dqn_replay_model.py), bit for bit:
  - a step_vs loop that writes its observations straight into the ring, gather of every live record after every turn;
  - episode ends fed through record(reward=, done=): not_done, zeroed next_state, the restarted turn counter, frozen envs, terminal_next;
  - a planted out-of-range unit or node; sample against the model's draw; an empty memory and one with a single valid record;
  - every batch size with canaries around the outputs and the ring; learner.step(mem) against sample + step_on, and a captured turn;
  - sampling by priority: handles against the model that holds the device's plane, importance weights, duplicates, stale stamps, wmax;
  - the example with --device-replay and with --prioritized."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import dqn_replay_model as dm

pytestmark = pytest.mark.gpu
CANARY = 0xA5
MARGIN = 256


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def past_caps(evg):
    """one batch size past the gather's and the draw's grid caps"""
    L = evg._lib
    return max(L.DQN_REPLAY_GATHER_MAX_BLOCKS * L.DQN_REPLAY_TILE, L.DQN_REPLAY_DRAW_MAX_BLOCKS * 256) + L.DQN_REPLAY_TILE + 1


def make(evg, N, H, dtype, auto_reset=True, shaping="reward_short_games", seed=3):
    env = evg.EvergladesVecEnv(N, seed=seed, obs_dtype=dtype, auto_reset=auto_reset)
    env.reset()
    mem = env.dqn_replay(H, shaping=shaping, seat=0)
    st = env.get_state()["env"]
    model = dm.DqnReplayModel(N, H, shaping, seat=0, auto_reset=auto_reset, turn0=st[:, 0], episode0=st[:, 2])
    return env, mem, model


def guard_ring(mem):
    """move the ring of observations between two runs of canary bytes (before slot 0, behind the last slot) and fill its padding with canaries"""
    import torch
    slots, stride = mem._obs.shape
    big = torch.full((MARGIN + slots * stride + MARGIN,), CANARY, dtype=torch.uint8, device=mem._obs.device)
    ring = big[MARGIN:MARGIN + slots * stride].view(slots, stride)
    dtype, N = mem.env.obs_dtype, mem.N
    elem = torch.empty((), dtype=dtype).element_size()
    mem._obs = ring
    mem._slot_obs = [ring[k, :N * 105 * elem].view(dtype).view(N, 105) for k in range(slots)]
    mem._d.obs = ring.data_ptr()
    assert ring.data_ptr() % 16 == 0
    for v in mem._slot_obs:
        v.zero_()
    return big, N * 105 * elem


def ring_canaries_intact(mem, big, used):
    slots, stride = mem._obs.shape
    b = big.cpu().numpy()
    body = b[MARGIN:MARGIN + slots * stride].reshape(slots, stride)
    return (b[:MARGIN] == CANARY).all() and (b[MARGIN + slots * stride:] == CANARY).all() and (body[:, used:] == CANARY).all()


class GuardedOutputs(object):
    """the memory's six output tensors for batch size B, each between two runs of canary bytes"""

    def __init__(self, mem, B):
        import torch
        dev = mem.env.device
        self.items = []
        outs = []
        for shape, dtype in (((B, 105), torch.float32), ((B, 7), torch.int64), ((B, 105), torch.float32), ((B,), torch.float32), ((B,), torch.bool),
                             ((B, 4), torch.int32)):
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            big = torch.full((MARGIN + nbytes + MARGIN,), CANARY, dtype=torch.uint8, device=dev)
            self.items.append((big, nbytes))
            outs.append(big[MARGIN:MARGIN + nbytes].view(dtype).view(*shape))
        mem._out[B] = tuple(outs)

    def intact(self):
        for big, nbytes in self.items:
            b = big.cpu().numpy()
            if not ((b[:MARGIN] == CANARY).all() and (b[MARGIN + nbytes:] == CANARY).all()):
                return False
        return True


def expected_batch(mem, model, handles, terminal_next=False):
    """the batch for handles int32 [B, 4] of VALID records, expanded with torch from the ring's own slots and the model's metadata"""
    import torch
    h = handles.long()
    slot, env = h[:, 0], h[:, 1]
    ring = torch.stack([mem.slot_obs(k) for k in range(mem.slots)])
    rows = torch.stack([mem.slot_actions(k) for k in range(mem.slots)]).long()
    hn = handles.cpu().numpy()
    nd = torch.as_tensor((model.meta[hn[:, 0], hn[:, 1], 2] & 1) != 0, device=h.device)
    state = ring[slot, env].to(torch.float32)
    nxt = ring[(slot + 1) % mem.slots, env].to(torch.float32)
    if not terminal_next:
        nxt = torch.where(nd[:, None], nxt, torch.zeros_like(nxt))
    action = rows[slot, env, :, 0] * 11 + rows[slot, env, :, 1]
    reward = torch.as_tensor(model.rew[hn[:, 0], hn[:, 1]].astype(np.float32), device=h.device)
    return state, action, nxt, reward, nd


def same(got, want):
    import torch
    names = ["state", "action", "next_state", "reward", "not_done"]
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype == torch.float32:
            assert torch.equal(g.view(torch.int32), w.contiguous().view(torch.int32)), name          # bit for bit
        else:
            assert torch.equal(g, w), name


def check_state(mem, model):
    assert np.array_equal(mem.valid.cpu().numpy(), model.valid)
    assert np.array_equal(mem.meta.cpu().numpy(), model.meta)
    assert np.array_equal(mem.rewards.cpu().numpy().view(np.uint64), model.rew.view(np.uint64))
    assert np.array_equal(mem.env_state.cpu().numpy(), model.ctr)
    assert int(mem.size().item()) == model.size()


def check_all_live(mem, model, terminal_next=False):
    import torch
    h = model.handles()
    if len(h):
        ht = torch.as_tensor(h, device=mem.env.device)
        same(mem.gather(ht, terminal_next=terminal_next), expected_batch(mem, model, ht, terminal_next))


def plant_obs(mem, t, rng):
    """values that exercise the conversion: the whole int16 range; float64 values that are no float32; float32 bit patterns as they are"""
    import torch
    v = mem.slot_obs(t)
    if v.dtype == torch.int16:
        a = rng.integers(-32768, 32768, v.shape).astype(np.int16)
        a.flat[:2] = (-32768, 32767)
    elif v.dtype == torch.float64:
        a = rng.standard_normal(v.shape) * 1000.0
        a.flat[:2] = (1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24)                 # ties of the float32 rounding: to even
    else:
        a = (rng.standard_normal(v.shape) * 1000.0).astype(np.float32)
    v.copy_(torch.as_tensor(a, device=v.device))


def random_rows(N, rng):
    return np.stack([np.stack([rng.permutation(12)[:7], rng.permutation(11)[:7]], 1) for _ in range(N)]).astype(np.int32)


def planted_loop(mem, model, turns, rng, done_at=None, bad=None, each=None):
    """`turns` turns of planted observations, rows, rewards and episode ends through the device and the model"""
    import torch
    dev, N = mem.env.device, mem.N
    if mem.turn == 0:
        plant_obs(mem, 0, rng)
    for _ in range(turns):
        t = mem.turn
        rows = random_rows(N, rng)
        if bad is not None and bad[0] == t:
            rows[bad[1], bad[2], bad[3]] = bad[4]
        mem.slot_actions(t).copy_(torch.as_tensor(rows, device=dev))
        plant_obs(mem, t + 1, rng)
        reward = rng.random((N, 2)).astype(np.float32)
        done = np.zeros(N, np.uint8)
        done[list((done_at or {}).get(t, ()))] = 1
        mem.record(torch.as_tensor(reward, device=dev), torch.as_tensor(done, device=dev))
        model.record(rows, reward, done)
        if each is not None:
            each(t)


# ---------------------------------------------------------------------- 1. the step loop writes the ring
@pytest.mark.parametrize("N,H,dtype", [(1, 2, "int16"), (5, 3, "float32"), (67, 2, "float64"), (67, 3, "int16")])
def test_step_loop_writes_the_ring_and_every_live_record_gathers(evg, N, H, dtype):
    import torch
    env, mem, model = make(evg, N, H, dtype)
    big, used = guard_ring(mem)
    torch.manual_seed(N)
    net = torch.nn.Sequential(torch.nn.Linear(105, 8), torch.nn.ReLU(), torch.nn.Linear(8, 132), torch.nn.ReLU()).to(env.device)
    qnet = env.dqn_qnet(net)
    assert env.observe_seat(0, out=mem.slot_obs(0)).data_ptr() == mem.slot_obs(0).data_ptr()
    for t in range(2 * H + 3):
        obs_t = mem.slot_obs(t).clone()
        rows = env.dqn_get_action(qnet(mem.slot_obs(t)), 0.5, seat=0, out=mem.slot_actions(t))
        assert rows.data_ptr() == mem.slot_actions(t).data_ptr()
        obs, reward, done, info = env.step_vs("random_actions", rows, seat=0, out=mem.slot_obs(t + 1))
        assert obs.data_ptr() == mem.slot_obs(t + 1).data_ptr() and torch.equal(mem.slot_obs(t), obs_t)      # stored once, in place
        mem.record()
        model.record(rows.cpu().numpy(), env.reward.cpu().numpy(), env.done.cpu().numpy())
        check_state(mem, model)
        check_all_live(mem, model)
        assert model.size() == min(t + 1, H) * N
    assert ring_canaries_intact(mem, big, used)
    assert mem.status() == 0
    mem.check()
    env.close()


# ---------------------------------------------------------------------- 2. episode ends
@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
@pytest.mark.parametrize("auto_reset", [True, False])
def test_episode_ends_not_done_zeroed_next_state_and_frozen_envs(evg, dtype, auto_reset):
    N, H = 5, 3
    env, mem, model = make(evg, N, H, dtype, auto_reset=auto_reset)
    rng = np.random.default_rng(5)
    done_at = {1: [0, 3], 2: [4], 5: [0], 6: [1, 2]}
    seen = {"terminal": 0}

    def each(t):
        check_state(mem, model)
        check_all_live(mem, model)
        if not auto_reset:
            check_all_live(mem, model, terminal_next=True)
        r = model.records()
        seen["terminal"] += int((~r["not_done"]).sum())

    planted_loop(mem, model, 2 * H + 3, rng, done_at=done_at, each=each)
    assert seen["terminal"] > 0
    if auto_reset:
        assert model.ctr[0].tolist()[:2] == [2 * H + 3 - 6, 2] and (model.ctr[:, 3] == 0).all()      # the turn counter restarted twice for env 0
        with pytest.raises(ValueError, match="terminal_next"):
            mem.sample(4, 1, terminal_next=True)
        import ctypes as C
        o = [C.c_void_p(t.data_ptr()) for t in mem._outputs(4)]
        rc = mem.R.evg_dqn_replay_sample(env._h, C.byref(mem._d), 4, 1, evg._lib.DQN_REPLAY_TERMINAL_NEXT, *o, env._stream())
        assert rc == -1 and "auto_reset" in mem.R.evg_last_error().decode()
    else:
        assert model.ctr[:, 3].tolist() == [1, 1, 1, 1, 1] and model.size() == 2                    # all frozen: only the last two terminal records are left
    assert mem.status() == 0
    env.close()


def test_shaped_reward_uses_the_envs_own_turn_and_episode_counters(evg):
    """reward_short_games' (150 - turn) / 150 and transition's episode ratio, with the counters taken from the handle at clear()"""
    for shaping in ("reward_short_games", ("transition", "basic_reward", "reward_short_games", 3), "penalize_long_games", "normalized_score"):
        env, mem, model = make(evg, 5, 2, "float32", shaping=shaping)
        for _ in range(7):
            env.step(env.random_actions())
        mem.clear()
        st = env.get_state()["env"]
        assert (st[:, 0] == 7).all()
        model = dm.DqnReplayModel(5, 2, shaping, turn0=st[:, 0], episode0=st[:, 2])
        planted_loop(mem, model, 6, np.random.default_rng(1), done_at={1: [0, 1, 2], 4: [0, 3]}, each=lambda t: check_state(mem, model))
        assert model.rew.any()
        env.close()
    env, mem, model = make(evg, 3, 2, "float32", shaping="custom")
    import torch
    custom = torch.tensor([0.1, -2.5, 3.0], device=env.device)
    plant_obs(mem, 0, np.random.default_rng(0))
    mem.slot_actions(0).copy_(torch.as_tensor(random_rows(3, np.random.default_rng(0)), device=env.device))
    mem.record(shaped=custom)
    assert np.array_equal(mem.rewards[0].cpu().numpy(), custom.cpu().numpy().astype(np.float64))
    env.close()


# ---------------------------------------------------------------------- 3. action validity
@pytest.mark.parametrize("col,value", [(0, 12), (0, -1), (1, 11), (1, -7), (0, 1 << 20)])
def test_an_out_of_range_unit_or_node_is_no_transition(evg, col, value):
    import torch
    N, H = 5, 3
    env, mem, model = make(evg, N, H, "int16")
    rng = np.random.default_rng(9)
    planted_loop(mem, model, 3, rng, bad=(1, 2, 6, col, value), each=lambda t: check_state(mem, model))
    assert model.size() == 3 * N - 1 and model.valid[1, 2] == 0
    assert mem.status() == evg._lib.DQN_REPLAY_S_BAD_ACTION == model.status
    check_all_live(mem, model)                                                                     # all other envs unaffected
    for seed in range(4):                                                                          # never drawn
        h = mem.sample(257, seed, return_handles=True)[5].cpu().numpy()
        assert not ((h[:, 0] == 1) & (h[:, 1] == 2)).any()
    bad = torch.tensor([[1, 2, 0, 0], [1, 1, 0, 0]], dtype=torch.int32, device=env.device)
    got = [t.clone() for t in mem.gather(bad)]
    assert not any(t[0].any() for t in got) and got[0][1].any()                                    # zeros for the bad record, env 1 as ever
    same([t[1:] for t in got], expected_batch(mem, model, bad[1:]))
    assert mem.status() == evg._lib.DQN_REPLAY_S_BAD_ACTION | evg._lib.REPLAY_S_BAD_HANDLE
    with pytest.raises(evg.EvgError, match="order rows"):
        mem.check()
    env.close()


# ---------------------------------------------------------------------- 4. sample
@pytest.mark.parametrize("N,H,dtype", [(5, 3, "float32"), (67, 2, "int16")])
def test_sample_draws_the_models_handles_and_equals_gather(evg, N, H, dtype):
    import torch
    env, mem, model = make(evg, N, H, dtype)
    planted_loop(mem, model, H + 2, np.random.default_rng(2), done_at={1: [0], H: [N - 1]}, bad=(H, 0, 0, 0, 12))
    call = 0
    for seed, B in ((0, 1), (1, 3), (2, 7), (0xFFFFFFFFFFFFFFFF, 64), (1 << 40, 257)):
        assert int(mem.sample_calls.item()) == call
        out = [t.clone() for t in mem.sample(B, seed, return_handles=True)]
        want = model.draw(seed, call, B)
        assert np.array_equal(out[5].cpu().numpy(), want)
        same(out[:5], mem.gather(out[5]))
        same(out[:5], expected_batch(mem, model, out[5]))
        call += 1
    mem.sample_calls.fill_((1 << 33) + 5)                                                           # a call index past 32 bits
    h = mem.sample(64, 7, return_handles=True)[5].cpu().numpy()
    assert np.array_equal(h, model.draw(7, (1 << 33) + 5, 64))
    mem.sample_calls.fill_(1)                                                                       # assign it to repeat a draw
    assert np.array_equal(mem.sample(3, 1, return_handles=True)[5].cpu().numpy(), model.draw(1, 1, 3))
    env.close()


def test_empty_memory_and_a_single_valid_record(evg):
    import torch
    env, mem, model = make(evg, 5, 2, "float64")
    g = GuardedOutputs(mem, 7)
    out = mem.sample(7, 3, return_handles=True)
    assert not any(t.any() for t in out[:5]) and (out[5] == -1).all() and g.intact()
    assert mem.status() == evg._lib.REPLAY_S_EMPTY and int(mem.size().item()) == 0
    with pytest.raises(evg.EvgError, match="empty"):
        mem.check()
    mem.clear()
    assert mem.status() == 0
    # one valid record: every other env plays a wild row
    rng = np.random.default_rng(4)
    plant_obs(mem, 0, rng)
    rows = random_rows(5, rng)
    rows[[0, 1, 2, 4], 3, 1] = 11
    mem.slot_actions(0).copy_(torch.as_tensor(rows, device=env.device))
    plant_obs(mem, 1, rng)
    reward, done = rng.random((5, 2)).astype(np.float32), np.zeros(5, np.uint8)
    mem.record(torch.as_tensor(reward, device=env.device), torch.as_tensor(done, device=env.device))
    model.record(rows, reward, done)
    check_state(mem, model)
    assert model.size() == 1
    out = mem.sample(7, 9, return_handles=True)
    assert (out[5].cpu().numpy() == np.array([0, 3, 0, 0])).all() and np.array_equal(out[5].cpu().numpy(), model.draw(9, 0, 7))
    same(out[:5], expected_batch(mem, model, out[5]))
    env.close()


# ---------------------------------------------------------------------- 6. batch sizes, guard bands
@pytest.mark.parametrize("N,H,dtype", [(67, 3, "int16"), (5, 2, "float32"), (1, 2, "float64"), (67, 2, "float64")])
def test_every_batch_size_with_canaries_around_the_outputs_and_the_ring(evg, N, H, dtype):
    import torch
    env, mem, model = make(evg, N, H, dtype)
    big, used = guard_ring(mem)
    planted_loop(mem, model, H + 1, np.random.default_rng(N), done_at={H: [0]})
    live = model.handles()
    rng = np.random.default_rng(12)
    for B in (1, 3, 7, 64, 257, past_caps(evg)):
        g = GuardedOutputs(mem, B)
        h = live[rng.integers(0, len(live), B)]
        last = live[(live[:, 1] == N - 1)]
        h[-1] = last[np.argmax(last[:, 0])]                                                        # the last env of the highest live slot
        h[0] = [mem.slots - 1, N - 1, 0, 0]                                                        # the last env of the last slot, valid or not
        if B > 2:
            h[1] = [mem.slots, 0, 0, 0]                                                            # and a handle past the ring: zeros
        ht = torch.as_tensor(h, device=env.device)
        got = mem.gather(ht)
        ok = np.array([0 <= k < mem.slots and model.valid[k, e] != 0 for k, e, _, _ in h])
        want = expected_batch(mem, model, torch.as_tensor(np.where(ok[:, None], h, live[0]), device=env.device))
        okt = torch.as_tensor(ok, device=env.device)
        want = [torch.where(okt.view(-1, *([1] * (w.dim() - 1))), w, torch.zeros_like(w)) for w in want]
        same(got, want)
        assert g.intact(), B
        out = mem.sample(B, B, return_handles=True)
        assert g.intact(), B
        same(out[:5], expected_batch(mem, model, out[5]))
        first = max(0, B - 257)                                                                     # (the tail: draws past the draw kernel's grid cap)
        assert np.array_equal(out[5].cpu().numpy()[first:], model.draw(B, int(mem.sample_calls.item()) - 1, B, first=first))
        del mem._out[B]
    assert ring_canaries_intact(mem, big, used)
    env.close()


# ---------------------------------------------------------------------- 7. the learner's step from the memory
def _nets(env, h1=48):
    import torch
    torch.manual_seed(3)
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(105, h1), torch.nn.ReLU(), torch.nn.Linear(h1, 132), torch.nn.ReLU()).to(env.device)
    a, b, target = mk(), mk(), mk()
    b.load_state_dict(a.state_dict())
    with torch.no_grad():
        for net in (a, b, target):
            net[0].weight.mul_(0.02)                                           # observations reach the thousands: keep the hidden layer O(1)
    b.load_state_dict(a.state_dict())
    return a, b, target


@pytest.mark.parametrize("B", [7, 129])
def test_learner_step_from_the_memory_equals_sample_then_step_on(evg, B):
    import torch
    env, mem, model = make(evg, 67, 3, "int16")
    planted_loop(mem, model, 4, np.random.default_rng(6), done_at={2: [0, 1, 2, 3, 4, 5]})
    a, b, target = _nets(env)
    la, lb = env.dqn_learner(a, target, lr=1e-3), env.dqn_learner(b, target, lr=1e-3)
    for seed in (1, 2, 3):
        calls = mem.sample_calls.clone()
        loss_a = la.step(mem, B, seed).clone()
        assert int(mem.sample_calls.item()) == int(calls.item()) + 1
        mem.sample_calls.copy_(calls)
        batch = [t.clone() for t in mem.sample(B, seed)]
        loss_b = lb.step_on(tuple(batch)).clone()
        assert torch.equal(loss_a, loss_b) and torch.isfinite(loss_a) and float(loss_a) > 0
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
        assert all(torch.equal(p, q) for p, q in zip(la.m + la.v + [la.ctl], lb.m + lb.v + [lb.ctl]))
    assert not all(torch.equal(p, q) for p, q in zip(a.parameters(), _nets(env)[0].parameters()))   # the steps moved the parameters
    env.close()


def test_a_captured_turn_replayed_equals_the_eager_turn(evg):
    """act, step, record, learner step: two envs of one seed play K eager turns; one then plays turn K eagerly, the other replays its capture"""
    import torch
    K, B = 3, 64
    results = []
    for captured in (False, True):
        env, mem, model = make(evg, 67, 3, "float32", seed=21)
        policy, _, target = _nets(env)
        qnet = env.dqn_qnet(policy)
        learner = env.dqn_learner(policy, target, lr=1e-3)
        env.observe_seat(0, out=mem.slot_obs(0))

        def turn(t):
            rows = env.dqn_get_action(qnet(mem.slot_obs(t)), 0.3, seat=0, out=mem.slot_actions(t))
            env.step_vs("random_actions", rows, seat=0, out=mem.slot_obs(t + 1))
            mem.record()
            learner.step(mem, B, seed=t)

        for t in range(K):
            turn(t)
        if captured:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                turn(K)
            g.replay()
        else:
            turn(K)
        torch.cuda.synchronize()
        results.append([t.clone().cpu() for t in list(policy.parameters()) + learner.m + learner.v +
                        [learner.ctl, learner.loss, mem._obs, mem._actions, mem.rewards, mem.meta, mem.valid, mem.env_state, mem.ctl] + list(mem._outputs(B))])
        assert mem.status() == 0
        env.close()
    assert all(torch.equal(x, y) for x, y in zip(*results))


# ---------------------------------------------------------------------- 5. sampling by priority
import dqn_replay_priority_model as pm     # noqa: E402


def make_prioritized(evg, N, H, dtype, alpha=0.6, auto_reset=True):
    env = evg.EvergladesVecEnv(N, seed=3, obs_dtype=dtype, auto_reset=auto_reset)
    env.reset()
    mem = env.dqn_prioritized_replay(H, alpha=alpha, shaping="reward_short_games", seat=0)
    st = env.get_state()["env"]
    model = dm.DqnReplayModel(N, H, "reward_short_games", seat=0, auto_reset=auto_reset, turn0=st[:, 0], episode0=st[:, 2])
    return env, mem, model, pm.DqnPriorityModel(model, alpha)


def load_plane(mem, pmodel):
    pmodel.load(mem.priorities.cpu().numpy(), mem.stamps.cpu().numpy(), float(mem.wmax.item()))


def same_plane(mem, pmodel):
    """the device's weights, stamps and wmax against the model's, on the records the model knows updated (elsewhere both count as never updated)"""
    fresh = (pmodel.stamps == pmodel.record_stamps()) & (pmodel.base.valid != 0)
    w, st = mem.priorities.cpu().numpy(), mem.stamps.cpu().numpy().view(np.uint32)
    assert np.array_equal(w.view(np.uint32)[fresh], pmodel.weights.view(np.uint32)[fresh]) and np.array_equal(st[fresh], pmodel.stamps[fresh])
    assert np.float32(mem.wmax.item()) == pmodel.wmax


@pytest.mark.parametrize("N,H,dtype,alpha", [(5, 3, "float32", 0.6), (67, 2, "int16", 1.0), (67, 3, "float64", 0.0)])
def test_prioritized_sample_update_and_weights(evg, N, H, dtype, alpha):
    import torch
    env, mem, model, pmodel = make_prioritized(evg, N, H, dtype, alpha)
    dev = env.device
    rng = np.random.default_rng(8)
    planted_loop(mem, model, H, rng, done_at={1: [0]}, bad=(1, N - 1, 2, 0, 12))
    assert float(mem.wmax.item()) == 1.0 and not mem.priorities.any()
    call = 0
    for rnd, (B, beta) in enumerate(((7, 0.4), (64, 1.0), (257, 0.0), (3, 0.7), (1, 0.4), (past_caps(evg), 0.4))):
        load_plane(mem, pmodel)
        g = GuardedOutputs(mem, B)
        out = mem.sample(B, 100 + rnd, beta)
        assert len(out) == 7 and g.intact()
        handles, idx = pmodel.draw(100 + rnd, call, B)
        call += 1
        assert np.array_equal(out[6].cpu().numpy(), handles)                                       # bit-equal to the model holding the device's plane
        want = pmodel.importance(idx, beta)
        got = out[5].cpu().numpy()
        assert np.abs(got / want - 1).max() <= 1e-6 and got.max() == 1.0
        if beta == 0.0:
            assert (got == 1.0).all()
        same(out[:5], expected_batch(mem, model, out[6]))
        # hand priorities back; duplicates of a record in one update keep the largest
        pr = rng.uniform(0.01, 30.0, B).astype(np.float32)
        mem.update_priorities(out[6], torch.as_tensor(pr, device=dev))
        pmodel.update(handles, pr)
        same_plane(mem, pmodel)
        del mem._out[B]
    assert mem.status() == evg._lib.DQN_REPLAY_S_BAD_ACTION                                        # the planted row; nothing else
    # the uniform draw over the same memory shares the call counter
    h = mem.uniform_sample(64, 5, return_handles=True)[5].cpu().numpy()
    assert np.array_equal(h, model.draw(5, call, 64))
    env.close()


def test_priority_duplicates_bad_priorities_stale_stamps_and_wmax(evg):
    import torch
    N, H = 5, 2
    env, mem, model, pmodel = make_prioritized(evg, N, H, "float32", 0.6)
    dev = env.device
    rng = np.random.default_rng(10)
    planted_loop(mem, model, 2, rng)
    t = lambda a, dt: torch.as_tensor(np.asarray(a, dt), device=dev)
    rec = [0, 3, 0, 0]
    for pr in ([0.5, 7.0, 2.0], [7.0, 2.0, 0.5], [2.0, 0.5, 7.0]):                                  # the largest of the duplicates, in any order
        mem.update_priorities(t([rec] * 3, np.int32), t(pr, np.float32))
        pmodel.update([rec] * 3, pr)
        assert np.float32(mem.priorities[0, 3].item()) == pm.weight(np.float32(7.0), 0.6)
    mem.update_priorities(t([rec], np.int32), t([0.25], np.float32))                               # a later update replaces it, smaller or not
    pmodel.update([rec], [0.25])
    assert np.float32(mem.priorities[0, 3].item()) == pm.weight(np.float32(0.25), 0.6)
    assert np.float32(mem.wmax.item()) == pm.weight(np.float32(7.0), 0.6) == pmodel.wmax           # wmax never falls
    same_plane(mem, pmodel)
    before = mem.priorities.clone()
    mem.update_priorities(t([[0, 0, 0, 0], [0, 1, 0, 0], [0, 2, 0, 0], [0, 4, 0, 0]], np.int32), t([np.nan, np.inf, 0.0, -1.0], np.float32))
    assert mem.status() == evg._lib.DQN_REPLAY_S_BAD_PRIORITY and torch.equal(mem.priorities, before)
    with pytest.raises(evg.EvgError, match="priority"):
        mem.check()
    mem.update_priorities(t([[2, 0, 0, 0], [0, 5, 0, 0], [0, 0, 1, 0], [3, 0, 0, 0]], np.int32), t([1.0] * 4, np.float32))       # slot 2 is empty
    assert mem.status() == evg._lib.DQN_REPLAY_S_BAD_PRIORITY | evg._lib.REPLAY_S_BAD_HANDLE and torch.equal(mem.priorities, before)
    # a never-updated record weighs wmax as of the draw: the probabilities of the model that holds the device's plane
    load_plane(mem, pmodel)
    eff = pmodel.effective()
    assert (eff == pmodel.wmax).sum() == len(eff) - 1
    out = mem.sample(257, 1, 0.5)
    handles, idx = pmodel.draw(1, 0, 257)
    assert np.array_equal(out[6].cpu().numpy(), handles)
    # the slot is reused: the stale stamp means "never updated", though the weight is still stored
    planted_loop(mem, model, H + 1, rng)
    assert model.valid[0, 3] == 1 and float(mem.priorities[0, 3].item()) != 0.0
    load_plane(mem, pmodel)
    assert (pmodel.effective() == pmodel.wmax).all()
    out = mem.sample(64, 2, 0.5)
    assert np.array_equal(out[6].cpu().numpy(), pmodel.draw(2, 1, 64)[0])
    mem.clear()
    assert float(mem.wmax.item()) == 1.0 and not mem.priorities.any() and mem.status() == 0
    env.close()


def test_prioritized_sample_of_an_empty_memory(evg):
    env, mem, model, pmodel = make_prioritized(evg, 5, 2, "int16")
    out = mem.sample(7, 1, 0.4)
    assert not any(t.any() for t in out[:6]) and (out[6] == -1).all()
    assert mem.status() == evg._lib.REPLAY_S_EMPTY
    env.close()


def test_learner_step_from_the_prioritized_memory(evg):
    """learner.step(mem, B, seed, beta) == mem.sample, step_on with its weights, update_priorities with the TD head's priorities: parameters, loss, plane"""
    import torch
    B = 129
    env, mem, model, pmodel = make_prioritized(evg, 67, 3, "int16")
    planted_loop(mem, model, 4, np.random.default_rng(6), done_at={2: [0, 1, 2, 3, 4, 5]})
    a, b, target = _nets(env)
    kw = dict(lr=1e-3, mode="squared", clamp=None)
    la, lb = env.dqn_learner(a, target, **kw), env.dqn_learner(b, target, **kw)
    for seed in (1, 2, 3):
        calls, plane, stamps, pctl = mem.sample_calls.clone(), mem.priorities.clone(), mem.stamps.clone(), mem.pctl.clone()
        loss_a = la.step(mem, B, seed, beta=0.4).clone()
        after = [mem.priorities.clone(), mem.stamps.clone(), mem.pctl.clone()]
        mem.sample_calls.copy_(calls)
        mem.priorities.copy_(plane)
        mem.stamps.copy_(stamps)
        mem.pctl.copy_(pctl)
        out = [t.clone() for t in mem.sample(B, seed, 0.4)]
        loss_b, prios = lb.step_on(tuple(out[:5]), weights=out[5])
        mem.update_priorities(out[6], prios)
        assert torch.equal(loss_a, loss_b.clone()) and torch.isfinite(loss_a)
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
        assert all(torch.equal(x, y) for x, y in zip(after, [mem.priorities, mem.stamps, mem.pctl]))
        assert len(np.unique(out[6].cpu().numpy(), axis=0)) < B                                    # duplicates were in the update
        # the update is idempotent under its duplicates: once more, nothing changes
        mem.update_priorities(out[6], prios)
        assert torch.equal(after[0], mem.priorities)
    # beta=None on a prioritized memory draws uniformly
    calls = mem.sample_calls.clone()
    loss_a = la.step(mem, B, 9).clone()
    mem.sample_calls.copy_(calls)
    loss_b = lb.step_on(tuple(t.clone() for t in mem.uniform_sample(B, 9))).clone()
    assert torch.equal(loss_a, loss_b)
    with pytest.raises(ValueError, match="prioritized"):
        la.step(env.dqn_replay(2), 4, 1, beta=0.4)
    env.close()


# ---------------------------------------------------------------------- 8. the example
def test_training_example_runs_with_the_device_replay():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dqn_training.py"), "64", "40", "128", "--device-replay"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device replay" in out.stdout and "all finite: True" in out.stdout


def test_training_example_runs_with_the_prioritized_device_replay():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dqn_training.py"), "64", "40", "128", "--device-replay", "--prioritized"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "prioritized" in out.stdout and "all finite: True" in out.stdout
