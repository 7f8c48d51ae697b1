#!/usr/bin/env python3
"""Times the agents/DQN family's replay memory on the MI355X (include/evg_dqn_replay.h), float32 observations, a ring of 8 turns.

a) The memory work of one turn, at 4 096 envs / B = 128, 65 536 envs / B = 1 024 and 65 536 envs / B = 16 384:
  (1) mem.record() + mem.sample(B, seed)                                   (DqnReplay: record, scan, top, draw, gather)
  (2) mem.record() + mem.sample(B, seed, beta) + mem.update_priorities     (PrioritizedDqnReplay)
  (3) the torch ring of examples/dqn_training.py --device-learner as it stood before the memory: four copy_ into the ring (one of them the
      multiply-add of the unravelled action), torch.randint, four index-gathers
b) The whole training turn of examples/dqn_training.py (act, step, memory, learner step; h1 = 528) with --device-learner (the torch ring) against
   --device-replay, at 4 096 envs / B = 128 and 65 536 envs / B = 1 024.
c) The gather kernel alone at B = 16 384 (float32 and int16 rings of 65 536 envs) against the bytes it must move -- two source rows read and 840
   bytes written per transition -- as a fraction of the copy rate a plain device copy of the same number of bytes reaches in the same run.

Timing: stream time per call from device events around CALLS calls, after a warm-up of every form.  The forms ALTERNATE inside one process, ROUNDS
bursts each: the figure is the median of the bursts, the spread each form's own min .. max.

    python tools/dqn_replay_time.py [out_file]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import everglades_amd as evg

ROUNDS, WARM, RING = 9, 10, 8
H1, GAMMA, LR = 528, 0.99, 1e-4
SHAPES = ((4096, 128), (65536, 1024), (65536, 16384))


def burst(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                    # us per call


def alternate(forms, calls):
    """-> [(median, min, max)] per form: ROUNDS bursts of each, alternating"""
    for _ in range(WARM):
        for f in forms:
            f()
    torch.cuda.synchronize()
    t = [[] for _ in forms]
    for _ in range(ROUNDS):
        for i, f in enumerate(forms):
            t[i].append(burst(f, calls))
    return [(statistics.median(v), min(v), max(v)) for v in t]


def make_net(dev):
    return torch.nn.Sequential(torch.nn.Linear(105, H1), torch.nn.ReLU(), torch.nn.Linear(H1, 132), torch.nn.ReLU()).to(dev)


class TorchRing(object):
    """the ring, the draw and the gathers of examples/dqn_training.py --device-learner before the device memory"""

    def __init__(self, envs, dev):
        self.envs = envs
        self.mem = dict(state=torch.zeros((RING, envs, 105), device=dev), action=torch.zeros((RING, envs, 7), dtype=torch.int64, device=dev),
                        reward=torch.zeros((RING, envs), device=dev), next_state=torch.zeros((RING, envs, 105), device=dev))
        self.gen = torch.Generator(device=dev).manual_seed(2)
        self.dev, self.t = dev, 0

    def turn(self, obs, rows, reward, nxt, batch):
        mem, slot = self.mem, self.t % RING
        mem["state"][slot].copy_(obs)
        mem["action"][slot].copy_(rows[:, :, 0] * 11 + rows[:, :, 1])
        mem["reward"][slot].copy_(reward[:, 0])
        mem["next_state"][slot].copy_(nxt)
        filled = min(self.t + 1, RING) * self.envs
        idx = torch.randint(0, filled, (batch,), generator=self.gen, device=self.dev)
        self.t += 1
        return (mem["state"].view(-1, 105)[idx], mem["action"].view(-1, 7)[idx], mem["next_state"].view(-1, 105)[idx], mem["reward"].view(-1)[idx], None)


def filled_memory(env, prioritized):
    """a memory whose ring holds RING turns of a real game"""
    mem = env.dqn_prioritized_replay(RING) if prioritized else env.dqn_replay(RING)
    env.observe_seat(0, out=mem.slot_obs(0))
    for t in range(RING + 1):
        rows = env.random_actions_seat(0, out=mem.slot_actions(t))
        rows[:, :, 1].sub_(1).clamp_(0, 10)                       # {group, node 1..11} -> this family's {unit, node 0..10}
        env.step_vs("random_actions", rows, seat=0, out=mem.slot_obs(t + 1))
        mem.record()
    return mem


def time_memory(envs, B, lines):
    env = evg.EvergladesVecEnv(envs, seed=1, auto_reset=True)
    env.reset()
    dev = env.device
    mem, pmem = filled_memory(env, False), filled_memory(env, True)
    ring = TorchRing(envs, dev)
    obs, nxt = mem.slot_obs(0).clone(), mem.slot_obs(1).clone()
    rows = mem.slot_actions(0).clone()
    pr = torch.rand((B,), device=dev) + 0.01
    seed = [0]

    def f_uniform():
        seed[0] += 1
        mem.record()
        mem.sample(B, seed[0])

    def f_prioritized():
        seed[0] += 1
        pmem.record()
        out = pmem.sample(B, seed[0], 0.4)
        pmem.update_priorities(out[6], pr)

    def f_torch():
        ring.turn(obs, rows, env.reward, nxt, B)

    res = alternate([f_uniform, f_prioritized, f_torch], 100)
    names = ["(1) record + sample", "(2) record + sample(beta) + update_priorities", "(3) torch ring: 4 copy_, randint, 4 gathers"]
    for name, (med, lo, hi) in zip(names, res):
        lines.append("  %6d envs, B = %6d  %-46s %8.1f us  (%.1f .. %.1f, spread %.1f)" % (envs, B, name, med, lo, hi, hi - lo))
    spread = res[2][2] - res[2][1]
    for i in (0, 1):
        met = res[i][0] <= res[2][0] + spread
        lines.append("  %6d envs, B = %6d  %s / torch ring = %.3f: %s" % (envs, B, names[i][:3], res[i][0] / res[2][0],
                                                                         "not slower than the torch ring by more than its spread" if met else
                                                                         "SLOWER than the torch ring by more than its spread (%.1f us)" % spread))
    mem.check()
    pmem.check()
    env.close()


def time_turn(envs, B, lines):
    """the loop bodies of examples/dqn_training.py --device-learner and --device-replay"""
    forms = []
    envs_made = []
    for device_replay in (False, True):
        env = evg.EvergladesVecEnv(envs, seed=1, auto_reset=True)
        env.reset()
        envs_made.append(env)
        dev = env.device
        torch.manual_seed(1)
        policy, target = make_net(dev), make_net(dev)
        qnet = env.dqn_qnet(policy)
        learner = env.dqn_learner(policy, target, lr=LR, gamma=GAMMA, mode="huber", clamp=1.0)
        explored = torch.zeros(envs, dtype=torch.uint8, device=dev)
        if device_replay:
            mem = env.dqn_replay(RING)
            env.observe_seat(0, out=mem.slot_obs(0))

            def turn(env=env, mem=mem, qnet=qnet, learner=learner, explored=explored):
                t = mem.turn
                rows = env.dqn_get_action(qnet(mem.slot_obs(t)), 0.5, seat=0, out=mem.slot_actions(t), explored=explored)
                env.step_vs("random_actions", rows, seat=0, out=mem.slot_obs(t + 1))
                mem.record()
                learner.step(mem, B, seed=t)
        else:
            ring = TorchRing(envs, dev)
            state = {"obs": env.observe_seat(0)}

            def turn(env=env, ring=ring, qnet=qnet, learner=learner, explored=explored, state=state):
                obs, m, slot = state["obs"], ring.mem, ring.t % RING
                m["state"][slot].copy_(obs)
                rows = env.dqn_get_action(qnet(obs), 0.5, seat=0, explored=explored)
                m["action"][slot].copy_(rows[:, :, 0] * 11 + rows[:, :, 1])
                nxt, reward, done, info = env.step_vs("random_actions", rows, seat=0)
                m["reward"][slot].copy_(reward[:, 0])
                m["next_state"][slot].copy_(nxt)
                filled = min(ring.t + 1, RING) * envs
                idx = torch.randint(0, filled, (B,), generator=ring.gen, device=ring.dev)
                ring.t += 1
                learner.step_on((m["state"].view(-1, 105)[idx], m["action"].view(-1, 7)[idx], m["next_state"].view(-1, 105)[idx], m["reward"].view(-1)[idx], None))
                state["obs"] = nxt
        forms.append(turn)
    res = alternate(forms, 40)
    names = ["--device-learner (torch ring)", "--device-replay"]
    for name, (med, lo, hi) in zip(names, res):
        lines.append("  %6d envs, B = %6d  %-32s %8.1f us  (%.1f .. %.1f, spread %.1f)" % (envs, B, name, med, lo, hi, hi - lo))
    lines.append("  %6d envs, B = %6d  --device-replay / --device-learner = %.3f" % (envs, B, res[1][0] / res[0][0]))
    for env in envs_made:
        env.close()


def time_gather(dtype, lines):
    envs, B = 65536, 16384
    env = evg.EvergladesVecEnv(envs, seed=1, obs_dtype=dtype, auto_reset=True)
    env.reset()
    mem = filled_memory(env, False)
    handles = mem.sample(B, 1, return_handles=True)[5].clone()
    elem = mem.slot_obs(0).element_size()
    moved = B * (2 * 105 * elem + 2 * 105 * 4)                     # two rows read, 840 bytes written (the 73 bytes of metadata per row aside)
    src = torch.empty((moved // 2,), dtype=torch.uint8, device=env.device)
    dst = torch.empty_like(src)
    res = alternate([lambda: mem.gather(handles), lambda: dst.copy_(src)], 200)
    rates = [moved / r[0] * 1e-3 for r in res]                     # GB/s at the median
    lines.append("  %-8s gather of %d transitions: %8.1f us  (%.1f .. %.1f), %d bytes moved, %.0f GB/s" % (dtype, B, res[0][0], res[0][1], res[0][2], moved, rates[0]))
    lines.append("  %-8s copy_ of %d bytes (the same bytes moved): %8.1f us  (%.1f .. %.1f), %.0f GB/s; gather / copy rate = %.3f" % (
        dtype, moved // 2, res[1][0], res[1][1], res[1][2], rates[1], rates[0] / rates[1]))
    env.close()


def main(out=None):
    lines = ["device: %s, torch %s; %d alternating bursts per form (median, min .. max), warm-up %d calls of each" % (
        torch.cuda.get_device_name(0), torch.__version__, ROUNDS, WARM)]
    lines.append("a) the memory work of one turn, ring of %d turns, float32 observations:" % RING)
    for envs, B in SHAPES:
        time_memory(envs, B, lines)
    lines.append("b) the whole training turn of examples/dqn_training.py, h1 = %d:" % H1)
    for envs, B in SHAPES[:2]:
        time_turn(envs, B, lines)
    lines.append("c) the gather kernel alone against a plain device copy of the same bytes:")
    for dtype in ("float32", "int16"):
        time_gather(dtype, lines)
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
