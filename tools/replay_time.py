#!/usr/bin/env python3
"""Times the Smart_State replay memory on the MI355X (device events around many calls, after a warm-up):
  - evg_replay_record per turn;
  - evg_replay_sample at B = 1 024 and 65 536: microseconds and the fraction of 8 TB/s its OUTPUT bytes would take;
  - the training turn (step_vs_q) and the self-play turn (step_q) with and without record.

    python tools/replay_time.py [envs] [out_file]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

OUT_BYTES = 59 * 4 + 8 + 12 * 59 * 4 + 4 + 1 + 16            # swarm_obs, action, next_state, reward, not_done, handle per transition


def timed(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps                     # us per call


def main(N=65536, out=None):
    lines = ["device: %s, envs %d, torch %s" % (torch.cuda.get_device_name(0), N, torch.__version__)]
    env = evg.EvergladesVecEnv(N, seed=1)
    env.reset()
    dev = env.device
    # training turn: step_vs_q, one-seat memory
    mem = env.smart_replay(8, n_step=1, gamma=0.999, shaping="reward_short_games", seats=0)
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    q = torch.randn((N, 12, 5), device=dev)
    t = [0]

    def turn_vs(record):
        def f():
            env.step_vs_q("swarm", q, 0.1, seat=0, features=mem.slot_features(t[0] + 1), directions=mem.slot_directions(t[0]))
            if record:
                mem.record()
            t[0] += 1
        return f

    def rec_only():
        mem.record()

    us_vs = timed(turn_vs(False), 200)
    mem.clear(); t[0] = 0
    us_vs_rec = timed(turn_vs(True), 200)
    us_rec = timed(rec_only, 500)
    lines.append("training turn (step_vs_q): %.1f us without record, %.1f us with record; record alone %.2f us per turn" % (us_vs, us_vs_rec, us_rec))
    size = int(mem.size().item())
    lines.append("memory: %d transitions in %d kept turns" % (size, mem.H))
    for B in (1024, 65536):
        us = timed(lambda: mem.sample(B, seed=3), 200)
        byts = B * OUT_BYTES
        lines.append("sample B=%d: %.1f us (count + draw + gather), %.1f MB written, %.1f %% of 8 TB/s on the output bytes (%.2f TB/s)"
                     % (B, us, byts / 1e6, 100.0 * (byts / 8e12) / (us * 1e-6), byts / (us * 1e-6) / 1e12))
        hs = mem.sample(B, seed=3, return_handles=True)[5].clone()
        usg = timed(lambda: mem.gather(hs), 200)
        lines.append("gather B=%d: %.1f us, %.1f %% of 8 TB/s on the output bytes" % (B, usg, 100.0 * (B * (OUT_BYTES - 16) / 8e12) / (usg * 1e-6)))
    mem.check()
    # self-play turn: step_q, two-seat memory
    mem2 = env.smart_replay(8, n_step=1, gamma=0.999, shaping="reward_short_games", seats=(0, 1))
    q2 = torch.randn((N, 2, 12, 5), device=dev)
    t2 = [0]

    def turn_q(record):
        def f():
            env.step_q(q2, 0.1, features=mem2.slot_features(t2[0] + 1), directions=mem2.slot_directions(t2[0]))
            if record:
                mem2.record()
            t2[0] += 1
        return f

    us_q = timed(turn_q(False), 200)
    mem2.clear(); t2[0] = 0
    us_q_rec = timed(turn_q(True), 200)
    lines.append("self-play turn (step_q): %.1f us without record, %.1f us with record" % (us_q, us_q_rec))
    mem2.check()
    env.close()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 65536, a[1] if len(a) > 1 else None)
