#!/usr/bin/env python3
"""Stream time of the Minimized agents' hot path at 65 536 envs, each against its Smart_State counterpart, alternating in one process on one device:

  turn   step_vs_q with the 11-way head (evg_step_vs_policy_minimized_q) | step_vs_q with the 5-way head (evg_step_vs_policy_smart_q) |
         this change's own two-launch composition minimized_get_action + step_vs(features=...)
  qnet   MinimizedQNet 59-80-11 | SmartQNet 59-60-60-5, compact layout, 65 536 x 12 rows

Each figure is the median over ROUNDS alternations of the mean of a window of calls between two stream events; a window is sized per case, from a
calibration run after the warm-up, to last at least WINDOW_MS of stream time (a shorter window measures the clock ramp and the scheduler).  The envs
keep playing, so every round sees fresh states.  Prints one line per round, then median, min and max per case; redirect to
profiles/r11_b_minimized_time.txt.

    python tools/minimized_time.py [envs] [rounds] [window_ms]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def main(N=65536, rounds=9, window_ms=300):
    env = evg.EvergladesVecEnv(N, seed=5, auto_reset=True)
    env.reset()
    dev = env.device
    g = torch.Generator(device="cpu").manual_seed(0)
    q11 = torch.randn((N, 12, 11), generator=g).to(dev)
    q5 = torch.randn((N, 12, 5), generator=g).to(dev)
    shared, swarm = torch.zeros((N, 34), device=dev), torch.zeros((N, 12, 13), device=dev)
    rows = torch.zeros((N, 7, 2), dtype=torch.int32, device=dev)
    env.smart_state_compact(-1, env.observe_seat(0), shared, swarm)
    torch.manual_seed(0)
    mini = torch.nn.Sequential(torch.nn.Linear(59, 80), torch.nn.ReLU(), torch.nn.Linear(80, 11), torch.nn.ReLU()).to(dev)
    smart = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5), torch.nn.ReLU()).to(dev)
    nm, ns = env.minimized_qnet(mini), env.smart_qnet(smart)
    o11, o5 = torch.zeros((N, 12, 11), device=dev), torch.zeros((N, 12, 5), device=dev)

    def two_launch():
        env.minimized_get_action(q11, 0.3, out=rows)
        env.step_vs("swarm", rows, features=(shared, swarm))

    cases = [("turn_minimized_q", lambda: env.step_vs_q("swarm", q11, 0.3, features=(shared, swarm), actions_out=rows)),
             ("turn_smart_q", lambda: env.step_vs_q("swarm", q5, 0.3, features=(shared, swarm), actions_out=rows)),
             ("turn_two_launch", two_launch),
             ("qnet_minimized_80", lambda: nm(shared, swarm, out=o11)),
             ("qnet_smart_60_60", lambda: ns(shared, swarm, out=o5))]
    reps = {}
    for k, fn in cases:
        timed(fn, 200)
        reps[k] = max(200, int(window_ms * 1000.0 / timed(fn, 200)) + 1)
    print("%d envs, %d rounds, calls per window: " % (N, rounds) + "  ".join("%s %d" % (k, reps[k]) for k, _ in cases), flush=True)
    res = {k: [] for k, _ in cases}
    for r in range(rounds):
        for k, fn in cases:
            res[k].append(timed(fn, reps[k]))
        print("round %d: " % r + "  ".join("%s %.2f us" % (k, res[k][-1]) for k, _ in cases), flush=True)
    for k, v in res.items():
        print("%-20s median %.2f us  min %.2f  max %.2f" % (k, statistics.median(v), min(v), max(v)))
    env.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(*a)
