#!/usr/bin/env python3
"""Stream time of the Minimized self-play turn at 65 536 envs, alternating in one process on one device:

  fused          step_q with the 11-way head and features (evg_step_minimized_q): one launch
  five_calls     the same turn on the entry points there were before it: minimized_get_action for seat 0 and seat 1, the two row tensors stacked into
                 [N, 2, 7, 2] (torch.stack into a preallocated tensor: one more small launch), step, smart_state_compact for player 0 and player 1
  league_all_q   step_q(league=...) (evg_step_league_minimized_q), league ["q", "random_actions_delay"], every env assigned to the network member
  league_all_bot ... every env assigned to the bot
  league_half    ... even envs to the network, odd envs to the bot (both kinds in every wavefront)

The leagues are created with resample=False and a caller-written assignment, so the mix stays what the case says while the envs keep playing.  Each
figure is the median over ROUNDS alternations of the mean of a window of calls between two stream events; a window is sized per case, from a calibration
run after the warm-up, to last at least WINDOW_MS of stream time.  Prints one line per round, then median, min and max per case; redirect to
profiles/r12_b_minimized_self_play_time.txt.

    python tools/minimized_self_play_time.py [envs] [rounds] [window_ms]
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
    q = torch.randn((N, 2, 12, 11), generator=g).to(dev)
    qs = [q[:, p].contiguous() for p in range(2)]
    feat = (torch.zeros((N, 2, 34), device=dev), torch.zeros((N, 2, 12, 13), device=dev))
    feats = [(torch.zeros((N, 34), device=dev), torch.zeros((N, 12, 13), device=dev)) for _ in range(2)]
    rows2 = torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=dev)
    rows = [torch.zeros((N, 7, 2), dtype=torch.int32, device=dev) for _ in range(2)]
    explored = torch.zeros((N, 2), dtype=torch.uint8, device=dev)
    eps = (0.3, 0.3)

    def five_calls():
        for p in range(2):
            env.minimized_get_action(qs[p], eps[p], seat=p, out=rows[p])
        torch.stack(rows, dim=1, out=rows2)
        obs = env.step(rows2)[0]
        for p in range(2):
            env.smart_state_compact(p, obs, *feats[p])

    leagues = {}
    for name, assign in (("league_all_q", torch.zeros(N, dtype=torch.uint8)), ("league_all_bot", torch.ones(N, dtype=torch.uint8)),
                         ("league_half", (torch.arange(N) % 2).to(torch.uint8))):
        lg = env.opponent_league(["q", "random_actions_delay"], seat=0, resample=False)
        lg.assign.copy_(assign.to(dev))
        leagues[name] = lg

    def league_turn(lg):
        return lambda: env.step_q(q, eps, features=feat, actions_out=rows2, explored=explored, league=lg)

    cases = [("fused", lambda: env.step_q(q, eps, features=feat, actions_out=rows2, explored=explored)), ("five_calls", five_calls)]
    cases += [(name, league_turn(lg)) for name, lg in leagues.items()]
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
        print("%-16s median %.2f us  min %.2f  max %.2f" % (k, statistics.median(v), min(v), max(v)))
    for lg in leagues.values():
        assert lg.status() == 0
    env.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(*a)
