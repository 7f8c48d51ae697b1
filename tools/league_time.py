#!/usr/bin/env python3
"""Diagnostic: what a per-env opponent costs in the learner's turn.  Stream time per turn of the Q-form step at 65 536 envs, on one box, alternating:
  (a) evg_step_vs_policy_smart_q against ONE bot (the seat_q form);
  (b) evg_step_vs_league_q with every env on that same bot (the seat_q_league form: the form's own overhead);
  (c) evg_step_vs_league_q with the cycled script's 15 members mixed within each wavefront (env e plays member e % 15: the divergence cost of agent_rows);
  (d) the 15 bots as 15 consecutive plain launches over their shares of the batch (15 handles of N / 15 envs): what (c) replaces.
Each figure is the mean over `reps` turns between two events; the cases alternate `rounds` times and every round is printed (the spread between rounds of
one case is the noise floor of the comparison)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 150
BOT = "swarm_agent"
SCRIPT = ["random_actions_delay", "random_actions", "bull_rush", "all_cycle", "base_rush_v1", "cycle_rush_turn25", "cycle_rush_turn50", "cycle_target_node",
          "cycle_target_node1", "cycle_target_node11", "cycle_target_node11P2", "random_actions_2", "same_commands_2", "same_commands", "swarm_agent"]


def make(n):
    env = evg.EvergladesVecEnv(n, seed=1, auto_reset=True)
    env.reset()
    dev = env.device
    return env, dict(q=torch.randn((n, 12, 5), device=dev), features=(torch.empty((n, 34), device=dev), torch.empty((n, 12, 13), device=dev)),
                     directions=torch.zeros((n, 7, 2), dtype=torch.int32, device=dev), explored=torch.zeros(n, dtype=torch.uint8, device=dev))


def timed(fn, reps):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def q_turn(env, b, opponent):
    return lambda: env.step_vs_q(opponent, b["q"], 0.1, features=b["features"], directions=b["directions"], explored=b["explored"])


env_a, buf_a = make(N)
env_b, buf_b = make(N)
one = env_b.opponent_league([BOT], resample=False)
env_c, buf_c = make(N)
mixed = env_c.opponent_league(SCRIPT, resample=False)
mixed.assign.copy_((torch.arange(N, device=env_c.device) % 15).to(torch.uint8))
parts = [make((N - m + 14) // 15) for m in range(15)]
turns = [q_turn(env, b, SCRIPT[m]) for m, (env, b) in enumerate(parts)]


def fifteen():
    for f in turns:
        f()


cases = [("a", "step_vs_q, one bot (%s)" % BOT, q_turn(env_a, buf_a, BOT)), ("b", "league form, every env on that bot", q_turn(env_b, buf_b, one)),
         ("c", "league form, 15 members mixed in every wavefront", q_turn(env_c, buf_c, mixed)), ("d", "15 plain launches over 15 shares of the batch", fifteen)]
res = {k: [] for k, _, _ in cases}
for r in range(ROUNDS):
    for k, _, fn in cases:
        res[k].append(timed(fn, REPS))
print("%d envs, epsilon 0.1, features + directions + explored written; us per turn (stream time), %d rounds x %d turns, alternating" % (N, ROUNDS, REPS))
for k, what, _ in cases:
    v = res[k]
    print("(%s) %-52s median %7.2f   rounds %s" % (k, what, sorted(v)[len(v) // 2], " ".join("%.2f" % x for x in v)))
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
print("(b) / (a) = %.3f   (c) / (a) = %.3f   (c) / (d) = %.3f" % (med["b"] / med["a"], med["c"] / med["a"], med["c"] / med["d"]))
for env in [env_a, env_b, env_c] + [p[0] for p in parts]:
    env.close()
