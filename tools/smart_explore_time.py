#!/usr/bin/env python3
"""Diagnostic: stream time of evg_smart_actions against evg_smart_get_action (DQNAgent.get_action: coin + get_random_actions) at 65 536 envs; then the
Smart_State learner's turn from Q to the next features, per turn, as two calls (evg_smart_get_action + evg_step_vs_policy_smart) and as the one fused launch
(evg_step_vs_policy_smart_q), timed the same way; then the self-play turn (a DQNAgent on each seat) from both seats' Q to both players' next features, as
five calls (evg_smart_get_action x 2, evg_step, evg_smart_state_compact x 2; plus the copy that stacks the two seats' rows into evg_step's [N, 2, 7, 2]
tensor) and as the one fused launch (evg_step_smart_q)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
env = evg.EvergladesVecEnv(N, seed=1, auto_reset=True)
env.reset()
env.rollout_random(60, turns_per_launch=60)
q = torch.randn((N, 12, 5), device=env.device)
sobs = env.observe_seat(0)


def timed(fn, reps=200):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


print("evg_smart_actions                 %.2f us per call" % timed(lambda: env.smart_actions(q, obs=sobs)))
for eps in (0.0, 0.1, 1.0):
    print("evg_smart_get_action eps = %.1f    %.2f us per call" % (eps, timed(lambda: env.smart_get_action(q, eps, seat=0, obs=sobs))))
sh = torch.empty((N, 34), device=env.device)
sw = torch.empty((N, 12, 13), device=env.device)
rows = env.random_actions_seat(0).clone()
print("evg_step_vs_policy                %.2f us per call" % timed(lambda: env.step_vs("random", rows, seat=0)))
print("evg_step_vs_policy_smart          %.2f us per call (the same turn + the Smart_State features of the new observation)" % timed(lambda: env.step_vs("random", rows, seat=0, features=(sh, sw))))
print("evg_smart_state_compact           %.2f us per call (the separate feature kernel it replaces)" % timed(lambda: env.smart_state_compact(-1, sobs, sh, sw)))
dirs = torch.zeros((N, 7, 2), dtype=torch.int32, device=env.device)
ex = torch.zeros(N, dtype=torch.uint8, device=env.device)
for eps in (0.0, 0.1):
    def two_calls():
        a = env.smart_get_action(q, eps, seat=0, obs=sobs, directions=dirs, explored=ex)
        env.step_vs("swarm", a, seat=0, features=(sh, sw))
    def fused():
        env.step_vs_q("swarm", q, eps, seat=0, features=(sh, sw), directions=dirs, explored=ex)
    print("TRAINING turn eps = %.1f, two calls  %.2f us per turn (evg_smart_get_action + evg_step_vs_policy_smart)" % (eps, timed(two_calls)))
    print("TRAINING turn eps = %.1f, fused      %.2f us per turn (evg_step_vs_policy_smart_q)" % (eps, timed(fused)))
q2 = torch.randn((N, 2, 12, 5), device=env.device)
q_seat = [q2[:, p].contiguous() for p in range(2)]                 # (two networks: two [N, 12, 5] outputs)
rows2 = [torch.zeros((N, 7, 2), dtype=torch.int32, device=env.device) for _ in range(2)]
dirs2 = [torch.zeros((N, 7, 2), dtype=torch.int32, device=env.device) for _ in range(2)]
ex2 = [torch.zeros(N, dtype=torch.uint8, device=env.device) for _ in range(2)]
acts = torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=env.device)
feat2 = [(torch.empty((N, 34), device=env.device), torch.empty((N, 12, 13), device=env.device)) for _ in range(2)]
feat_f = (torch.empty((N, 2, 34), device=env.device), torch.empty((N, 2, 12, 13), device=env.device))
dirs_f = torch.zeros((N, 2, 7, 2), dtype=torch.int32, device=env.device)
ex_f = torch.zeros((N, 2), dtype=torch.uint8, device=env.device)
env.observe()
for eps in ((0.0, 0.0), (0.1, 0.0)):
    def five_calls():
        for p in range(2):
            env.smart_get_action(q_seat[p], eps[p], seat=p, obs=env.obs, out=rows2[p], directions=dirs2[p], explored=ex2[p])
        torch.stack(rows2, dim=1, out=acts)
        env.step(acts)
        for p in range(2):
            env.smart_state_compact(p, env.obs, *feat2[p])
    def fused2():
        env.step_q(q2, eps, features=feat_f, directions=dirs_f, explored=ex_f)
    print("SELF-PLAY turn eps = (%.1f, %.1f), five calls  %.2f us per turn (evg_smart_get_action x 2 + stack + evg_step + evg_smart_state_compact x 2)"
          % (eps + (timed(five_calls),)))
    print("SELF-PLAY turn eps = (%.1f, %.1f), fused       %.2f us per turn (evg_step_smart_q)" % (eps + (timed(fused2),)))
env.close()
