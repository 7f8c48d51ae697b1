#!/usr/bin/env python3
"""Self-play with a Smart_State DQNAgent on each seat (agents/Smart_State/training_scripts/dqn_smart_state_self_play.py:120-128: get_action for both
players, then env.step), everything but the two networks on the device.  Seat 0 trains (epsilon 0.1 here), seat 1 is a frozen copy (epsilon 0.0,
DQNAgent.py:15-17,73-75).

fused=True, one launch per turn from both seats' Q values to both players' next features (evg_step_smart_q):

    features [N, 2, ...] --(network p on player p's features)--> Q [N, 2, 12, 5] --evg_step_smart_q--> observation, reward, done AND the next features

fused=False, the same turn as separate calls: evg_smart_get_action for seat 0 and for seat 1, evg_step with both seats' rows (stacked into [N, 2, 7, 2]),
evg_smart_state_compact for player 0 and for player 1.

The networks are stand-ins with random weights (examples/smart_state_loop.py's make_network, two seeds) evaluated on the compact features; with
device_net=True by env.smart_qnet (evg_smart_qnet): fused, both seats' networks in one launch on [N, 2, ...]; otherwise one launch per seat.

    python examples/smart_state_self_play.py [envs] [turns] [fused] [device_net]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import everglades_amd as evg
from smart_state_loop import make_network


def main(num_envs=8192, turns=200, epsilon=(0.1, 0.0), seed=1, fused=False, device_net=False):
    env = evg.EvergladesVecEnv(num_envs, seed=seed, auto_reset=True)
    nets = (make_network(env.device, seed=0), make_network(env.device, seed=1))
    dev = env.device
    if device_net:
        pair = env.smart_qnet((nets[0].params, nets[1].params), final_relu=False)     # both seats, one launch
        qbuf = torch.empty((num_envs, 2, 12, 5), device=dev)
        nets = tuple((lambda q: (lambda shared, swarm: q(shared, swarm)))(env.smart_qnet(n.params, final_relu=False)) for n in nets)
    obs = env.reset()                                                 # [N, 2, 105]
    if fused:
        shared = torch.empty((num_envs, 2, 34), device=dev)
        swarm = torch.empty((num_envs, 2, 12, 13), device=dev)
        for p in range(2):                                            # the first features of the loop; afterwards the step launch refills them
            s, w = env.smart_state_compact(p, obs)
            shared[:, p].copy_(s)
            swarm[:, p].copy_(w)
        # (each network reads a contiguous copy of its player's rows: the same operands, hence the same Q values, as the five-call path's buffers)
        feats = [(shared[:, p], swarm[:, p]) for p in range(2)]
        directions = torch.zeros((num_envs, 2, 7, 2), dtype=torch.int32, device=dev)
        explored = torch.zeros((num_envs, 2), dtype=torch.uint8, device=dev)
    else:
        feats = [env.smart_state_compact(p, obs) for p in range(2)]
        rows = [torch.zeros((num_envs, 7, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        directions = [torch.zeros((num_envs, 7, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        explored = [torch.zeros(num_envs, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(turns):
        if fused:            # one launch: both seats' orders are decoded from q inside the step (evg_step_smart_q)
            if device_net:
                q = pair(shared, swarm, out=qbuf)
            else:
                q = torch.stack([nets[p](feats[p][0].contiguous(), feats[p][1].contiguous()) for p in range(2)], dim=1)     # [N, 2, 12, 5]
            obs, reward, done, info = env.step_q(q, epsilon, features=(shared, swarm), directions=directions, explored=explored)
        else:
            for p in range(2):
                env.smart_get_action(nets[p](*feats[p]), epsilon[p], seat=p, obs=obs, out=rows[p], directions=directions[p], explored=explored[p])
            obs, reward, done, info = env.step(torch.stack(rows, dim=1))
            for p in range(2):
                env.smart_state_compact(p, obs, *feats[p])
        # (the training seat would push (features, directions, reward, done) of seat 0 into its replay memory here)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = env.episode_stats()
    print("%s: %d envs x %d turns in %.3f s = %.1f M env-steps/s (networks included); episodes finished %d, wins seat0 / seat1 / ties %s"
          % ("fused" if fused else "five calls", num_envs, turns, dt, num_envs * turns / dt / 1e6, int(st["totals"][0]), st["totals"][1:].tolist()))
    env.close()
    return st


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 8192, int(a[1]) if len(a) > 1 else 200, fused=len(a) > 2 and a[2] in ("1", "fused"),
         device_net=len(a) > 3 and a[3] in ("1", "device_net"))
