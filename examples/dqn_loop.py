#!/usr/bin/env python3
"""The acting loop of the reference's base agent (agents/DQN/training_scripts/dqn_training.py:130-154 over DQNAgent.get_action, DQNAgent.py:119-197) with
the agent's whole turn on the device, one launch each:

    observation [N, 105] --evg_dqn_qnet (QNetwork 105-528-132, the consumer's torch parameters read in place)--> Q [N, 132]
                         --evg_dqn_get_action (the epsilon coin, then 7 random rows or filter_actions)--> orders [N, 7, 2]
                         --evg_step_vs_policy (the scripted opponent inside the step kernel)--> observation, reward, done

Epsilon is the reference's schedule, computed by the caller as DQNAgent.epsilon_greedy computes it (:144): eps_end + (eps_start - eps_end) *
exp(-eps_decay * steps_done), one step per agent call.  The transitions go to a ring of raw observations in torch, as remember_game_state stores them
(the unravelled action group * 11 + node); the learner of this family is not on the device, so a training step here would be torch's.

    python examples/dqn_loop.py [envs] [turns]
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

EPS_START, EPS_END, EPS_DECAY = 0.9, 0.01, 0.00001                 # dqn_training.py:50-52


def main(envs=4096, turns=300, opponent="random_actions", ring=8):
    env = evg.EvergladesVecEnv(envs, seed=1, auto_reset=True)
    env.reset()
    dev = env.device
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(105, 528), torch.nn.ReLU(), torch.nn.Linear(528, 132), torch.nn.ReLU()).to(dev)     # QNetwork.forward
    qnet = env.dqn_qnet(net)
    explored = torch.zeros(envs, dtype=torch.uint8, device=dev)
    # a replay of raw observations in torch: state, the 7 unravelled actions, reward, next state
    mem = dict(state=torch.zeros((ring, envs, 105), device=dev), action=torch.zeros((ring, envs, 7), dtype=torch.int64, device=dev),
               reward=torch.zeros((ring, envs), device=dev), next_state=torch.zeros((ring, envs, 105), device=dev))
    obs = env.observe_seat(0)
    steps_done, episodes, explored_total = 0, 0, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        eps = EPS_END + (EPS_START - EPS_END) * math.exp(steps_done * -EPS_DECAY)
        steps_done += 1
        slot = t % ring
        mem["state"][slot].copy_(obs)
        rows = env.dqn_get_action(qnet(obs), eps, seat=0, explored=explored)
        mem["action"][slot].copy_(rows[:, :, 0] * 11 + rows[:, :, 1])
        obs, reward, done, info = env.step_vs(opponent, rows, seat=0)
        mem["reward"][slot].copy_(reward[:, 0])
        mem["next_state"][slot].copy_(obs)
        if t % 50 == 49:                                           # the only host reads of the loop
            episodes += int(done.sum())
            explored_total += int(explored.sum())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d envs x %d turns of the agents/DQN acting loop against %s: %.1f us per turn (%.2f M env-steps/s), epsilon %.4f -> %.4f" % (
        envs, turns, opponent, dt / turns * 1e6, envs * turns / dt / 1e6, EPS_START, eps))
    env.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 300)
