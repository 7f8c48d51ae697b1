#!/usr/bin/env python3
"""The training loop of the reference's base agent (agents/DQN/training_scripts/dqn_training.py:130-154) end to end: examples/dqn_loop.py's acting loop
and ring of raw observations, plus DQNAgent.optimize_model (DQNAgent.py:218-282) in torch once per turn --

    state_action_values = policy_net(state_batch).gather(1, action_batch)           the 7 unravelled actions of each row
    next_state_values   = target_net(next_states).topk(7, 1)[0]                      evg_dqn_qnet through DqnQNet.rows: no autograd needed
    expected            = next_state_values * gamma + reward.unsqueeze(1).repeat(1, 7)
    loss = F.smooth_l1_loss(state_action_values, expected); loss.backward(); param.grad.data.clamp_(-1, 1); Adam; the target update

-- with the policy forward either torch's own (the default) or, with --device-backward, DqnQNet.with_grad: the same values from one launch, whose
backward() is the device's backward pass (include/evg_dqn_grad.h).  The TD head and Adam of this family are torch's in both.  With --device-learner
the whole torch block is one learner.step_on(batch) of env.dqn_learner (include/evg_dqn_learn.h): both forwards, the top-7 TD head, the backward and
Adam as a chain of launches; the ring and the index draw stay torch's.  With --device-replay (which implies --device-learner) the ring, the draw
and the gathers are the device memory env.dqn_replay (include/evg_dqn_replay.h): the step writes each observation straight into the ring, the network
reads it there, mem.record() follows the step and learner.step(mem, batch, seed) is the training step -- no torch op between step_vs and the updated
parameters.  --prioritized (with --device-replay) samples by priority instead: prioritized_optimize_model (DQNAgent.py:294-337) with the squared loss,
the importance weights and the TD head's priorities handed back, all inside learner.step(mem, batch, seed, beta).

    python examples/dqn_training.py [envs] [turns] [batch] [--device-backward | --device-learner | --device-replay [--prioritized]]
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import everglades_amd as evg

EPS_START, EPS_END, EPS_DECAY = 0.9, 0.01, 0.00001                 # dqn_training.py:50-52
GAMMA, LR, TARGET_UPDATE = 0.99, 1e-4, 10


def make_net(dev):
    return torch.nn.Sequential(torch.nn.Linear(105, 528), torch.nn.ReLU(), torch.nn.Linear(528, 132), torch.nn.ReLU()).to(dev)     # QNetwork.forward


def main(envs=4096, turns=300, batch=128, device_backward=False, opponent="random_actions", ring=8, device_learner=False, device_replay=False, prioritized=False):
    device_learner = device_learner or device_replay
    env = evg.EvergladesVecEnv(envs, seed=1, auto_reset=True)
    env.reset()
    dev = env.device
    torch.manual_seed(1)
    policy, target = make_net(dev), make_net(dev)
    target.load_state_dict(policy.state_dict())
    optimizer = torch.optim.Adam(policy.parameters(), lr=LR)
    qnet, tnet = env.dqn_qnet(policy), env.dqn_qnet(target)
    if prioritized:
        learner = env.dqn_learner(policy, target, lr=LR, gamma=GAMMA, mode="squared", clamp=None)       # prioritized_optimize_model has no clamp
    else:
        learner = env.dqn_learner(policy, target, lr=LR, gamma=GAMMA, mode="huber", clamp=1.0) if device_learner else None
    explored = torch.zeros(envs, dtype=torch.uint8, device=dev)
    if device_replay:
        return device_replay_loop(env, qnet, learner, policy, envs, turns, batch, opponent, ring, explored, prioritized)
    mem = dict(state=torch.zeros((ring, envs, 105), device=dev), action=torch.zeros((ring, envs, 7), dtype=torch.int64, device=dev),
               reward=torch.zeros((ring, envs), device=dev), next_state=torch.zeros((ring, envs, 105), device=dev))
    gen = torch.Generator(device=dev).manual_seed(2)
    obs = env.observe_seat(0)
    steps_done, losses = 0, []
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
        # ---- optimize_model on a batch drawn from the filled part of the ring
        filled = min(t + 1, ring) * envs
        idx = torch.randint(0, filled, (batch,), generator=gen, device=dev)
        state, action = mem["state"].view(-1, 105)[idx], mem["action"].view(-1, 7)[idx]
        rew, nxt = mem["reward"].view(-1)[idx], mem["next_state"].view(-1, 105)[idx]
        if learner is not None:
            loss = learner.step_on((state, action, nxt, rew, None))
        else:
            q = qnet.with_grad(state) if device_backward else policy(state)
            predicted = q.gather(1, action)
            expected = tnet.rows(nxt).topk(7, 1)[0] * GAMMA + rew.unsqueeze(1).repeat(1, 7)
            loss = F.smooth_l1_loss(predicted, expected)
            optimizer.zero_grad()
            loss.backward()
            for p in policy.parameters():
                p.grad.data.clamp_(-1, 1)
            optimizer.step()
        if t % TARGET_UPDATE == TARGET_UPDATE - 1:
            if learner is not None:
                learner.sync_target()
            else:
                target.load_state_dict(policy.state_dict())
        if t % 20 == 19:                                           # the only host reads of the loop
            losses.append(float(loss))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    finite = all(bool(torch.isfinite(p).all()) for p in policy.parameters()) and all(math.isfinite(v) for v in losses)
    print("%d envs x %d turns of the agents/DQN training loop against %s, batch %d, %s: %.1f us per turn, loss %s, all finite: %s" % (
        envs, turns, opponent, batch, "device learner (DqnFamilyLearner.step_on)" if device_learner else "device backward (DqnQNet.with_grad)" if device_backward else "torch backward", dt / turns * 1e6,
        " ".join("%.4f" % v for v in losses), finite))
    env.close()
    return finite


PER_ALPHA, PER_BETA = 0.6, 0.4                                     # PrioritizedMemory's defaults


def device_replay_loop(env, qnet, learner, policy, envs, turns, batch, opponent, ring, explored, prioritized):
    """the same loop on the device memory: `ring` turns of all envs, reward_short_games as dqn_training.py:148"""
    if prioritized:
        mem = env.dqn_prioritized_replay(capacity_turns=ring, alpha=PER_ALPHA, shaping="reward_short_games", seat=0)
    else:
        mem = env.dqn_replay(capacity_turns=ring, shaping="reward_short_games", seat=0)
    env.observe_seat(0, out=mem.slot_obs(0))
    steps_done, losses = 0, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        eps = EPS_END + (EPS_START - EPS_END) * math.exp(steps_done * -EPS_DECAY)
        steps_done += 1
        rows = env.dqn_get_action(qnet(mem.slot_obs(t)), eps, seat=0, out=mem.slot_actions(t), explored=explored)
        env.step_vs(opponent, rows, seat=0, out=mem.slot_obs(t + 1))
        mem.record()
        loss = learner.step(mem, batch, seed=t, beta=PER_BETA if prioritized else None)
        if t % TARGET_UPDATE == TARGET_UPDATE - 1:
            learner.sync_target()
        if t % 20 == 19:                                           # the only host reads of the loop
            losses.append(float(loss))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    mem.check()
    finite = all(bool(torch.isfinite(p).all()) for p in policy.parameters()) and all(math.isfinite(v) for v in losses)
    print("%d envs x %d turns of the agents/DQN training loop against %s, batch %d, %sdevice replay (DqnReplay + DqnFamilyLearner.step): %.1f us per turn, "
          "loss %s, all finite: %s" % (envs, turns, opponent, batch, "prioritized " if prioritized else "", dt / turns * 1e6, " ".join("%.4f" % v for v in losses), finite))
    env.close()
    return finite


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    a = [v for v in sys.argv[1:] if not v.startswith("--")]
    known = {"--device-backward", "--device-learner", "--device-replay", "--prioritized"}
    if set(flags) - known:
        sys.exit("unknown option %s" % " ".join(sorted(set(flags) - known)))
    if "--device-backward" in flags and len(set(flags)) > 1:
        sys.exit("--device-backward and --device-learner exclude each other")
    if "--prioritized" in flags and "--device-replay" not in flags:
        sys.exit("--prioritized needs --device-replay")
    ok = main(int(a[0]) if len(a) > 0 else 4096, int(a[1]) if len(a) > 1 else 300, int(a[2]) if len(a) > 2 else 128, "--device-backward" in flags,
              device_learner="--device-learner" in flags, device_replay="--device-replay" in flags, prioritized="--prioritized" in flags)
    sys.exit(0 if ok else 1)
