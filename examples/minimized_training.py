#!/usr/bin/env python3
"""The Minimized agent's training loop (agents/Minimized/training_scripts/dqn_training.py) end to end on the device: N envs against a scripted bot -- or,
league=True, against the cycled scripts' 15-bot league redrawn each episode --, one step launch per turn from the network's 11-way Q values (step_vs_q),
the n-step replay memory filled on the device with the agent's own rows {swarm, node} (action = node - 1) and its own reward scale (reward / 10000,
DQNAgent.py:300, through shaping="custom"), optimize_model fed by SmartReplay.sample.

    features --QNetwork(59, 11, 80)--> Q [N, 12, 11] --evg_step_vs_policy_minimized_q--> reward, done, next features, the rows played
             --evg_replay_record--> n-step sums --evg_replay_sample--> swarm_obs, action, next_state_swarms, reward, not_done --optimize_model (torch)--> loss

The acting forward and the target network's forward run as one launch each (env.minimized_qnet: the modules' parameters are read in place); the policy
forward inside optimize_model is torch's (its gradient is the loss's) or, with --device-backward, MinimizedQNet.with_grad: the fp32 evaluator's
forward with the device's backward pass behind it (include/evg_qnet_grad.h); the loss, the clamp and Adam are torch's either way.  A DQN loss need
not decrease.

    python examples/minimized_training.py [envs] [turns] [batch] [league] [--device-backward] [--device-learner]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import everglades_amd as evg

GAMMA, N_STEP, LR, FC1 = 0.99, 1, 1e-4, 80
LEAGUE = ["random_actions_delay", "random_actions", "bull_rush", "all_cycle", "base_rush_v1", "cycle_rush_turn25", "cycle_rush_turn50",
          "cycle_target_node", "cycle_target_node1", "cycle_target_node11", "cycle_target_node11P2", "random_actions_2", "same_commands_2",
          "same_commands", "swarm_agent"]


def make_qnet(device, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(59, FC1), torch.nn.ReLU(), torch.nn.Linear(FC1, 11), torch.nn.ReLU()).to(device)


def optimize_model(policy, target_eval, opt, batch, policy_forward=None):
    """policy_forward: the policy network's differentiable forward on the device (MinimizedQNet.with_grad) in place of the module's own"""
    swarm_obs, action, next_state, reward, not_done = batch
    predicted = (policy if policy_forward is None else policy_forward)(swarm_obs).gather(1, action.unsqueeze(1))
    with torch.no_grad():
        nxt = target_eval(next_state)                                                      # [B, 12, 11]
        nxt = torch.where(not_done[:, None, None], nxt, torch.zeros_like(nxt))
        estimated = nxt.amax(2).mean(1) * (GAMMA ** N_STEP) + reward
    loss = F.smooth_l1_loss(predicted, estimated.unsqueeze(1))
    opt.zero_grad()
    loss.backward()
    for p in policy.parameters():
        p.grad.data.clamp_(-1, 1)
    opt.step()
    return loss.detach()


def main(num_envs=8192, turns=300, batch=256, opponent="random_actions", seat=0, seed=1, epsilon=0.3, league=False, acting_precision="fp32",
         device_backward=False, device_learner=False):
    env = evg.EvergladesVecEnv(num_envs, seed=seed, auto_reset=True)
    policy, target = make_qnet(env.device, 0), make_qnet(env.device, 0)
    target.load_state_dict(policy.state_dict())
    opt = torch.optim.Adam(policy.parameters(), lr=LR)
    # acting and the target network on the device; "bf16": both on the bf16 matrix cores (include/evg_qnet_bf16.h); the policy forward whose
    # gradient the loss needs is torch's, or (device_backward) the fp32 evaluator's with_grad: the gradient is defined on the fp32 chain
    act_net = env.minimized_qnet(policy, precision=acting_precision)
    target_eval = env.minimized_qnet(target, precision=acting_precision).expanded
    policy_forward = env.minimized_qnet(policy).with_grad if device_backward else None
    mem = env.smart_replay(8, n_step=N_STEP, gamma=GAMMA, shaping="custom", seats=seat)
    # --device-learner: the whole optimize_model as env.minimized_learner's step (everglades_amd.DqnLearner, include/evg_learn.h): sample, the two
    # forwards, the TD head, the backward pass and Adam are launches of the library; the learner owns the gradients and Adam's state
    learner = env.minimized_learner(policy, target, mem, lr=LR, gamma=GAMMA, n_step=N_STEP, target_precision=acting_precision) if device_learner else None
    env.reset()
    if league:
        opponent = env.opponent_league(LEAGUE, seat=seat)
    env.smart_state_compact(-1, env.observe_seat(seat), *mem.slot_features(0))
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        q = act_net(*mem.slot_features(t))
        env.step_vs_q(opponent, q, epsilon, seat=seat, features=mem.slot_features(t + 1), actions_out=mem.slot_directions(t))
        mem.record(shaped=(env.reward[:, seat] / 10000.0).contiguous())
        if t >= N_STEP + 1 and learner is not None:
            losses.append(learner.step(batch, seed).clone())         # (the loss is the learner's own buffer: keep a copy for the report)
        elif t >= N_STEP + 1:
            losses.append(optimize_model(policy, target_eval, opt, mem.sample(batch, seed=seed), policy_forward))
        if t % 100 == 99:
            learner.sync_target() if learner is not None else target.load_state_dict(policy.state_dict())
            if league:
                opponent.reweight()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses = torch.stack(losses).cpu()
    mem.check()
    assert int(mem.size().item()) > 0
    print("%d envs x %d turns in %.3f s (%.1f M env-steps/s, network and learning included); memory holds %d transitions; loss first %.4g last %.4g, "
          "all finite: %s%s" % (num_envs, turns, dt, num_envs * turns / dt / 1e6, int(mem.size().item()), float(losses[0]), float(losses[-1]),
                               bool(torch.isfinite(losses).all()), "; optimize_model on the device learner" if device_learner else
                               "; policy forward with the device backward" if device_backward else ""))
    assert bool(torch.isfinite(losses).all())
    env.close()
    return losses


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x not in ("--device-backward", "--device-learner")]
    precision = "fp32"                                    # --acting-precision {fp32,bf16}
    for i, x in enumerate(a):
        if x == "--acting-precision" or x.startswith("--acting-precision="):
            precision = x.split("=", 1)[1] if "=" in x else a[i + 1]
            del a[i:i + (1 if "=" in x else 2)]
            break
    if precision not in ("fp32", "bf16"):
        sys.exit("--acting-precision must be fp32 or bf16")
    main(int(a[0]) if a else 8192, int(a[1]) if len(a) > 1 else 300, int(a[2]) if len(a) > 2 else 256, league=len(a) > 3 and a[3] in ("1", "league"),
         acting_precision=precision, device_backward="--device-backward" in sys.argv[1:],
         device_learner="--device-learner" in sys.argv[1:])
