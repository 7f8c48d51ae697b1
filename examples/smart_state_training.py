#!/usr/bin/env python3
"""The Smart_State learner's training loop (agents/Smart_State/training_scripts/dqn_smart_state_training.py:90-140) end to end on the device: N envs
against a scripted bot, one step launch per turn from the network's Q values (step_vs_q), the replay memory filled on the device (SmartReplay.record:
reward_shaping.reward_short_games + remember_game_state + end_of_episode's n-step push) and optimize_model fed by SmartReplay.sample.

    features --QNetwork--> Q --evg_step_vs_policy_smart_q--> reward, done, next features (written into the memory's next slot)
             --evg_replay_record--> shaped reward, n-step sums --evg_replay_sample--> swarm_obs, action, next_state_swarms, reward, not_done
             --optimize_model (DQNAgent.py:336-385, torch)--> loss

The network is the reference's QNetwork shape (59-60-60-5, relu) with random weights; the loss is F.smooth_l1_loss of the reference, the target the mean
over swarms of the best target-network Q of the next state, times gamma ** n_step, plus the n-step reward.  A DQN loss need not decrease.

With device_net=True the acting forward (policy on the compact features) and the target network's forward on sample()'s next_state_swarms run as
one launch each (env.smart_qnet, evg_smart_qnet: the modules' parameters read in place, so Adam's steps and load_state_dict are seen); the policy
forward inside optimize_model is torch's (its gradient is the loss's) or, with --device-backward, SmartQNet.with_grad: the fp32 evaluator's forward
with the device's backward pass behind it (include/evg_qnet_grad.h).  The loss, the clamp and Adam are torch's either way.

With --prioritized the memory is env.prioritized_replay (agents/DQN/PrioritizedMemory.py: alpha 0.6, beta 0.4): the batch is drawn by priority, the
Huber loss is weighted per sample by the importance weights and |td| + 1e-5 goes back as the new priorities (evg_replay_update_priorities).

With --device-learner the whole of optimize_model is env.smart_learner's step (everglades_amd.DqnLearner, include/evg_learn.h): sample, the two
forwards, the TD head, the backward pass and Adam are launches of the library and no torch op runs between the memory and the updated parameters.  It
implies the device networks and combines with --prioritized and --acting-precision (the target network's precision).

    python examples/smart_state_training.py [envs] [turns] [batch] [device_net] [--prioritized] [--device-backward] [--device-learner]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import everglades_amd as evg

GAMMA, N_STEP, LR = 0.999, 1, 1e-4


def make_qnet(device, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5)).to(device)


def q_values(net, shared, swarm):
    """Q [N, 12, 5] from the compact features: features[e, s] = cat(shared[e], swarm[e, s], onehot(s))."""
    return net(evg.EvergladesVecEnv.expand_smart_state(shared, swarm)).contiguous()


def optimize_model(policy, target, opt, batch, target_eval=None, weights=None, policy_forward=None):
    """DQNAgent.optimize_model (DQNAgent.py:336-385) on the sampled operands.  target_eval: the target network on the device (SmartQNet.expanded).
    weights: importance weights [B] of a prioritized batch -- the loss is then the weighted mean of the per-sample Huber terms and the call returns
    (loss, new priorities |td| + 1e-5).  policy_forward: the policy network's differentiable forward on the device (SmartQNet.with_grad) in place of
    the module's own."""
    swarm_obs, action, next_state, reward, not_done = batch
    predicted = (policy if policy_forward is None else policy_forward)(swarm_obs).gather(1, action.unsqueeze(1))
    with torch.no_grad():
        nxt = target(next_state) if target_eval is None else target_eval(next_state)                                       # [B, 12, 5]; zeros rows where not_done is False give Q of zeros: mask below
        nxt = torch.where(not_done[:, None, None], nxt, torch.zeros_like(nxt))
        future = nxt.amax(2).mean(1)
        estimated = future * (GAMMA ** N_STEP) + reward
    if weights is None:
        loss = F.smooth_l1_loss(predicted, estimated.unsqueeze(1))
    else:
        loss = (F.smooth_l1_loss(predicted, estimated.unsqueeze(1), reduction="none").squeeze(1) * weights).mean()
    opt.zero_grad()
    loss.backward()
    for p in policy.parameters():
        p.grad.data.clamp_(-1, 1)
    opt.step()
    if weights is not None:
        return loss.detach(), ((predicted.detach().squeeze(1) - estimated).abs() + 1e-5).contiguous()
    return loss.detach()


def main(num_envs=8192, turns=300, batch=1024, opponent="swarm_agent", seat=0, seed=1, epsilon=0.3, device_net=False, prioritized=False,
         acting_precision="fp32", device_backward=False, device_learner=False):
    env = evg.EvergladesVecEnv(num_envs, seed=seed, auto_reset=True)
    dev = env.device
    policy, target = make_qnet(dev, 0), make_qnet(dev, 0)
    target.load_state_dict(policy.state_dict())
    opt = torch.optim.Adam(policy.parameters(), lr=LR)
    act_net = target_eval = None
    if device_net or device_learner or acting_precision != "fp32":
        # acting and the target network on the device; "bf16": both on the bf16 matrix cores (include/evg_qnet_bf16.h).  The policy forward whose
        # gradient the loss needs is torch's, or (device_backward) the fp32 evaluator's with_grad: the gradient is defined on the fp32 chain.
        act_net = env.smart_qnet(policy, precision=acting_precision)
        target_eval = env.smart_qnet(target, precision=acting_precision).expanded
    policy_forward = env.smart_qnet(policy).with_grad if device_backward else None
    if prioritized:
        mem = env.prioritized_replay(8, alpha=0.6, n_step=N_STEP, gamma=GAMMA, shaping="reward_short_games", seats=seat)
    else:
        mem = env.smart_replay(8, n_step=N_STEP, gamma=GAMMA, shaping="reward_short_games", seats=seat)
    # the whole optimize_model on the device: the learner owns the gradients and Adam's state, `opt` stays unused
    learner = env.smart_learner(policy, target, mem, lr=LR, gamma=GAMMA, n_step=N_STEP, target_precision=acting_precision) if device_learner else None
    env.reset()
    env.smart_state_compact(-1, env.observe_seat(seat), *mem.slot_features(0))   # record 0's features
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        with torch.no_grad():
            q = q_values(policy, *mem.slot_features(t)) if act_net is None else act_net(*mem.slot_features(t))
        env.step_vs_q(opponent, q, epsilon, seat=seat, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        mem.record()
        if t >= N_STEP + 1 and learner is not None:
            losses.append(learner.step(batch, seed).clone())         # (the loss is the learner's own buffer: keep a copy for the report)
        elif t >= N_STEP + 1 and prioritized:
            out = mem.sample(batch, seed=seed, beta=0.4)
            loss, priorities = optimize_model(policy, target, opt, out[:5], target_eval, weights=out[5], policy_forward=policy_forward)
            mem.update_priorities(out[6], priorities)
            losses.append(loss)
        elif t >= N_STEP + 1:
            losses.append(optimize_model(policy, target, opt, mem.sample(batch, seed=seed), target_eval, policy_forward=policy_forward))
        if t % 100 == 99 and learner is not None:
            learner.sync_target()
        elif t % 100 == 99:
            target.load_state_dict(policy.state_dict())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses = torch.stack(losses).cpu()
    mem.check()
    print("%d envs x %d turns in %.3f s (%.1f M env-steps/s, network and learning included); memory holds %d transitions; loss first %.4g last %.4g, "
          "all finite: %s%s" % (num_envs, turns, dt, num_envs * turns / dt / 1e6, int(mem.size().item()), float(losses[0]), float(losses[-1]),
                               bool(torch.isfinite(losses).all()), "; optimize_model on the device learner" if device_learner else
                               "; policy forward with the device backward" if device_backward else ""))
    assert bool(torch.isfinite(losses).all())
    env.close()
    return losses


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x not in ("--prioritized", "--device-backward", "--device-learner")]
    precision = "fp32"                                    # --acting-precision {fp32,bf16} (implies the device network for bf16)
    for i, x in enumerate(a):
        if x == "--acting-precision" or x.startswith("--acting-precision="):
            precision = x.split("=", 1)[1] if "=" in x else a[i + 1]
            del a[i:i + (1 if "=" in x else 2)]
            break
    if precision not in ("fp32", "bf16"):
        sys.exit("--acting-precision must be fp32 or bf16")
    main(int(a[0]) if a else 8192, int(a[1]) if len(a) > 1 else 300, int(a[2]) if len(a) > 2 else 1024, device_net=len(a) > 3 and a[3] in ("1", "device_net"),
         prioritized="--prioritized" in sys.argv[1:], acting_precision=precision, device_backward="--device-backward" in sys.argv[1:],
         device_learner="--device-learner" in sys.argv[1:])
