#!/usr/bin/env python3
"""Minimized self-play (agents/Minimized/training_scripts/dqn_self_play.py) end to end on the device: a DQNAgent on EACH seat and both learn.  One launch
evaluates both networks (a two-set MinimizedQNet), one launch plays the turn from both seats' 11-way Q values (step_q: evg_step_minimized_q), the n-step
replay memory records both seats' rows {swarm, node} (SmartReplay(seats=(0, 1)) fed `actions_out`), and torch updates each network from its own seat's
transitions of the sampled batch.

    features [N, 2, ...] --MinimizedQNet (set p on seat p)--> Q [N, 2, 12, 11] --evg_step_minimized_q--> reward, done, both seats' next features and rows
             --evg_replay_record--> n-step sums --evg_replay_sample--> swarm_obs, action, next_state_swarms, reward, not_done, handles {.., seat, ..}
             --optimize_model (torch), seat by seat--> two losses

staggered=True is dqn_staggered_self_play.py: seat 1 is drawn once per episode, per env, from the second DQN or random_actions_delay -- an OpponentLeague
["q", "random_actions_delay"] and step_q(league=...) (evg_step_league_minimized_q).

Where this departs from the scripts: the replay memory records every env's seat-1 row of every turn, so with staggered=True the seat-1 memory also holds
the turns the BOT played (the script's second agent remembers only its own games).  The step marks them -- explored[:, 1] == 2 -- and a caller that wants
the script's memory masks those transitions out with it; this example trains on all of them.  One batch is drawn for both learners and split by the
seat of each transition, where the script draws one batch per agent.  A DQN loss need not decrease.

    python examples/minimized_self_play.py [envs] [turns] [batch] [staggered]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
import everglades_amd as evg
from minimized_training import GAMMA, LR, N_STEP, make_qnet


def optimize_seat(policy, target_eval, opt, batch, mine):
    """optimize_model over the transitions of one seat (`mine`: bool [B]) of a batch drawn for both"""
    swarm_obs, action, next_state, reward, not_done = batch
    predicted = policy(swarm_obs).gather(1, action.unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        nxt = target_eval(next_state)                                                      # [B, 12, 11]
        nxt = torch.where(not_done[:, None, None], nxt, torch.zeros_like(nxt))
        estimated = nxt.amax(2).mean(1) * (GAMMA ** N_STEP) + reward
    w = mine.to(predicted.dtype)
    loss = (F.smooth_l1_loss(predicted, estimated, reduction="none") * w).sum() / w.sum().clamp(min=1.0)
    opt.zero_grad()
    loss.backward()
    for p in policy.parameters():
        p.grad.data.clamp_(-1, 1)
    opt.step()
    return loss.detach()


def main(num_envs=8192, turns=300, batch=256, seed=1, epsilon=(0.3, 0.3), staggered=False):
    env = evg.EvergladesVecEnv(num_envs, seed=seed, auto_reset=True)
    policies = [make_qnet(env.device, p) for p in range(2)]
    targets = [make_qnet(env.device, p) for p in range(2)]
    for p in range(2):
        targets[p].load_state_dict(policies[p].state_dict())
    opts = [torch.optim.Adam(policies[p].parameters(), lr=LR) for p in range(2)]
    act_nets = env.minimized_qnet((policies[0], policies[1]))                              # both seats' networks, one launch
    target_evals = [env.minimized_qnet(t).expanded for t in targets]
    mem = env.smart_replay(8, n_step=N_STEP, gamma=GAMMA, shaping="custom", seats=(0, 1))
    obs = env.reset()
    league = env.opponent_league(["q", "random_actions_delay"], seat=0) if staggered else None
    shared0, swarm0 = mem.slot_features(0)
    for p in range(2):                                                                     # the first features; afterwards the step launch writes them
        s, w = env.smart_state_compact(p, obs)
        shared0[:, p].copy_(s)
        swarm0[:, p].copy_(w)
    explored = torch.zeros((num_envs, 2), dtype=torch.uint8, device=env.device)
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        q = act_nets(*mem.slot_features(t))                                                # [N, 2, 12, 11]
        env.step_q(q, epsilon, features=mem.slot_features(t + 1), actions_out=mem.slot_directions(t), explored=explored, league=league)
        mem.record(shaped=(env.reward / 10000.0).contiguous())
        if t >= N_STEP + 1:
            *b, handles = mem.sample(batch, seed=seed, return_handles=True)
            losses.append(torch.stack([optimize_seat(policies[p], target_evals[p], opts[p], b, handles[:, 2] == p) for p in range(2)]))
        if t % 100 == 99:
            for p in range(2):
                targets[p].load_state_dict(policies[p].state_dict())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses = torch.stack(losses).cpu()                                                     # [turns - N_STEP - 1, 2]
    mem.check()
    assert int(mem.size().item()) > 0
    note = ""
    if staggered:
        note = "; seat 1 held by the network in %d of %d envs now" % (int((league.assign == league.q_member).sum().item()), num_envs)
    print("%d envs x %d turns in %.3f s (%.1f M env-steps/s, networks and learning included); memory holds %d transitions; loss seat 0 / seat 1 first "
          "%.4g / %.4g last %.4g / %.4g, all finite: %s%s" % (num_envs, turns, dt, num_envs * turns / dt / 1e6, int(mem.size().item()), float(losses[0, 0]),
                                                              float(losses[0, 1]), float(losses[-1, 0]), float(losses[-1, 1]),
                                                              bool(torch.isfinite(losses).all()), note))
    env.close()
    return losses


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 8192, int(a[1]) if len(a) > 1 else 300, int(a[2]) if len(a) > 2 else 256, staggered=len(a) > 3 and a[3] in ("1", "staggered"))
