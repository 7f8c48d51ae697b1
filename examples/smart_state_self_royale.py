#!/usr/bin/env python3
"""Smart_State self-royale (agents/Smart_State/training_scripts/dqn_smart_state_self_royale.py) end to end on the device: each seat has a TEAM of 4
DQNAgents (:28, :51-70), random.choice(team) picks the member that plays an episode (:106-107), and only the members that played remember the game and
learn from it (:148-201) -- per env here: a SmartQPopulation keeps member[e, p], evaluates every env through its own member's 59-60-60-5 network in one
grouped forward, and redraws the members of the envs whose episode ended.

    features [N, 2, ...] --SmartQPopulation (member[e, p] of team p)--> Q [N, 2, 12, 5] --evg_step_smart_q (per-member epsilon [N, 2])--> reward, done, ...
             --evg_smart_population_assign--> per-member tally, the next episode's members
             --evg_replay_record / _sample--> a batch; each transition belongs to the (seat, member) that played it: `played`, a ring parallel to the
             replay memory's slots --optimize_model (torch), one masked loss per (seat, member); targets from the member's own target network in one
             grouped launch per seat (SmartQPopulation.expanded)

Where this departs from the script: one batch is drawn for all eight learners and split by (seat, member), where the script draws one batch per agent
that played; a member with no transition in the batch takes a zero loss and no step.  `played` holds the members of every turn (a copy of pop.member ahead
of the step: end_of_turn's history= names the members of the envs whose episode ended, here kept as last_game).  A DQN loss need not decrease.

    python examples/smart_state_self_royale.py [envs] [turns] [batch] [--device-learner] [--acting-precision {fp32,bf16}]

--device-learner: the learning block is two PopulationLearners (everglades_amd.PopulationLearner, one per seat's team): one step_on per seat trains
every member on the rows it played, with the other seat's rows passed as id 255 -- no torch forward, backward or optimizer.  There a member without
a row in the batch really takes no step (the torch loop's zero-gradient opt.step() still moves its parameters through Adam's moments).

--acting-precision bf16: the acting populations evaluate on the bf16 matrix cores (QPopulationBf16 / SmartQPopulationBf16, include/evg_pop_bf16.h); with
--device-learner the learners' targets do too, as one grouped forward each (target_precision="bf16_grouped").  The policy forward that is trained stays fp32.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
import everglades_amd as evg
from smart_state_training import GAMMA, LR, N_STEP, make_qnet

NUM_AGENTS_PER_TEAM = 4


def main(num_envs=8192, turns=300, batch=256, seed=1, team_size=NUM_AGENTS_PER_TEAM, device_learner=False, acting_precision="fp32"):
    env = evg.EvergladesVecEnv(num_envs, seed=seed, auto_reset=True)
    dev, K = env.device, team_size
    policies = [[make_qnet(dev, 10 * p + m) for m in range(K)] for p in range(2)]
    targets = [[make_qnet(dev, 10 * p + m) for m in range(K)] for p in range(2)]
    # each member explores at its own rate: epsilon [N, 2] is gathered from this table by the members that play
    eps_table = torch.stack([torch.linspace(0.1, 0.4, K), torch.linspace(0.4, 0.1, K)]).to(dev)
    mem = env.smart_replay(8, n_step=N_STEP, gamma=GAMMA, shaping="custom", seats=(0, 1))
    obs = env.reset()
    pop = env.smart_q_population(policies[0], policies[1], precision=acting_precision)          # the acting networks, drawn per env and episode
    if device_learner:                                                                     # one learner per seat's team; it owns the target forward
        learners = [env.smart_population_learner(policies[p], targets[p], lr=LR, gamma=GAMMA, n_step=N_STEP, mode="max_mean", clamp=1.0,
                                                 target_precision="bf16_grouped" if acting_precision == "bf16" else "fp32")
                    for p in range(2)]
        nobody = torch.full((batch,), 255, dtype=torch.uint8, device=dev)
    else:
        opts = [[torch.optim.Adam(policies[p][m].parameters(), lr=LR) for m in range(K)] for p in range(2)]
        tpop = env.smart_q_population(targets[0], targets[1], max_rows=12 * batch)                 # the target networks, evaluated by recorded member
    shared0, swarm0 = mem.slot_features(0)
    for p in range(2):                                                                     # the first features; afterwards the step launch writes them
        s, w = env.smart_state_compact(p, obs)
        shared0[:, p].copy_(s)
        swarm0[:, p].copy_(w)
    q = torch.zeros((num_envs, 2, 12, 5), device=dev)
    played = torch.zeros((mem.slots, num_envs, 2), dtype=torch.uint8, device=dev)          # who played the transition of (slot, env, seat)
    last_game = torch.zeros((num_envs, 2), dtype=torch.uint8, device=dev)                  # who played each env's last finished episode (history=)
    seats = torch.arange(2, device=dev)
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        pop(*mem.slot_features(t), out=q)
        members = pop.member.long()
        played[mem.slot(t)].copy_(pop.member)
        eps = eps_table[seats[None, :], members].contiguous()                              # [N, 2]
        env.step_q(q, eps, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        pop.end_of_turn(history=last_game)                                                 # tally, and new members where an episode ended
        mem.record(shaped=(env.reward / 10000.0).contiguous())
        if t >= N_STEP + 1:
            swarm_obs, action, next_state, reward, not_done, handles = mem.sample(batch, seed=seed, return_handles=True)
            h = handles.long()
            who = played[h[:, 0], h[:, 1], h[:, 2]]                                        # [B] the member that played each transition
            row = []
            if device_learner:
                for p in range(2):                                                         # seat p's rows keep their member, the others are nobody's
                    row.append(learners[p].step_on((swarm_obs, action, next_state, reward, not_done), torch.where(h[:, 2] == p, who, nobody)).clone())
                losses.append(torch.stack(row))
            else:
                for p in range(2):
                    with torch.no_grad():
                        nxt = tpop.expanded(next_state, who, p)                                # [B, 12, 5]: each transition through its member's target
                        nxt = torch.where(not_done[:, None, None], nxt, torch.zeros_like(nxt))
                        estimated = nxt.amax(2).mean(1) * (GAMMA ** N_STEP) + reward
                    for m in range(K):
                        mine = ((h[:, 2] == p) & (who == m)).to(estimated.dtype)
                        predicted = policies[p][m](swarm_obs).gather(1, action.unsqueeze(1)).squeeze(1)
                        loss = (F.smooth_l1_loss(predicted, estimated, reduction="none") * mine).sum() / mine.sum().clamp(min=1.0)
                        opts[p][m].zero_grad()
                        loss.backward()
                        for w in policies[p][m].parameters():
                            w.grad.data.clamp_(-1, 1)
                        opts[p][m].step()
                        row.append(loss.detach())
                losses.append(torch.stack(row).view(2, K))
        if t % 100 == 99:
            for p in range(2):
                for m in range(K):
                    targets[p][m].load_state_dict(policies[p][m].state_dict())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses = torch.stack(losses).cpu()                                                     # [turns - N_STEP - 1, 2, K]
    mem.check()
    pop.check()
    if not device_learner:
        tpop.check()
    counts = pop.counts[:, :K].cpu()
    print("%s%d envs x %d turns in %.3f s (%.1f M env-steps/s, networks and learning included); games per member seat 0 %s seat 1 %s, wins %s / %s; "
          "loss of member 0 first %.4g / %.4g last %.4g / %.4g, all finite: %s" % (
              "device learner: " if device_learner else "", num_envs, turns, dt, num_envs * turns / dt / 1e6, counts[0, :, 0].tolist(), counts[1, :, 0].tolist(), counts[0, :, 1].tolist(),
              counts[1, :, 1].tolist(), float(losses[0, 0, 0]), float(losses[0, 1, 0]), float(losses[-1, 0, 0]), float(losses[-1, 1, 0]),
              bool(torch.isfinite(losses).all())))
    env.close()
    return losses


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--device-learner"]
    precision = "fp32"                                    # --acting-precision {fp32,bf16}
    for i, x in enumerate(a):
        if x == "--acting-precision" or x.startswith("--acting-precision="):
            precision = x.split("=", 1)[1] if "=" in x else a[i + 1]
            del a[i:i + (1 if "=" in x else 2)]
            break
    if precision not in ("fp32", "bf16"):
        sys.exit("--acting-precision must be fp32 or bf16")
    main(int(a[0]) if a else 8192, int(a[1]) if len(a) > 1 else 300, int(a[2]) if len(a) > 2 else 256, device_learner="--device-learner" in sys.argv[1:],
         acting_precision=precision)
