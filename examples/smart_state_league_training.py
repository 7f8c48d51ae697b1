#!/usr/bin/env python3
"""The cycled training script (agents/Smart_State/training_scripts/dqn_smart_state_cycled_training_with_importance.py) on the device: N envs, each
playing the opponent that `random.choices(opposing_agents, opposing_agent_weights)` gives ITS episode (:210) from the script's 15 scripted bots (:68-160),
games and wins tallied per bot (:281-285), and the weights moved towards the bots the learner loses to on the script's cadence (updateAgentWeights,
:166-173, every IMPORTANCE_UPDATE_AFTER = 50 episodes, :319-322) -- all of it inside the one step launch per turn of examples/smart_state_training.py:

    features --QNetwork--> Q --evg_step_vs_league_q--> reward, done, next features; at an episode's end: the tally, the next member, the object swap
             --evg_replay_record / evg_replay_sample--> optimize_model (torch)          every 50 batch-episodes: evg_league_importance -> the weights

`main(evaluate_all=True)` is evaluate_all.py's shape instead: a fixed assignment `arange(N) % 15`, no redraw, and the win rate per bot at the end.

    python examples/smart_state_league_training.py [envs] [turns] [batch] [evaluate_all]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg
from smart_state_training import GAMMA, N_STEP, LR, make_qnet, q_values, optimize_model

# opposing_agents of the script, in its order (:68-160); random_actions_2 and same_commands_2 are members of their own with the ids of their twins
OPPOSING_AGENTS = ["random_actions_delay", "random_actions", "bull_rush", "all_cycle", "base_rush_v1", "cycle_rush_turn25", "cycle_rush_turn50",
                   "cycle_target_node", "cycle_target_node1", "cycle_target_node11", "cycle_target_node11P2", "random_actions_2", "same_commands_2",
                   "same_commands", "swarm_agent"]
IMPORTANCE_UPDATE_AFTER = 50        # episodes (:37); one batch-episode here is 150 turns of every env


def main(num_envs=8192, turns=600, batch=1024, seat=0, seed=1, epsilon=0.3, evaluate_all=False, fused=True, learn=True, reweight_every=IMPORTANCE_UPDATE_AFTER * 150,
         verbose=True):
    """fused=False plays the turn as smart_get_action + step_vs(league) instead of step_vs_q(league): the same games.  Returns (counts [15, 4] as a
    host array, win rate per bot)."""
    env = evg.EvergladesVecEnv(num_envs, seed=seed, auto_reset=True)
    dev = env.device
    policy, target = make_qnet(dev, 0), make_qnet(dev, 0)
    target.load_state_dict(policy.state_dict())
    opt = torch.optim.Adam(policy.parameters(), lr=LR)
    act_net, target_eval = env.smart_qnet(policy), env.smart_qnet(target).expanded
    mem = env.smart_replay(8, n_step=N_STEP, gamma=GAMMA, shaping="reward_short_games", seats=seat)
    env.reset()
    league = env.opponent_league(OPPOSING_AGENTS, seat=seat, resample=not evaluate_all)
    if evaluate_all:
        league.assign.copy_((torch.arange(num_envs, device=dev) % len(OPPOSING_AGENTS)).to(torch.uint8))
        epsilon, learn = 0.0, False
    obs_seat = env.observe_seat(seat)
    env.smart_state_compact(-1, obs_seat, *mem.slot_features(0))
    rows = torch.zeros((num_envs, 7, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(turns):
        q = act_net(*mem.slot_features(t))
        if fused:
            env.step_vs_q(league, q, epsilon, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        else:
            env.smart_get_action(q, epsilon, seat=seat, obs=obs_seat, out=rows, directions=mem.slot_directions(t))
            obs_seat = env.step_vs(league, rows, features=mem.slot_features(t + 1))[0]
        mem.record()
        if learn and t >= N_STEP + 1:
            optimize_model(policy, target, opt, mem.sample(batch, seed=seed), target_eval)
            if t % 100 == 99:
                target.load_state_dict(policy.state_dict())
        if not evaluate_all and (t + 1) % reweight_every == 0:
            league.reweight()                   # on the stream: the episodes that start from here on draw with the new weights
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    counts = league.counts.cpu().numpy()
    status = league.status()
    rates = [float(w) / g if g else float("nan") for g, w in counts[:, :2].tolist()]
    if verbose:
        print("%d envs x %d turns in %.3f s; league status %d; weights %s" % (num_envs, turns, dt, status, [round(x, 3) for x in league.weights.cpu().tolist()]))
        for name, (g, w, ti, lo), r in zip(OPPOSING_AGENTS, counts.tolist(), rates):
            print("  %-24s games %6d  wins %6d  ties %6d  losses %6d  win rate %s" % (name, g, w, ti, lo, "-" if g == 0 else "%.3f" % r))
    env.close()
    return counts, rates


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 8192, int(a[1]) if len(a) > 1 else 600, int(a[2]) if len(a) > 2 else 1024, evaluate_all=len(a) > 3 and a[3] in ("1", "evaluate_all"))
