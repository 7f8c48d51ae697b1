#!/usr/bin/env python3
"""Writes tests/golden/smart_replay.npz: the Smart_State learner's n-step replay memory as the reference builds it, for the replay tests
(tests/test_replay_model.py against the host model, tests/test_gpu_replay.py against the device).

The reference is imported, not restated: the game through oracle/gen_golden.py's Runner (read-only helpers), the learner is the reference's
DQNAgent (agents/Smart_State/DQNAgent.py, created without __init__: a seeded random QNetwork, epsilon 0.3), its memory the reference's
Multi_Step.NStepModule fed by DQNAgent.remember_game_state and addGameToReplayMemory, its rewards utils/reward_shaping.py -- the loop of
dqn_smart_state_training.py:114-140.  The opponent is the reference's SwarmAgent.

Per variant <v>, per turn of the recorded episodes (one env playing them back to back): the compact features of the observation the learner acted on
(v_shared [T, 34], v_swarm [T, 12, 13] float32 -- create_swarm_obs's float64 values rounded once), v_dirs [T, 7, 2] (get_action's directions),
v_reward [T, 2] float64 (the env's reward), v_done [T], v_turn [T], v_episode [T]; and the reference's replay memory deduplicated against the records:
v_tr int32 [M, 5] {record, swarm, action, next record or -1, doesNotHitDone}, v_tr_reward float64 [M] -- checked entry by entry against the reference's
Transition tuples (swarm_obs / next_state_swarms bit for bit) before anything is written.  v_params: n, gamma, shaping, transition K, episode base.

    python tools/gen_replay_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
"""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smart_replay.npz")
SHAPES = ["normalized_score", "basic_reward", "penalize_long_games", "reward_short_games", "transition"]

# name, n, gamma, shaping (code, from, to, K), episode base, episodes, seed, pre-edit of episode 0
VARIANTS = [
    ("a", 1, 0.999, (4, 0, 3, 200), 198, 3, 71, False),      # transition(normalized_score, reward_short_games, 200, i_episode), i_episode 199, 200, 201
    ("b", 3, 0.9, (3, 0, 0, 1), 0, 2, 72, False),            # reward_short_games, n = 3
    ("c", 3, 0.95, (2, 0, 0, 1), 0, 2, 73, True),            # penalize_long_games; episode 0 ends at once by annihilation (shorter than n)
]


def main():
    R = gg.Runner()
    sys.path.insert(0, gg.REF)
    import torch
    import agents.Smart_State.DQNAgent as D
    import agents.Smart_State.Multi_Step as MS
    import agents.Smart_State.QNetwork as QN
    import utils.reward_shaping as RS
    fns = [RS.normalized_score, RS.basic_reward, RS.penalize_long_games, RS.reward_short_games]
    out = {}
    for name, n, gamma, (code, f1, f2, K), ep_base, episodes, seed, edit in VARIANTS:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        agent = D.DQNAgent.__new__(D.DQNAgent)
        agent.num_nodes, agent.epsilon = gg.NN, 0.3
        agent.policy_net = QN.QNetwork(D.INPUT_SIZE, D.OUTPUT_SIZE, D.FC1_SIZE, D.FC2_SIZE)
        agent.NStepModule = MS.NStepModule(n, gamma, 10 ** 7)
        bot = gg.load_agent(R.proxy, "swarm_agent.py", "SwarmAgent", 1)
        ns = types.SimpleNamespace(num_nodes=gg.NN)
        rows = dict(shared=[], swarm=[], dirs=[], reward=[], done=[], turn=[], episode=[])
        feats64 = []                                   # [T][12][59] float64: what the reference's memory holds
        for ep in range(episodes):
            obs = R.reset(seed, 0, ep)
            if edit and ep == 0:
                gg.edit_annihilation(R.env.game)
                obs = R.env._build_observations()
            done, turn_num, i_episode = 0, 0, ep_base + 1 + ep
            while not done:
                a0, directions = agent.get_action(obs[0])
                a1 = bot.get_action(obs[1])
                prev = obs[0]
                al = D.DQNAgent.get_allies_on_node_data(ns, prev)
                f = np.stack([D.DQNAgent.create_swarm_obs(ns, s, prev, al) for s in range(gg.NG)])
                obs, reward, done, info = R.env.step({0: a0, 1: np.array(a1, dtype=np.float64)})
                if code == 4:
                    shaped = RS.transition(fns[f1], fns[f2], K, i_episode, 0, reward, done, turn_num)
                else:
                    shaped = fns[code](0, reward, done, turn_num)
                agent.remember_game_state(prev, obs[0], directions, shaped)
                feats64.append(f)
                rows["shared"].append(f[0, :34].astype(np.float32))
                rows["swarm"].append(f[:, 34:47].astype(np.float32))
                rows["dirs"].append(np.asarray(directions).astype(np.int32))
                rows["reward"].append([float(reward[0]), float(reward[1])])
                rows["done"].append(int(bool(done)))
                rows["turn"].append(turn_num)
                rows["episode"].append(ep)
                turn_num += 1
            agent.NStepModule.addGameToReplayMemory()
        mem = agent.NStepModule.replay_memory.memory
        # deduplicate: the reference pushes, per episode, per step, per swarm 0..11 whose first order row has direction != 0
        tr, trr, i = [], [], 0
        T = len(rows["done"])
        start = 0
        while start < T:
            end = start
            while not rows["done"][end]:
                end += 1
            for s in range(start, end + 1):
                d = rows["dirs"][s]
                for sw in range(gg.NG):
                    hit = [r for r in range(7) if d[r, 0] == sw]
                    if not hit or d[hit[0], 1] - 1 == -1:
                        continue
                    nxt = s + n if s + n <= end else -1
                    m = mem[i]
                    i += 1
                    assert np.array_equal(m.swarm_obs, feats64[s][sw]), (name, s, sw)
                    assert m.swarm_action == int(d[hit[0], 1]) - 1
                    assert np.array_equal(m.next_state_swarms, feats64[nxt] if nxt >= 0 else np.zeros((12, 59)))
                    assert bool(m.doesNotHitDone) == (nxt >= 0)
                    tr.append([s, sw, m.swarm_action, nxt, int(m.doesNotHitDone)])
                    trr.append(float(m.reward))
            start = end + 1
        assert i == len(mem), (i, len(mem))
        for k in rows:
            out["%s_%s" % (name, k)] = np.asarray(rows[k], dtype={"shared": np.float32, "swarm": np.float32, "dirs": np.int32, "reward": np.float64,
                                                                  "done": np.uint8, "turn": np.int32, "episode": np.int32}[k])
        out[name + "_tr"] = np.asarray(tr, np.int32)
        out[name + "_tr_reward"] = np.asarray(trr, np.float64)
        out[name + "_params"] = np.array([n, gamma, code, f1, f2, K, ep_base], np.float64)
        print("variant %s: %d turns, episode ends at %s, %d transitions" % (name, T, np.flatnonzero(out[name + "_done"]).tolist(), len(tr)), flush=True)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
