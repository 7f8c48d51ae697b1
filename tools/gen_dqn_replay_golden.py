#!/usr/bin/env python3
"""Writes tests/golden/dqn_replay.npz from the reference's own agents/DQN family: the last TURNS turns of a recorded game (tests/golden/traj_random.npz,
its final turn included) pushed through the reference's own DQNAgent.remember_game_state into its own SimpleMemory.ReplayMemory, with the turn's reward
from its own utils/reward_shaping.reward_short_games -- the loop of agents/DQN/training_scripts/dqn_training.py:129-150, imported from the reference
tree at run time, not restated.  Only numbers go into the file:

  obs [TURNS + 1, 105] int16      seat 0's observation before each turn, and after the last
  rows [TURNS, 7, 2] int32        the {unit, node 0..10} rows played (drawn here: the recorded game's own orders are not this family's)
  reward [TURNS, 2] float32, done [TURNS] uint8, turn [TURNS] int32     the step's outputs and the script's turnNum
  ref_state [TURNS, 105], ref_action [TURNS, 7], ref_next_state [TURNS, 105], ref_reward [TURNS]   float64: the memory's contents in push order
  prio [40] float32, prio_alpha, prio_beta        priorities handed to the reference's own PrioritizedMemory.update_priorities for 40 pushed records
  prio_pow [40] float32                           its prios ** prob_alpha, as sample() computes it
  prio_indices [64] int64, prio_weights [64] float32   what its sample(64, beta) drew (np.random seeded) and the importance weights it returned

    python tools/gen_dqn_replay_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("EVG_REFERENCE", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TURNS, SEED = 12, 20261026


def main():
    sys.path.insert(0, REF)
    sys.modules.setdefault("gym", types.ModuleType("gym"))         # agents/DQN/QNetwork.py imports gym and never uses it
    import agents.DQN.DQNAgent as D
    from agents.DQN.SimpleMemory import ReplayMemory
    from utils.reward_shaping import reward_short_games
    traj = np.load(os.path.join(GOLDEN, "traj_random.npz"))
    g = int(np.argmax(traj["done"].max(1) > 0))                               # a game that ends inside the recording
    length = int(traj["length"][g])
    assert traj["done"][g, length - 1] and length > TURNS
    t0 = length - TURNS
    obs = traj["obs"][g, t0:length + 1, 0].astype(np.int16)
    reward = traj["reward"][g, t0:length].astype(np.float32)
    done = traj["done"][g, t0:length].astype(np.uint8)
    turn = np.arange(t0, length, dtype=np.int32)
    rng = np.random.default_rng(SEED)
    rows = np.stack([np.stack([rng.permutation(12)[:7], rng.permutation(11)[:7]], 1) for _ in range(TURNS)]).astype(np.int32)
    agent = object.__new__(D.DQNAgent)
    agent.memory = ReplayMemory(10000)
    for t in range(TURNS):
        shaped = reward_short_games(0, reward[t].astype(np.float64), bool(done[t]), int(turn[t]))
        agent.remember_game_state(obs[t].astype(np.float64), rows[t], shaped, obs[t + 1].astype(np.float64))
    mem = agent.memory.memory
    assert len(mem) == TURNS
    out = dict(obs=obs, rows=rows, reward=reward, done=done, turn=turn,
               ref_state=np.stack([m.state.numpy() for m in mem]).astype(np.float64), ref_action=np.stack([m.action.numpy() for m in mem]).astype(np.float64),
               ref_next_state=np.stack([m.next_state.numpy() for m in mem]).astype(np.float64),
               ref_reward=np.array([float(m.reward) for m in mem], np.float64))
    assert out["ref_reward"][-1] != 0.0 and not out["ref_reward"][:-1].any()
    from agents.DQN.PrioritizedMemory import PrioritizedMemory
    alpha, beta = 0.6, 0.4
    pm = PrioritizedMemory(40, prob_alpha=alpha)
    z = np.zeros(105)
    for i in range(40):
        pm.push(z, 0, 0.0, z, False)
    prio = rng.uniform(0.05, 5.0, 40).astype(np.float32)
    pm.update_priorities(np.arange(40), prio)
    np.random.seed(SEED % (1 << 32))
    ret = pm.sample(64, beta)
    out.update(prio=prio, prio_alpha=np.float64(alpha), prio_beta=np.float64(beta), prio_pow=(pm.priorities ** pm.prob_alpha).astype(np.float32),
               prio_indices=np.asarray(ret[5], np.int64), prio_weights=np.asarray(ret[6], np.float32))
    path = os.path.join(GOLDEN, "dqn_replay.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes, %d turns of game %d (turns %d..%d), last reward %r" % (path, os.path.getsize(path), TURNS, g, t0, length - 1,
                                                                                    out["ref_reward"][-1]))


if __name__ == "__main__":
    main()
