#!/usr/bin/env python3
"""Fixture generator for tests/test_oracle_vs_live_reference.py (TEST INFRASTRUCTURE; needs the reference, like oracle/gen_golden.py).

The imported reference plays RANDOM configurations (oracle/custom_configs.py: random directed graphs, control points, defenses, resources, bases and
unit files inside the domain include/evg.h states) and random inputs of the Smart_State agent; what it returned is written as numbers under tests/golden/,
so the tests replay the oracle against it without the reference:

    tests/golden/fuzz_configs.npz   10 configurations x ('random', 'wild') order streams: the map / unit JSON text and every turn's observations, scores,
                                    status, rewards, float64 health, packed state, list order, fog mask and knowledge levels (oracle/gen_golden.py's Runner)
    tests/golden/fuzz_agents.npz    12 configurations x a random pairing of the reference's own agent classes, two episodes with the objects kept alive
    tests/golden/fuzz_smart.npz     1 500 random observations / Q tensors / epsilons through DQNAgent.get_action and DQNAgent.create_swarm_obs

    python oracle/gen_fuzz_golden.py          # about a minute; EVG_REFERENCE names the reference's directory (as for oracle/gen_golden.py)
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402
from custom_configs import random_config  # noqa: E402

OUT = gg.OUT
CONFIGS_SEED, CONFIGS_COUNT = 20261008, 10
AGENTS_SEED, AGENTS_COUNT = 20261011, 12
SMART_SEED, SMART_CALLS = 5, 1500

AGENT_CLASSES = dict(swarm=("swarm_agent.py", "SwarmAgent"), cyc25=("cycle_rush_turn25.py", "Cycle_BRush_Turn25"),
                     cyc50=("cycle_rush_turn50.py", "Cycle_BRush_Turn50"), dfs=("dfs_attack.py", "dfs_attack"),
                     ctn=("cycle_target_node.py", "Cycle_Target_Node"), ctn1=("cycle_target_node1.py", "cycle_targetedNode1"),
                     ctn11=("cycle_target_node11.py", "cycle_targetedNode11"), ctnp2=("cycle_target_node11P2.py", "cycle_targetedNode11P2"),
                     bull=("bull_rush.py", "bull_rush"), brv1=("base_rush_v1.py", "base_rushV1"), allc=("all_cycle.py", "all_cycle"),
                     rnd=("random_actions.py", "random_actions"), delay=("random_actions_delay.py", "random_actions_delay"),
                     same=("same_commands.py", "same_commands"))


def _config_files(tmp, seed0, c):
    """configuration c of a fuzz run: (rng positioned after the draw, map text, unit text, map path, unit path)"""
    rng = np.random.default_rng([seed0, c])
    mobj, uobj = random_config(rng)
    mtxt, utxt = json.dumps(mobj), json.dumps(uobj)
    mp, up = os.path.join(tmp, "m%d.json" % c), os.path.join(tmp, "u%d.json" % c)
    open(mp, "w").write(mtxt)
    open(up, "w").write(utxt)
    return rng, mtxt, utxt, mp, up


def gen_configs(R, tmp):
    saved = dict(R.cfg)
    games, metas, mtexts, utexts = [], [], [], []
    for c in range(CONFIGS_COUNT):
        _, mtxt, utxt, mp, up = _config_files(tmp, CONFIGS_SEED, c)
        R.cfg = dict(saved, map_file=mp, unit_file=up)
        for pol in ("random", "wild"):
            seed, env_id = 5000 + c, 3 * c + (pol == "wild")
            games.append(R.play(pol, seed, env_id, 0, max_turns=60 if pol == "wild" else 150, obs_bound=511))
            metas.append(dict(policy=pol, seed=seed, env_id=env_id, episode=0))
            mtexts.append(mtxt), utexts.append(utxt)
    R.cfg = saved
    d = gg.pack(games, metas)
    d.update(map_json=np.array(mtexts), unit_json=np.array(utexts))
    np.savez_compressed(os.path.join(OUT, "fuzz_configs.npz"), **d)
    print("fuzz_configs: %d games, %d turns" % (len(games), int(d["length"].sum())), flush=True)


def gen_agents(R, tmp):
    saved = dict(R.cfg)
    names = sorted(AGENT_CLASSES)
    keys = ("obs", "actions", "length", "scores", "status")
    rec = {k: [] for k in keys + ("policy", "pairing", "seed", "env_id", "map_json", "unit_json")}
    for c in range(AGENTS_COUNT):
        rng, mtxt, utxt, mp, up = _config_files(tmp, AGENTS_SEED, c)
        R.cfg = dict(saved, map_file=mp, unit_file=up)
        a, b = (names[int(i)] for i in rng.integers(0, len(names), 2))
        seed, env_id = 6000 + c, 2 * c + 1
        d = gg.play_agents(R, (AGENT_CLASSES[a], AGENT_CLASSES[b]), seed, env_id, 2)     # the reference's own agent classes, alive across both episodes
        for k in keys:
            rec[k].append(d[k])
        rec["policy"].append([gg.AGENT_POLICY[AGENT_CLASSES[a][1]], gg.AGENT_POLICY[AGENT_CLASSES[b][1]]])
        rec["pairing"].append("%s-%s" % (a, b))
        rec["seed"].append(seed), rec["env_id"].append(env_id), rec["map_json"].append(mtxt), rec["unit_json"].append(utxt)
    R.cfg = saved
    out = {k: np.stack(rec[k]) for k in keys}
    out.update(policy=np.array(rec["policy"], np.int32), pairing=np.array(rec["pairing"]), seed=np.array(rec["seed"], np.uint64),
               env_id=np.array(rec["env_id"], np.uint32), map_json=np.array(rec["map_json"]), unit_json=np.array(rec["unit_json"]))
    np.savez_compressed(os.path.join(OUT, "fuzz_agents.npz"), **out)
    print("fuzz_agents: %d configurations, %d turns" % (AGENTS_COUNT, int(out["length"].sum())), flush=True)


def gen_smart():
    """DQNAgent.get_action / create_swarm_obs of the reference on random inputs; the three draws of get_action served from the keyed stream
    (rng_spec.explore_draws) by module proxies, as in oracle/gen_golden.py's smart_explore fixture."""
    import rng_spec
    import torch
    sys.path.insert(0, gg.REF)
    import agents.Smart_State.DQNAgent as D
    rng = np.random.default_rng(SMART_SEED)
    M = SMART_CALLS
    # random but well-formed observations of one player: turn, 11 x (flags, control, opposing units), 12 x (node, type, avg health, in transit, alive)
    obs = np.zeros((M, 105))
    obs[:, 0] = rng.integers(0, 151, M)
    for n in range(11):
        obs[:, 1 + 4 * n] = rng.integers(0, 2, M); obs[:, 2 + 4 * n] = rng.integers(0, 2, M)
        obs[:, 3 + 4 * n] = rng.integers(-500, 501, M); obs[:, 4 + 4 * n] = rng.integers(0, 101, M)
    for k in range(12):
        obs[:, 45 + 5 * k] = rng.integers(1, 12, M); obs[:, 46 + 5 * k] = rng.integers(0, 3, M); obs[:, 47 + 5 * k] = rng.integers(0, 101, M)
        obs[:, 48 + 5 * k] = rng.integers(0, 2, M); obs[:, 49 + 5 * k] = rng.integers(0, 13, M)
    q = rng.standard_normal((M, 12, 5)).astype(np.float32)
    q[M // 2:] = np.round(q[M // 2:] * 2) / 2                                # ties between swarms and between directions
    eps = rng.choice(np.array([0.0, 0.05, 0.3, 0.7, 1.0], np.float32), M)
    seed, player = 99, int(rng.integers(0, 2))
    cur = dict(m=0)

    class _Std(object):
        def random(self):
            L = sys._getframe(1).f_locals
            return rng_spec.explore_draws(seed, cur["m"], cur["m"] % 5, int(L["obs"][0]), player)[0] / 4294967296.0

    class _NpRandom(object):
        def choice(self, a, size, replace=True):
            L = sys._getframe(1).f_locals
            coin, swarms, dirs = rng_spec.explore_draws(seed, cur["m"], cur["m"] % 5, int(L["obs"][0]), player)
            return np.array(swarms if a == 12 else dirs)

    class _Np(object):
        random = _NpRandom()

        def __getattr__(self, k):
            return getattr(np, k)

    D.random, D.np = _Std(), _Np()
    agent = D.DQNAgent.__new__(D.DQNAgent)
    agent.num_nodes = 11
    ns = types.SimpleNamespace(num_nodes=11)
    acts, dirs, feats = np.zeros((M, 7, 2), np.int32), np.zeros((M, 7, 2), np.int32), np.zeros((M, 12, 59))
    for m in range(M):
        cur["m"] = m
        agent.epsilon = float(eps[m])
        agent.policy_net = lambda so, m=m: torch.from_numpy(q[m, int(np.argmax(so[47:59]))].copy())
        a, d = agent.get_action(obs[m])
        acts[m], dirs[m] = a.astype(np.int32), d.astype(np.int32)
        al = D.DQNAgent.get_allies_on_node_data(ns, obs[m])
        for sw in range(12):
            feats[m, sw] = D.DQNAgent.create_swarm_obs(ns, sw, obs[m], al)
    assert np.all(obs == np.round(obs)) and np.abs(obs).max() <= 500
    np.savez_compressed(os.path.join(OUT, "fuzz_smart.npz"), obs=obs.astype(np.int16), q=q, eps=eps, seed=np.uint32(seed), player=np.int32(player),
                        actions=acts.astype(np.int8), directions=dirs.astype(np.int8), features=feats)
    print("fuzz_smart: %d agent calls" % M, flush=True)


def main():
    R = gg.Runner()
    tmp = tempfile.mkdtemp(prefix="evg_fuzz_")
    gen_configs(R, tmp)
    gen_agents(R, tmp)
    gen_smart()


if __name__ == "__main__":
    main()
