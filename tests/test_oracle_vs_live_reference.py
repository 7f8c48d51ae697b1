"""CPU test: the oracle against the reference on RANDOM configurations, recorded from the live reference.

tests/golden/custom_*.npz pin three hand-made non-default map / unit files.  These tests go further: oracle/gen_fuzz_golden.py draws random configurations
inside the domain include/evg.h states -- random DIRECTED graphs over the 11 nodes (1-5 outbound edges per node, distances 1..7, possibly disconnected),
control points 1..511, StructureDefense with up to two decimals incl. 0, random resource sets, bases on any two nodes, 3-4 unit types in random order with
random stats (an army's total damage <= 255) -- writes them as the reference's JSON files, lets the imported reference play keyed-random and 'wild' order
streams (oracle/gen_golden.py's Runner: the unmodified server with the keyed entropy source planted), random pairings of its own agent classes, and its
Smart_State agent methods on random inputs, and stores what the reference returned (tests/golden/fuzz_*.npz, with the JSON text of every configuration).
Here the oracle replays every turn: observations, scores, status, float64 health bits, packed groups and nodes, per-node list order, fog mask, knowledge
levels, the bots' orders, get_action and create_swarm_obs."""
import numpy as np

from conftest import load_golden


def test_oracle_smart_state_agent_equals_the_live_reference_on_random_inputs(oracle_mod):
    """DQNAgent.create_swarm_obs and DQNAgent.get_action (epsilon coin, get_random_actions, get_best_actions) of the reference on 1 500 random
    observations / Q tensors / epsilons (tests/golden/fuzz_smart.npz; the three draws served from the keyed stream by module proxies, as in
    oracle/gen_golden.py) against the oracle's restatements."""
    om = oracle_mod
    d = load_golden("fuzz_smart.npz")
    obs, q, eps = d["obs"].astype(np.float64), d["q"], d["eps"]
    M, seed, player = len(obs), int(d["seed"]), int(d["player"])
    assert M == 1500
    ga, gd, gx = om.smart_get_action(q, obs, seed, np.arange(M, dtype=np.uint32), (np.arange(M) % 5).astype(np.uint32), player, eps)
    assert np.array_equal(ga, d["actions"].astype(np.int32)) and np.array_equal(gd, d["directions"].astype(np.int32)), "get_action"
    assert np.array_equal(om.smart_state(obs), d["features"]), "create_swarm_obs"
    assert 0 < int(gx.sum()) < M                                             # both branches of the epsilon coin are exercised


def test_oracle_bots_equal_the_live_reference_agents_on_random_configurations(oracle_mod):
    """The same for the scripted opponents: random pairings of the reference's own agent classes (14 of agents/State_Machine/) on random maps / unit files,
    two consecutive episodes with the agent objects kept alive (tests/golden/fuzz_agents.npz) -- the oracle's bots emit the same orders, turn by turn, and
    the games end alike.  (The bots route by their own DemoMap constants whatever the map is; on a random map most of their orders are rejected by the server.)"""
    om = oracle_mod
    d = load_golden("fuzz_agents.npz")
    assert len(d["seed"]) == 12
    turns = 0
    for c in range(len(d["seed"])):
        pol = [int(x) for x in d["policy"][c]]
        o = om.Oracle(1, seed=int(d["seed"][c]), env_id_base=int(d["env_id"][c]), tables=om.tables_from_json_text(str(d["map_json"][c]), str(d["unit_json"][c])))
        for ep in range(2):
            obs = o.reset()
            T = int(d["length"][c, ep])
            for t in range(T):
                what = (c, str(d["pairing"][c]), ep, t)
                assert np.array_equal(obs[0], d["obs"][c, ep, t].astype(np.float64)), ("obs",) + what
                act = np.zeros((1, 2, 7, 2), np.int32)
                o.scripted_actions(pol[0], 0, obs, act)
                o.scripted_actions(pol[1], 1, obs, act)
                assert np.array_equal(act[0], d["actions"][c, ep, t]), ("orders",) + what + (act[0].tolist(), d["actions"][c, ep, t].tolist())
                obs, rew, done, info = o.step(act)
            assert done[0] == 1 and info["status"][0] == d["status"][c, ep] and np.array_equal(info["scores"][0], d["scores"][c, ep]), ("ending", c, ep)
            turns += T
    assert turns == int(d["length"].sum())


def test_oracle_equals_the_live_reference_on_random_configurations(oracle_mod):
    """10 random configurations x ('random', 'wild') order streams (tests/golden/fuzz_configs.npz) replayed turn by turn through the oracle."""
    om = oracle_mod
    d = load_golden("fuzz_configs.npz")
    assert len(d["length"]) == 20 and len(set(d["map_json"].tolist())) == 10
    for g in range(len(d["length"])):
        mtxt, utxt = str(d["map_json"][g]), str(d["unit_json"][g])
        o = om.Oracle(1, seed=int(d["seed"][g]), env_id_base=int(d["env_id"][g]), tables=om.tables_from_json_text(mtxt, utxt))
        obs = o.reset()
        assert np.array_equal(obs[0], d["obs"][g, 0].astype(np.float64)), ("reset obs", g)
        for t in range(int(d["length"][g])):
            obs, reward, done, info = o.step(d["actions"][g, t][None].astype(np.int32))
            what = (g, str(d["policy"][g]), t, mtxt, utxt)
            assert np.array_equal(obs[0], d["obs"][g, t + 1].astype(np.float64)), ("obs",) + what
            assert np.array_equal(info["scores"][0], d["scores"][g, t]) and info["status"][0] == d["status"][g, t] and done[0] == d["done"][g, t], \
                ("scores / status",) + what
            assert np.allclose(reward[0], d["reward"][g, t], rtol=0, atol=1e-12), ("reward",) + what
            s = o.get_state()
            assert np.array_equal(s["health"][0], d["health"][g, t + 1]), ("health bits",) + what
            assert np.array_equal(s["groups"][0], d["groups"][g, t + 1]) and np.array_equal(s["nodes"][0], d["nodes"][g, t + 1]), ("state",) + what
            assert np.array_equal(s["rank"][0], d["rank"][g, t + 1]), ("list order",) + what
            assert np.array_equal(o.fog_of_war()[0], d["fog"][g, t + 1]) and np.array_equal(o.knowledge()[0], d["know"][g, t + 1]), ("fog / knowledge",) + what
