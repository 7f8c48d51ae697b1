#!/usr/bin/env python3
"""Writes tests/golden/dqn_agent.npz from the reference's own agents/DQN family (QNetwork.py, DQNAgent.py; imported from the reference tree at run time,
not restated).  Only numbers go into the file:

(a) forward   QNetwork((105,), 132, seed, fc1_unit=48).forward (torch CPU) with seeded weights on 64 observation rows of a seeded reference game
              (tests/golden/traj_random.npz): a_w1 [48, 105], a_b1, a_w2 [132, 48], a_b2, a_x [64, 105] float32, a_q [64, 132] float32.
(b) decode    DQNAgent.filter_actions (:161-197), run by the reference's own method on an object created without __init__, on 312 Q rows: uniform random;
              a grid of halves (ties are common); post-ReLU rows with many zeros; small integers; all zero; all negative; rows with NaN and +-Inf
              planted: b_q [312, 132] float32, b_rows [312, 7, 2] int32.
(c) exploring DQNAgent.get_action / epsilon_greedy (:119-159) on the first 104 rows of (b) x 2 seats.  The module's `random` and `np` are proxies that
    turn      serve random.random() and the two np.random.choice calls from the keyed stream (tests/dqn_model.explore_draws: the agent of row m is env id
              m, episode c_episode[m], turn c_turn[m], seat p); the module-global steps_done is 0 and eps_start = eps_end = the row's epsilon, so that
              eps_threshold IS that epsilon.  Epsilon takes the values 0, 0.3, 1 and per-row values; row 0's epsilon equals its coin exactly on both
              seats (its turn and episode were searched for coins that are float32 values) and explores: `sample > eps` is the greedy branch; row 1 has
              the next float32 below its coin and is greedy.  c_eps [104, 2] float32, c_turn, c_episode [104], c_seed, c_rows [104, 2, 7, 2] int32,
              c_explored [104, 2] uint8.

    python tools/gen_dqn_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("EVG_REFERENCE", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SEED = 20261021
M_C = 104


def gen_forward(out):
    import torch
    import agents.DQN.QNetwork as QN
    obs = np.load(os.path.join(GOLDEN, "traj_random.npz"))["obs"]            # [games, 151, 2, 105] int16: the reference's own seeded games
    turns = np.linspace(0, 150, 32).astype(int)
    x = np.stack([obs[0, t, p] for t in turns for p in range(2)]).astype(np.float32)      # 64 rows: game 0, both seats, start to end
    net = QN.QNetwork((105,), 132, 1, fc1_unit=48)
    g = torch.Generator().manual_seed(SEED)
    scale = {"fc1.weight": 0.02, "fc1.bias": 0.3, "fc2.weight": 0.2, "fc2.bias": 0.3}     # observations reach the hundreds: keep the hidden layer O(1)
    net.load_state_dict({k: torch.randn(v.shape, generator=g) * scale[k] for k, v in net.state_dict().items()})
    with torch.no_grad():
        q = net(x.copy()).numpy().astype(np.float32)                          # forward takes the numpy row batch (:66-69)
    out.update(a_w1=net.fc1.weight.detach().numpy(), a_b1=net.fc1.bias.detach().numpy(), a_w2=net.fc2.weight.detach().numpy(),
               a_b2=net.fc2.bias.detach().numpy(), a_x=x, a_q=q)
    print("forward: QNetwork(105, 132, fc1_unit=48) on %d rows, %.1f %% of the outputs > 0" % (x.shape[0], 100.0 * (q > 0).mean()))


def decode_rows():
    rng = np.random.RandomState(SEED)
    parts = [
        rng.uniform(-1.0, 1.0, (80, 132)),                                                # uniform random
        np.round(rng.standard_normal((80, 132)) * 2.0) / 2.0,                              # a grid of halves: ties
        np.maximum(rng.standard_normal((60, 132)) - 0.8, 0.0),                             # post-ReLU: many zeros
        rng.randint(-2, 4, (50, 132)).astype(np.float64),                                  # small integers
        np.zeros((4, 132)),                                                                # all zero
        -np.abs(rng.standard_normal((8, 132))) - 0.01,                                     # all negative
    ]
    special = rng.uniform(-1.0, 1.0, (30, 132))                                            # NaN and +-Inf planted
    for r in range(30):
        at = rng.choice(132, 6, replace=False)
        special[r, at[:2]] = np.nan
        if r % 3 != 0:
            special[r, at[2:4]] = np.inf
        if r % 3 != 1:
            special[r, at[4:]] = -np.inf
    special[28] = np.nan
    special[29, ::2] = np.inf
    q = np.concatenate(parts + [special]).astype(np.float32)
    q[3, :] = 0.5                                                                          # everything ties
    q[4] = np.tile(q[4, :11], 12)                                                          # twelve equal groups
    return q


def bare_agent(D):
    agent = D.DQNAgent.__new__(D.DQNAgent)                    # no __init__: nothing is built or loaded
    agent.num_groups, agent.num_nodes, agent.num_actions, agent.n_actions, agent.shape = 12, 11, 7, 7, (7, 2)
    agent.eps_decay = 0.001
    return agent


def gen_decode(out):
    import torch
    import agents.DQN.DQNAgent as D
    q = decode_rows()
    agent = bare_agent(D)
    rows = np.zeros((q.shape[0], 7, 2), np.int32)
    for m in range(q.shape[0]):
        a = agent.filter_actions(np.zeros((7, 2)), torch.from_numpy(q[m].copy()))
        assert a.shape == (7, 2) and np.array_equal(a, a.astype(np.int32))
        rows[m] = a.astype(np.int32)
    out.update(b_q=q, b_rows=rows)
    print("decode: %d rows; rows 0, 3 -> %s %s" % (q.shape[0], rows[0].tolist(), rows[3].tolist()))


def f32_coin(dm, m, p):
    """(turn, episode) of the first key of env m, seat p whose coin / 2^32 is a float32 value."""
    for episode in range(64):
        for turn in range(150):
            coin = dm.explore_draws(SEED, m, episode, turn, p)[0]
            if coin and float(np.float32(coin / 4294967296.0)) == coin / 4294967296.0:
                return turn, episode
    raise RuntimeError("no float32 coin")


def gen_explore(out):
    import torch
    import agents.DQN.DQNAgent as D
    import dqn_model as dm
    q = out["b_q"][:M_C]
    rng = np.random.RandomState(SEED + 1)
    turn = rng.randint(0, 150, M_C).astype(np.int32)
    episode = (np.arange(M_C) % 3).astype(np.uint32)
    levels = np.array([0.0, 0.3, 1.0], np.float32)
    eps = levels[(np.arange(M_C)[:, None] + np.arange(2)[None, :]) % 3].copy()
    eps[40:] = np.where(rng.uniform(size=(M_C - 40, 2)) < 0.5, rng.uniform(0.0, 1.0, (M_C - 40, 2)), eps[40:]).astype(np.float32)   # per-row values
    # rows 0 and 1: a key whose coin is a float32 value for BOTH seats is searched per row with seat 0, and seat 1's epsilon pinned the same way if its
    # coin happens to be one too (otherwise it keeps its level)
    for m in (0, 1):
        turn[m], episode[m] = f32_coin(dm, m, 0)
        for p in range(2):
            c = dm.explore_draws(SEED, m, int(episode[m]), int(turn[m]), p)[0] / 4294967296.0
            if float(np.float32(c)) == c:
                eps[m, p] = np.float32(c) if m == 0 else np.nextafter(np.float32(c), np.float32(0))
    cur = dict(m=0, p=0)

    def draws():
        return dm.explore_draws(SEED, cur["m"], int(episode[cur["m"]]), int(turn[cur["m"]]), cur["p"])

    calls = []

    class _Std(object):
        def random(self):
            return draws()[0] / 4294967296.0

    class _NpRandom(object):
        def choice(self, a, size, replace=True):
            assert size == 7 and replace is False and a in (12, 11)
            calls.append(a)
            return np.array(draws()[1] if a == 12 else draws()[2])

    class _Np(object):
        random = _NpRandom()

        def __getattr__(self, k):
            return getattr(np, k)

    agent = bare_agent(D)
    rows, explored = np.zeros((M_C, 2, 7, 2), np.int32), np.zeros((M_C, 2), np.uint8)
    D.random, D.np = _Std(), _Np()
    try:
        for m in range(M_C):
            for p in range(2):
                cur.update(m=m, p=p)
                D.steps_done = 0
                agent.eps_start = agent.eps_end = float(eps[m, p])        # eps_threshold = eps_end + 0 * exp(...) = the row's epsilon
                agent.policy_net = lambda obs, m=m: torch.from_numpy(q[m].copy())
                obs = np.zeros(105)
                obs[0] = turn[m]
                n0 = len(calls)
                a = agent.get_action(obs)
                assert agent.eps_threshold == float(eps[m, p]) and len(calls) - n0 in (0, 2)
                explored[m, p] = (len(calls) - n0) // 2
                assert a.shape == (7, 2) and np.array_equal(a, a.astype(np.int32))
                rows[m, p] = a.astype(np.int32)
    finally:
        D.random, D.np = __import__("random"), np
    assert explored[0, 0] == 1 and explored[1, 0] == 0, "the pinned rows: coin == eps explores, the float32 below it does not"
    out.update(c_eps=eps, c_turn=turn, c_episode=episode, c_seed=np.array([SEED], np.uint64), c_rows=rows, c_explored=explored)
    print("exploring turn: %d rows x 2 seats, explored %d; pinned rows 0 / 1: eps %r / %r at turn %d / %d episode %d / %d" % (
        M_C, int(explored.sum()), eps[0].tolist(), eps[1].tolist(), turn[0], turn[1], episode[0], episode[1]))


if __name__ == "__main__":
    sys.path.insert(0, REF)
    sys.modules.setdefault("gym", types.ModuleType("gym"))     # agents/DQN/QNetwork.py imports gym and never uses it
    fx = {}
    gen_forward(fx)
    gen_decode(fx)
    gen_explore(fx)
    path = os.path.join(GOLDEN, "dqn_agent.npz")
    np.savez_compressed(path, **fx)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
