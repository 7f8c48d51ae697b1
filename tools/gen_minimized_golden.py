#!/usr/bin/env python3
"""Writes tests/golden/minimized_actions.npz and tests/golden/minimized_qnet.npz from the reference's own Minimized agent (agents/Minimized, imported from
the reference tree at run time, not restated).

minimized_actions.npz -- DQNAgent.get_best_actions and DQNAgent.get_action (agents/Minimized/DQNAgent.py:121-242), run by the reference's own methods on
an object created without __init__, on the observations of tests/golden/smart_actions.npz (M = 102 rows x 2 seats):
    obs [M, 2, 105] int16, q [M, 2, 12, 11] float32 -- seeded normals rounded to halves, so that exact ties within a swarm and between swarms are common;
    best [M, 2, 7, 2] int32 (get_best_actions); eps [M, 2] float32 (six levels), seed, episode [M]; actions [M, 2, 7, 2] int32 and explored [M, 2] uint8
    (get_action with the module's `random` and `np` replaced by proxies that serve random.random() and the two np.random.choice calls from the keyed
    draws of tests/minimized_model.explore_draws: the agent of row m is env id m, episode m % 3, turn = obs[0]).
minimized_qnet.npz -- QNetwork(59, 11, 80) (agents/Minimized/QNetwork.py) with fixed weights on the features of tests/golden/smart_state.npz:
    w1 [80, 59], b1, w2 [11, 80], b2 (float32), x [40, 12, 59] float32 (480 network rows), q [40, 12, 11] float32 (reference forward, torch CPU).

    python tools/gen_minimized_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("EVG_REFERENCE", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def gen_actions():
    import torch
    import agents.Minimized.DQNAgent as D
    import minimized_model as mm
    obs = np.load(os.path.join(GOLDEN, "smart_actions.npz"))["obs"]
    M = obs.shape[0]
    rng = np.random.RandomState(20261018)
    q = (np.round(rng.standard_normal((M, 2, 12, 11)) * 2.0) / 2.0).astype(np.float32)
    q[5, 0] = 0.25                                          # every swarm the same everywhere: argmax 0, order = swarm order
    q[6, 1, :, :] = q[6, 1, :1, :]                          # twelve equal swarms
    seed = 20261018
    eps_levels = np.array([0.0, 0.05, 0.3, 0.5, 0.95, 1.0], np.float32)
    eps = eps_levels[(np.arange(M)[:, None] + 3 * np.arange(2)[None, :]) % len(eps_levels)]
    cur = dict(m=0, p=0, turn=0)

    def draws():
        return mm.explore_draws(seed, cur["m"], cur["m"] % 3, cur["turn"], cur["p"])

    class _Std(object):
        def random(self):
            return draws()[0] / 4294967296.0

    class _NpRandom(object):
        def choice(self, a, size, replace=True):
            assert size == 7 and replace is False and a in (12, 11)
            return np.array(draws()[1]) if a == 12 else np.array(draws()[2]) - 1

    class _Np(object):
        random = _NpRandom()

        def __getattr__(self, k):
            return getattr(np, k)

    agent = D.DQNAgent.__new__(D.DQNAgent)
    agent.num_nodes = 11
    best, actions = np.zeros((M, 2, 7, 2), np.int32), np.zeros((M, 2, 7, 2), np.int32)
    explored = np.zeros((M, 2), np.uint8)
    calls = []
    orig = D.DQNAgent.get_random_actions

    def tapped(self_):
        calls.append(1)
        return orig(self_)

    for m in range(M):
        for p in range(2):
            o = obs[m, p].astype(np.float64)
            agent.policy_net = lambda swarm_obs, m=m, p=p: torch.from_numpy(q[m, p, int(np.argmax(np.asarray(swarm_obs)[47:59]))].copy())
            a = agent.get_best_actions(o)
            assert a.shape == (7, 2) and np.array_equal(a, a.astype(np.int32))
            best[m, p] = a.astype(np.int32)
    D.random, D.np = _Std(), _Np()
    D.DQNAgent.get_random_actions = tapped
    try:
        for m in range(M):
            for p in range(2):
                o = obs[m, p].astype(np.float64)
                cur.update(m=m, p=p, turn=int(o[0]))
                agent.epsilon = float(eps[m, p])
                agent.policy_net = lambda swarm_obs, m=m, p=p: torch.from_numpy(q[m, p, int(np.argmax(np.asarray(swarm_obs)[47:59]))].copy())
                n0 = len(calls)
                a = agent.get_action(o)
                explored[m, p] = len(calls) - n0
                assert a.shape == (7, 2) and np.array_equal(a, a.astype(np.int32))
                actions[m, p] = a.astype(np.int32)
    finally:
        D.DQNAgent.get_random_actions = orig
        D.random, D.np = __import__("random"), np
    out = os.path.join(GOLDEN, "minimized_actions.npz")
    np.savez_compressed(out, obs=obs, q=q, best=best, eps=eps, seed=np.array([seed], np.uint64), episode=(np.arange(M) % 3).astype(np.uint32),
                        actions=actions, explored=explored)
    print("minimized_actions: %d rows x 2 seats, explored %d; wrote %s (%d bytes)" % (M, int(explored.sum()), out, os.path.getsize(out)))


def gen_qnet():
    import torch
    import agents.Minimized.QNetwork as QN
    x = np.load(os.path.join(GOLDEN, "smart_state.npz"))["features"].astype(np.float32).reshape(-1, 12, 59)[:40]
    net = QN.QNetwork(59, 11, 80)
    g = torch.Generator().manual_seed(111)
    net.load_state_dict({k: torch.randn(v.shape, generator=g) * 0.3 for k, v in net.state_dict().items()})
    with torch.no_grad():
        q = net(torch.from_numpy(x)).numpy().astype(np.float32)
    out = os.path.join(GOLDEN, "minimized_qnet.npz")
    np.savez_compressed(out, w1=net.fc1.weight.detach().numpy(), b1=net.fc1.bias.detach().numpy(), w2=net.fc2.weight.detach().numpy(),
                        b2=net.fc2.bias.detach().numpy(), x=x, q=q)
    print("minimized_qnet: QNetwork(59, 11, 80) on %d rows, %.1f %% of the outputs > 0; wrote %s (%d bytes)" % (
        x.shape[0] * 12, 100.0 * (q > 0).mean(), out, os.path.getsize(out)))


if __name__ == "__main__":
    sys.path.insert(0, REF)
    gen_actions()
    gen_qnet()
