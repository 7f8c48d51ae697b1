"""Host model of the Minimized agents' device path (include/evg.h: evg_minimized_get_action, evg_step_vs_*_minimized_q, evg_minimized_qnet): our own numpy
restatement of agents/Minimized/DQNAgent.py's get_action / get_best_actions / get_random_actions / swarm_think and QNetwork.forward, with the agent's
random() and np.random.choice served from the keyed stream.  This file is also the statement of the Minimized use of RNG domain 4, next to
oracle/rng_spec.py's explore_draws (whose blocks, coin and swarm draw it shares; a seat runs one agent family per turn):

  explore (domain 4), Minimized: halves 0..6 of block 0 pick the 7 distinct swarms (explore_draws' own), halves 0..6 of block 1 the 7 distinct nodes of
                     np.random.choice(11, 7, replace=False) + 1 -- partial Fisher-Yates over the pool 0..10: j = i + ((h1[i] * (11 - i)) >> 16), swap,
                     node_i = pool[i] + 1 --, the coin is (half 7 of block 0 << 16 | half 7 of block 1) / 2^32.
"""
import numpy as np

import rng_spec
from qnet_model import fmaf32, layer  # noqa: F401  (the float32 fmaf chain)

NUM_SWARMS, NUM_NODES, NUM_ROWS = 12, 11, 7


def explore_draws(seed, env_id, episode, turn, player):
    """One Minimized DQNAgent.get_action call: (coin as a 32-bit integer, the 7 swarms, the 7 nodes in 1..11)."""
    coin, swarms, _ = rng_spec.explore_draws(seed, env_id, episode, turn, player)
    h1 = rng_spec.halves(rng_spec.philox4x32_10(rng_spec._ctr(rng_spec.DOMAIN_EXPLORE, 1, turn, 0, player, episode, env_id), rng_spec._key(seed)))
    pool = list(range(NUM_NODES))
    for i in range(NUM_ROWS):
        j = i + ((h1[i] * (NUM_NODES - i)) >> 16)
        pool[i], pool[j] = pool[j], pool[i]
    return coin, swarms, [n + 1 for n in pool[:NUM_ROWS]]


def swarm_best(v):
    """One swarm's 11 Q values -> (argmax + 1, sort key): the FIRST maximum, a NaN is the maximum; a NaN key sorts as +inf."""
    best, arg = np.float32(v[0]), 0
    for k in range(1, len(v)):
        x = np.float32(v[k])
        if x > best or (np.isnan(x) and not np.isnan(best)):
            best, arg = x, k
    return arg + 1, (np.float32(np.inf) if np.isnan(best) else best)


def best_actions(q):
    """q [12, 11] -> int32 [7, 2]: the swarms sorted by their best Q, ascending and stable; the first seven as {swarm, node}."""
    dec = [swarm_best(q[s]) for s in range(NUM_SWARMS)]
    order = sorted(range(NUM_SWARMS), key=lambda s: dec[s][1])           # Python's sort is stable
    return np.array([[s, dec[s][0]] for s in order[:NUM_ROWS]], np.int32)


def get_action(q, seed, env_ids, episodes, turns, player, eps):
    """q [N, 12, 11]; eps float32 [N] -> (rows int32 [N, 7, 2], explored uint8 [N])."""
    N = q.shape[0]
    rows, explored = np.zeros((N, NUM_ROWS, 2), np.int32), np.zeros(N, np.uint8)
    for e in range(N):
        coin, swarms, nodes = explore_draws(seed, int(env_ids[e]), int(episodes[e]), int(turns[e]), player)
        if coin / 4294967296.0 < float(np.float32(eps[e])):
            explored[e] = 1
            rows[e] = np.stack([swarms, nodes], axis=1)
        else:
            rows[e] = best_actions(q[e])
    return rows, explored


def forward(x, params, final_relu):
    """Expanded rows x [..., 59] -> Q [..., 11]: relu(fc2(relu(fc1(x)))) by the float32 fmaf chain; the ReLU is torch's (qnet_model.layer: a NaN stays
    a NaN, on the hidden layer and on the output), and the model has no padded units."""
    w1, b1, w2, b2 = params
    lead = x.shape[:-1]
    h = layer(np.asarray(x, np.float32).reshape(-1, 59), w1, b1, True)
    return layer(h, w2, b2, bool(final_relu)).reshape(lead + (NUM_NODES,))


def forward_compact(shared, swarm, params, final_relu):
    """Compact features shared [N, 34], swarm [N, 12, 13] -> Q [N, 12, 11]: the chain prefix b1 + the 34 shared terms once per env, continued per swarm
    with the 13 swarm terms and the one-hot term acc + W1[j][47 + s]."""
    w1, b1, w2, b2 = (np.asarray(t, np.float32) for t in params)
    shared, swarm = np.asarray(shared, np.float32), np.asarray(swarm, np.float32)
    N = shared.shape[0]
    pre = layer(shared, w1[:, :34], b1, False)
    acc = np.repeat(pre[:, None, :], 12, axis=1).reshape(N * 12, -1)
    sw = swarm.reshape(N * 12, 13)
    for k in range(13):
        acc = fmaf32(w1[None, :, 34 + k], sw[:, k:k + 1], acc)
    acc = (acc.reshape(N, 12, -1) + w1[:, 47:59].T[None]).astype(np.float32)      # fp32 add == fmaf(w, 1, acc)
    h = np.maximum(acc.reshape(N * 12, -1), np.float32(0))
    return layer(h, w2, b2, bool(final_relu)).reshape(N, 12, NUM_NODES)


def forward_f64(x, params, final_relu):
    """The same weights and inputs in float64 (the yardstick of the float32 chain's rounding error)."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in params)
    h = np.maximum(np.asarray(x, np.float64) @ w1.T + b1, 0.0)
    q = h @ w2.T + b2
    return np.maximum(q, 0.0) if final_relu else q
