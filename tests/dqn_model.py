"""Host model of the agents/DQN family's device path (include/evg_dqn.h: evg_dqn_qnet, evg_dqn_actions, evg_dqn_get_action): our own numpy restatement of
agents/DQN/QNetwork.py's forward and of DQNAgent.filter_actions / epsilon_greedy (agents/DQN/DQNAgent.py:131-197), with the agent's random.random() and
np.random.choice served from the keyed stream.  It restates the header's contracts.

  network   every pre-activation is acc = b[j], then acc = fmaf(W[j][k], x[k], acc) for k ascending over all of k (0..104, then 0..h1-1), then torch's
            ReLU (a NaN stays a NaN) on the hidden layer and, with final_relu, on the output; the model has no padded units and no chunks.
  decode    filter_actions, every quirk kept (below).
  explore   RNG domain 4 exactly as the Minimized agents use it (minimized_model.explore_draws: blocks 0 and 1 of the key (env id, episode, turn,
            seat), the coin, the two partial Fisher-Yates draws; a seat runs one agent family per turn), with the reference's two differences: the node
            is the drawn element itself, 0..10 (np.random.choice(11, 7, replace=False), no + 1), and `sample > eps` is the greedy branch, so an env
            explores iff coin / 2^32 <= eps, compared in float64.
"""
import numpy as np

import minimized_model
from qnet_model import layer

IN, OUT, NUM_GROUPS, NUM_NODES, NUM_ROWS = 105, 132, 12, 11, 7
U = 2.0 ** -24                                          # the unit roundoff of fp32


def forward(x, params, final_relu):
    """Rows x [..., 105] -> Q [..., 132]: relu?(fc2(relu(fc1(x)))) by the float32 fmaf chain (qnet_model.layer, generic in K and H)."""
    w1, b1, w2, b2 = params
    lead = np.shape(x)[:-1]
    h = layer(np.asarray(x, np.float32).reshape(-1, IN), w1, b1, True)
    return layer(h, w2, b2, bool(final_relu)).reshape(lead + (OUT,))


def forward_f64(x, params, final_relu):
    """The same weights and inputs in float64 (the yardstick of the float32 chain's rounding error)."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in params)
    h = np.maximum(np.asarray(x, np.float64) @ w1.T + b1, 0.0)
    q = h @ w2.T + b2
    return np.maximum(q, 0.0) if final_relu else q


def error_bound(x, params):
    """E2 [..., 132]: how far ANY summation order of the two layers in fp32 may lie from forward_f64, to first order -- counted, not tuned.
    Layer 1 (105 products and the bias: 105 roundings, 106 u with the bound's own slack): E1[j] = 106 u (|b1[j]| + sum_k |W1[j][k]| |x[k]|).
    Layer 2 carries E1 through |W2| (the ReLU does not stretch an error) and adds its own h1 + 1 roundings on the float64 activations a1:
    E2[o] = sum_j |W2[o][j]| E1[j] + (h1 + 1) u (|b2[o]| + sum_j |W2[o][j]| a1[j]).  The final ReLU does not stretch it either."""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in params)
    x = np.asarray(x, np.float64)
    h1 = w1.shape[0]
    e1 = 106 * U * (np.abs(b1) + np.abs(x) @ np.abs(w1).T)
    a1 = np.maximum(x @ w1.T + b1, 0.0)
    return e1 @ np.abs(w2).T + (h1 + 1) * U * (np.abs(b2) + a1 @ np.abs(w2).T)


def filter_actions(q):
    """q float32 [132] -> int32 [7, 2] of {unit, node}: DQNAgent.filter_actions (:161-197).  Three arrays of seven start at zero; for node 0..10, for
    group 0..11, for slot 0..6: where q[group * 11 + node] > best_q[slot] -- the group already among the seven unit values (an unfilled slot counts as
    unit 0) and not this slot's: on to the next slot; otherwise the slot takes {q, group, node} and the slot loop ends.  Nodes stay 0..10.  A NaN or a
    q <= 0 is never taken.  Comparisons on the fp32 values."""
    q = np.asarray(q, np.float32)
    best = [np.float32(0)] * NUM_ROWS
    unit, node = [0] * NUM_ROWS, [0] * NUM_ROWS
    for n in range(NUM_NODES):
        for g in range(NUM_GROUPS):
            v = q[g * NUM_NODES + n]
            for i in range(NUM_ROWS):
                if v > best[i]:
                    if g in unit and unit[i] != g:
                        continue
                    best[i], unit[i], node[i] = v, g, n
                    break
    return np.array([unit, node], np.int32).T.copy()


def explore_draws(seed, env_id, episode, turn, player):
    """One agents/DQN epsilon_greedy call: (coin as a 32-bit integer, the 7 units, the 7 nodes in 0..10)."""
    coin, units, nodes = minimized_model.explore_draws(seed, env_id, episode, turn, player)
    return coin, units, [n - 1 for n in nodes]


def get_action(q, seed, env_ids, episodes, turns, player, eps):
    """q [N, 132]; eps float32 [N] -> (rows int32 [N, 7, 2], explored uint8 [N])."""
    N = q.shape[0]
    rows, explored = np.zeros((N, NUM_ROWS, 2), np.int32), np.zeros(N, np.uint8)
    for e in range(N):
        coin, units, nodes = explore_draws(seed, int(env_ids[e]), int(episodes[e]), int(turns[e]), player)
        if coin / 4294967296.0 <= float(np.float32(eps[e])):
            explored[e] = 1
            rows[e] = np.stack([units, nodes], axis=1)
        else:
            rows[e] = filter_actions(q[e])
    return rows, explored
