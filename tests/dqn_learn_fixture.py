"""tests/golden/dqn_learn.npz (tools/gen_dqn_learn_golden.py: three steps of the reference's own DQNAgent.optimize_model with a real optim.Adam) and the
comparison against it, shared by the CPU test that measures the tolerance and the GPU test that applies it.

The reference forms its targets in float64 (numpy rewards) and the contract is fp32, so the comparison is not bit-equal.  Its tolerance is MEASURED on
the CPU: host_steps() runs the fp32 host model of the whole step -- the exact fmaf chain for both forwards (tests/dqn_model.py), td_head32, the float64
backward of tests/dqn_grad_model.py on the chain's activations rounded to fp32, the clamp, learner_model.adam32 -- and fixture_compare() gives its
deviation from the fixture: per parameter in units of lr, for the loss in fp32 ulps of the loss.  Measured (test_dqn_learn_abi.py asserts these figures
against the fixture, so they cannot go stale):

    FIXTURE_PARAM_DEV_LR  = the largest deviation of a compared parameter over the three steps, / lr
    FIXTURE_LOSS_DEV_ULPS = the largest deviation of a loss, / the fp32 spacing of the loss

The bounds are twice the measured values, as margin: the device equals the model bit for bit in the TD head and Adam and lies within the backward's
documented bound."""
import os

import numpy as np

import dqn_grad_model
import dqn_learn_model
import learner_model

NAMES = ("w1", "b1", "w2", "b2")
LR, STEPS = 1e-4, 3
FIXTURE_PARAM_DEV_LR = 2.9802322387695312e-4           # 2^-25 / lr: one fp32 spacing of a parameter in [0.25, 0.5); steps 0, 1, 2: 0.37e-4, 1.49e-4, 2.98e-4
FIXTURE_LOSS_DEV_ULPS = 1.3736514933407307              # steps 0, 1, 2: 0.76, 1.37, 0.20
FIXTURE_PARAM_BOUND_LR = 2 * FIXTURE_PARAM_DEV_LR
FIXTURE_LOSS_BOUND_ULPS = 2 * FIXTURE_LOSS_DEV_ULPS


def load_fixture():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dqn_learn.npz"))
    fx = {"gamma": float(z["gamma"]), "policy": [z["p_" + n] for n in NAMES], "target": [z["t_" + n] for n in NAMES], "batches": [], "after": [], "skip": [],
          "loss": []}
    for k in range(STEPS):
        fx["batches"].append({"state": z["s%d_state" % k], "next_state": z["s%d_next_state" % k], "action": z["s%d_action" % k],
                              "reward": z["s%d_reward" % k].astype(np.float32)})
        fx["after"].append([z["s%d_%s" % (k, n)] for n in NAMES])
        fx["skip"].append([z["s%d_skip_%s" % (k, n)] for n in NAMES])
        fx["loss"].append(float(z["s%d_loss" % k]))
    return fx


def fixture_compare(fx, k, params, loss):
    """step k's parameters and loss against the reference's -> (largest compared-parameter deviation / lr, loss deviation in fp32 ulps of the loss, the
    share of the elements left out)"""
    dev, left, total = 0.0, 0, 0
    for p, want, skip in zip(params, fx["after"][k], fx["skip"][k]):
        d = np.abs(np.asarray(p, np.float64) - want.astype(np.float64))
        dev = max(dev, float(d[~skip].max()))
        left, total = left + int(skip.sum()), total + skip.size
    ulps = abs(float(loss) - fx["loss"][k]) / float(np.spacing(np.float32(fx["loss"][k])))
    return dev / LR, ulps, left / float(total)


def host_steps(fx):
    """the fp32 host model of the three steps -> [(params after step k, loss of step k)]"""
    params = [a.copy() for a in fx["policy"]]
    m, v, ctl = [np.zeros_like(a) for a in params], [np.zeros_like(a) for a in params], learner_model.new_ctl()
    out = []
    for k in range(STEPS):
        b = fx["batches"][k]
        q_pred = dqn_grad_model.chain(b["state"], params, True)[1]
        q_next = dqn_grad_model.chain(b["next_state"], fx["target"], True)[1]
        td = dqn_learn_model.td_head32(q_pred, b["action"], q_next, b["reward"], None, None, fx["gamma"], "huber")
        grads = [g.astype(np.float32) for g in dqn_grad_model.backward(b["state"], params, True, td["gq"], clamp=1.0)[0]]
        params, m, v, ctl = learner_model.adam32(params, grads, m, v, ctl, lr=LR)
        out.append(([a.copy() for a in params], float(td["loss"])))
    return out
