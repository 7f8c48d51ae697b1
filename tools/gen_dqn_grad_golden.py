#!/usr/bin/env python3
"""Writes tests/golden/dqn_grad.npz from the reference's own agents/DQN family: QNetwork((105,), 132, seed, fc1_unit=48) as policy and target network
and DQNAgent.optimize_model (:218-282), run by the reference's own method on an object created without __init__ (imported from the reference tree at
run time, not restated).  Only numbers go into the file:

  w1 [48, 105], b1, w2 [132, 48], b2   the policy network before the step (float32)
  x [64, 105] float32                   the batch's states: observation rows of the reference's own seeded games (tests/golden/traj_random.npz)
  action [64, 7] int64                  the 7 unravelled actions per row, unit * 11 + node, as remember_game_state stores them
  q [64, 132] float32                   policy_net(state_batch), torch CPU
  expected [64, 7]                      expected_state_action_values: target_net(next states).topk(7)[0] * gamma + reward, in the dtype the reference
                                        computes it in
  loss                                  F.smooth_l1_loss(state_action_values, expected_state_action_values)
  g_w1, g_b1, g_w2, g_b2                the four .grad as autograd delivers them (a tensor hook on each parameter), float32
  c_w1, c_b1, c_w2, c_b2                ... after param.grad.data.clamp_(-1, 1), read where optimizer.step() is called

The memory and the optimizer are stand-ins that hold data only: sample() returns the 64 transitions in order, step() records the clamped gradients.

torch's forward sums in another order than the library's fmaf chain, so a candidate row is redrawn while any of its pre-activations -- the 48 hidden
ones, the 132 outputs -- lies within 4 x the first-order bound of tests/dqn_model.error_bound of zero; the generator asserts that none is left, which
keeps the fixture's ReLU masks those of the exact chain.  For the same reason a row is redrawn while one of torch's hidden activations lies further
than (B / 2) u a1 from the exact chain's: gW2's terms are d2 * a1 with torch's own a1, and with this the fixture's gW2 is a sum of the contract's
terms to within half of the model's E.

    python tools/gen_dqn_grad_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
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

SEED = 20261022
B, H1, GAMMA = 64, 48, 0.99


def margins(dm, x, params):
    """-> per row, the smallest |pre-activation| / bound over the hidden units and the outputs (float64 pre-activations)"""
    w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in params)
    x = np.asarray(x, np.float64)
    z1 = x @ w1.T + b1
    e1 = 106 * dm.U * (np.abs(b1) + np.abs(x) @ np.abs(w1).T)          # layer 1's share of dqn_model.error_bound
    z2 = np.maximum(z1, 0.0) @ w2.T + b2
    e2 = dm.error_bound(x, params)
    return np.minimum((np.abs(z1) / e1).min(1), (np.abs(z2) / e2).min(1))


def main():
    import torch
    import agents.DQN.DQNAgent as D
    import agents.DQN.QNetwork as QN
    import dqn_model as dm
    from qnet_model import layer
    traj = np.load(os.path.join(GOLDEN, "traj_random.npz"))
    obs, acts, rew = traj["obs"], traj["actions"], traj["reward"]
    g = torch.Generator().manual_seed(SEED)
    scale = {"fc1.weight": 0.02, "fc1.bias": 0.3, "fc2.weight": 0.2, "fc2.bias": 0.3}     # observations reach the hundreds: keep the hidden layer O(1)
    nets = []
    for seed in (1, 2):
        net = QN.QNetwork((105,), 132, seed, fc1_unit=H1)
        net.load_state_dict({k: torch.randn(v.shape, generator=g) * scale[k] for k, v in net.state_dict().items()})
        nets.append(net)
    policy, target = nets
    params = [t.detach().numpy().copy() for t in (policy.fc1.weight, policy.fc1.bias, policy.fc2.weight, policy.fc2.bias)]

    # ---- 64 transitions of the seeded games whose states keep every pre-activation of the policy network clear of zero
    rng = np.random.RandomState(SEED)
    picked, redrawn = [], 0

    def draw():
        nonlocal redrawn
        while True:
            key = (rng.randint(obs.shape[0]), rng.randint(int(traj["length"].min()) - 1), rng.randint(2))
            if key not in picked and margins(dm, obs[key].astype(np.float32)[None], params)[0] > 4.0:
                return key
            redrawn += 1

    while True:
        while len(picked) < B:
            picked.append(draw())
        x = np.stack([obs[k].astype(np.float32) for k in picked])
        # gW2's terms are d2 * a1 with torch's OWN a1: a row stays only while every hidden activation of torch's forward lies within (B / 2) u a1
        # of the exact chain's, so that sum_r d2 (a1_torch - a1_chain) is at most half of the model's E = B u sum_r |d2| a1 for gW2
        with torch.no_grad():
            a1_torch = torch.relu(policy.fc1(torch.from_numpy(x))).numpy().astype(np.float64)
        a1_chain = layer(x, params[0], params[1], True).astype(np.float64)
        far = (np.abs(a1_torch - a1_chain) > 0.5 * B * dm.U * a1_chain).any(1)
        if not far.any():
            break
        redrawn += int(far.sum())
        picked = [k for k, f in zip(picked, far) if not f]
    assert (margins(dm, x, params) > 4.0).all(), "a pre-activation within 4 x the bound of zero is left"
    assert ((a1_torch > 0) == (a1_chain > 0)).all()

    agent = D.DQNAgent.__new__(D.DQNAgent)                        # no __init__: nothing is built or loaded
    agent.batch_size, agent.gamma, agent.policy_net, agent.target_net = B, GAMMA, policy, target

    class Memory(object):
        def __init__(self):
            self.rows = []

        def push(self, *args):
            self.rows.append(D.Transition(*args))

        def __len__(self):
            return len(self.rows)

        def sample(self, n):
            assert n == len(self.rows)
            return list(self.rows)

    agent.memory = Memory()
    for game, turn, seat in picked:                               # remember_game_state unravels the 7 actions itself (:211-213)
        a = acts[game, turn, seat].astype(np.int64)
        a[:, 1] %= 11
        agent.remember_game_state(obs[game, turn, seat].astype(np.float64), a, float(rew[game, turn, seat]) + 0.25 * seat,
                                  obs[game, turn + 1, seat].astype(np.float64))
    seen = {}

    class Optimizer(object):
        def zero_grad(self):
            for p in policy.parameters():
                p.grad = None

        def step(self):
            seen["clamped"] = [p.grad.detach().clone().numpy() for p in policy.parameters()]

    class Functional(object):
        def __getattr__(self, k):
            return getattr(torch.nn.functional, k)

        def smooth_l1_loss(self, a, b):
            seen["predicted"], seen["expected"] = a.detach().clone(), b.detach().clone()
            return torch.nn.functional.smooth_l1_loss(a, b)

    agent.optimizer = Optimizer()
    raw = {}
    hooks = [p.register_hook(lambda grad, i=i: raw.__setitem__(i, grad.detach().clone().numpy())) for i, p in enumerate(policy.parameters())]
    D.F = Functional()
    try:
        agent.optimize_model()
    finally:
        D.F = torch.nn.functional
        for h in hooks:
            h.remove()
    action = torch.stack([t.action for t in agent.memory.rows]).long().numpy()
    with torch.no_grad():
        q = policy(torch.from_numpy(x)).numpy()
    assert np.array_equal(np.take_along_axis(q, action, 1), seen["predicted"].numpy())
    grads = [raw[i] for i in range(4)]
    assert all(np.array_equal(np.clip(a, -1, 1), c) for a, c in zip(grads, seen["clamped"]))
    assert any((np.abs(a) > 1).any() for a in grads), "no element is clamped: the clamped form would show nothing"
    names = ("w1", "b1", "w2", "b2")
    fx = dict(x=x, action=action, q=q, expected=seen["expected"].numpy(), loss=agent.loss.numpy())
    fx.update({n: p for n, p in zip(names, params)})
    fx.update({"g_" + n: a for n, a in zip(names, grads)})
    fx.update({"c_" + n: a for n, a in zip(names, seen["clamped"])})
    path = os.path.join(GOLDEN, "dqn_grad.npz")
    np.savez_compressed(path, **fx)
    print("optimize_model: %d rows (%d candidates redrawn), loss %.6f (%s), expected %s, %.1f %% of the outputs > 0, largest |grad| %s, clamped elements %s" % (
        B, redrawn, float(agent.loss), agent.loss.dtype, seen["expected"].dtype, 100.0 * (q > 0).mean(), [float(np.abs(a).max()) for a in grads],
        [int((np.abs(a) > 1).sum()) for a in grads]))
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    sys.path.insert(0, REF)
    sys.modules.setdefault("gym", types.ModuleType("gym"))         # agents/DQN/QNetwork.py imports gym and never uses it
    main()
