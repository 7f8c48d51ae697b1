#!/usr/bin/env python3
"""Writes tests/golden/dqn_learn.npz from the reference's own agents/DQN family: three consecutive DQNAgent.optimize_model calls (:220-290) on
QNetwork((105,), 132, seed, fc1_unit=48) as policy and target network, run by the reference's own method on an object created without __init__
(imported from the reference tree at run time, not restated), with a REAL torch.optim.Adam(lr=1e-4).  Only numbers go into the file:

  p_w1 [48, 105], p_b1, p_w2 [132, 48], p_b2      the policy network before the first step (float32); t_*: the target network
  gamma
  s{k}_state [64, 105], s{k}_next_state float32, s{k}_action [64, 7] int64, s{k}_reward [64] float64      step k's batch, k = 0, 1, 2
  s{k}_loss                                        agent.loss after step k, in the dtype the reference computes it in
  s{k}_w1, s{k}_b1, s{k}_w2, s{k}_b2               the policy's parameters after step k
  s{k}_skip_w1, ...                                bool: elements left out of the comparison at step k -- those whose clamped reference gradient g had
                                                   0 < |g| < 100 x Adam's eps at this or an earlier step (Adam's quotient g / (|g| + eps) is
                                                   ill-conditioned there, and a parameter keeps its deviation)

The memory is a stand-in that holds data only: sample() returns the step's 64 transitions in order.

torch's forward sums in another order than the library's fmaf chain, so a candidate row is redrawn while any pre-activation of the policy network AS IT
IS AT THAT STEP -- the 48 hidden ones, the 132 outputs -- lies within 4 x the first-order bound of tests/dqn_model.error_bound of zero (the rule of
tools/gen_dqn_grad_golden.py); the generator asserts that none is left.  It also asserts that at most 1 % of the elements are left out at any step, and
starts again from another seed if not.

    python tools/gen_dqn_learn_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("EVG_REFERENCE", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

SEED = 20261023
B, H1, GAMMA, LR, STEPS = 64, 48, 0.99, 1e-4, 3
TINY = 100 * 1e-8                                           # 100 x Adam's eps
CAP = 0.01
NAMES = ("w1", "b1", "w2", "b2")


def attempt(seed):
    import torch
    import agents.DQN.DQNAgent as D
    import agents.DQN.QNetwork as QN
    import dqn_model as dm
    from gen_dqn_grad_golden import margins
    traj = np.load(os.path.join(GOLDEN, "traj_random.npz"))
    obs, acts, rew = traj["obs"], traj["actions"], traj["reward"]
    g = torch.Generator().manual_seed(seed)
    scale = {"fc1.weight": 0.02, "fc1.bias": 0.3, "fc2.weight": 0.2, "fc2.bias": 0.3}     # observations reach the hundreds: keep the hidden layer O(1)
    nets = []
    for s in (1, 2):
        net = QN.QNetwork((105,), 132, s, fc1_unit=H1)
        net.load_state_dict({k: torch.randn(v.shape, generator=g) * scale[k] for k, v in net.state_dict().items()})
        nets.append(net)
    policy, target = nets

    def host(net):
        return [t.detach().numpy().copy() for t in (net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias)]

    fx = {"gamma": np.float64(GAMMA)}
    fx.update({"p_" + n: a for n, a in zip(NAMES, host(policy))})
    fx.update({"t_" + n: a for n, a in zip(NAMES, host(target))})

    agent = D.DQNAgent.__new__(D.DQNAgent)                        # no __init__: nothing is built or loaded
    agent.batch_size, agent.gamma, agent.policy_net, agent.target_net = B, GAMMA, policy, target
    agent.optimizer = torch.optim.Adam(policy.parameters(), lr=LR)
    seen = {}
    agent.optimizer.register_step_pre_hook(lambda opt, args, kwargs: seen.__setitem__("clamped", [p.grad.detach().clone().numpy() for p in policy.parameters()]))

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

    rng = np.random.RandomState(seed)
    used, redrawn = set(), 0
    skip = [np.zeros(a.shape, bool) for a in host(policy)]
    for k in range(STEPS):
        params = host(policy)
        picked = []
        while len(picked) < B:
            key = (rng.randint(obs.shape[0]), rng.randint(int(traj["length"].min()) - 1), rng.randint(2))
            if key not in used and margins(dm, obs[key].astype(np.float32)[None], params)[0] > 4.0:
                picked.append(key)
                used.add(key)
            else:
                redrawn += 1
        x = np.stack([obs[key].astype(np.float32) for key in picked])
        assert (margins(dm, x, params) > 4.0).all(), "a pre-activation within 4 x the bound of zero is left"
        agent.memory = Memory()
        for game, turn, seat in picked:                           # remember_game_state unravels the 7 actions itself (:211-213)
            a = acts[game, turn, seat].astype(np.int64)
            a[:, 1] %= 11
            agent.remember_game_state(obs[game, turn, seat].astype(np.float64), a, float(rew[game, turn, seat]) + 0.25 * seat,
                                      obs[game, turn + 1, seat].astype(np.float64))
        agent.optimize_model()
        rows = agent.memory.rows
        fx["s%d_state" % k] = x
        fx["s%d_next_state" % k] = np.stack([obs[game, turn + 1, seat].astype(np.float32) for game, turn, seat in picked])
        fx["s%d_action" % k] = torch.stack([t.action for t in rows]).long().numpy()
        fx["s%d_reward" % k] = np.array([float(t.reward) for t in rows], np.float64)      # as the reference holds them; the learner takes them as fp32
        fx["s%d_loss" % k] = agent.loss.numpy()
        fx.update({"s%d_%s" % (k, n): a for n, a in zip(NAMES, host(policy))})
        skip = [s | ((np.abs(c) > 0) & (np.abs(c) < TINY)) for s, c in zip(skip, seen["clamped"])]
        fx.update({"s%d_skip_%s" % (k, n): s.copy() for n, s in zip(NAMES, skip)})
        left_out = sum(int(s.sum()) for s in skip) / float(sum(s.size for s in skip))
        print("step %d: loss %.6f (%s), %d candidates redrawn so far, largest |clamped gradient| %s, left out %.3f %%" % (
            k, float(agent.loss), agent.loss.dtype, redrawn, [float(np.abs(c).max()) for c in seen["clamped"]], 100 * left_out))
        if left_out > CAP:
            return None
    return fx


def main():
    for seed in range(SEED, SEED + 20):
        fx = attempt(seed)
        if fx is not None:
            break
        print("more than %.0f %% of the elements would be left out: drawing again" % (100 * CAP))
    else:
        raise SystemExit("no seed keeps the left-out elements within the cap")
    total = sum(fx["s0_skip_" + n].size for n in NAMES)
    for k in range(STEPS):
        assert sum(int(fx["s%d_skip_%s" % (k, n)].sum()) for n in NAMES) <= CAP * total
    path = os.path.join(GOLDEN, "dqn_learn.npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < (1 << 20)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    sys.path.insert(0, REF)
    sys.modules.setdefault("gym", types.ModuleType("gym"))         # agents/DQN/QNetwork.py imports gym and never uses it
    main()
