#!/usr/bin/env python3
"""Times the agents/DQN family's learner step on the MI355X (include/evg_dqn_learn.h), h1 = 528 (125 796 parameters).

a) Adam on the network's four tensors, the same gradients for every form:
  (1) evg_adam_step_wide  (libevg_dqnlearn.so: the element launch over a grid and the one-thread ctl launch)
  (2) evg_adam_step       (libevg_learn.so: ONE workgroup of 1 024 threads, 123 trips per thread)
  (3) torch.optim.Adam in its default, foreach=True and fused=True forms, whichever the installed torch takes

b) The whole step at B = 128 (the reference's BATCH_SIZE), 1 024 and 16 384:
  (1) learner.step_on(batch)  (DqnFamilyLearner: two forwards, evg_dqn_td_head, evg_dqn_qnet_backward, evg_adam_step_wide)
  (2) the torch block of examples/dqn_training.py --device-backward: DqnQNet.with_grad, gather, DqnQNet.rows + topk(7), smooth_l1_loss, backward,
      clamp_, optim.Adam(default form).step() -- the same work as it stood before the learner
  (3) the same block with torch's own forward (examples/dqn_training.py without flags)

Timing: stream time per call from device events around CALLS calls, after a warm-up of every form.  The forms ALTERNATE inside one process, ROUNDS
bursts each: the figure is the median of the bursts, the spread each form's own min .. max.

    python tools/dqn_learn_time.py [out_file]
"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
import everglades_amd as evg

ROUNDS, WARM = 9, 10
H1, GAMMA, LR = 528, 0.99, 1e-4
SIZES = (128, 1024, 16384)


def burst(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                    # us per call


def alternate(forms, calls):
    """-> [(median, min, max)] per form: ROUNDS bursts of each, alternating"""
    for _ in range(WARM):
        for f in forms:
            f()
    torch.cuda.synchronize()
    t = [[] for _ in forms]
    for _ in range(ROUNDS):
        for i, f in enumerate(forms):
            t[i].append(burst(f, calls))
    return [(statistics.median(v), min(v), max(v)) for v in t]


def verdict(a, b, an, bn):
    return "%s faster" % an if a[2] < b[1] else "%s faster" % bn if b[2] < a[1] else "inside the spreads"


def make_net(dev):
    return torch.nn.Sequential(torch.nn.Linear(105, H1), torch.nn.ReLU(), torch.nn.Linear(H1, 132), torch.nn.ReLU()).to(dev)


def time_adam(env, lines):
    dev = env.device
    torch.manual_seed(2)
    net = make_net(dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    grads = [torch.randn(p.shape, generator=gen, device=dev) * 0.1 for p in net.parameters()]
    learner = env.dqn_learner(net, make_net(dev), lr=LR)
    L = evg._lib.load_learn()
    narrow = evg._lib.EvgAdamArgs()

    def f_wide():
        learner.adam_step(grads=grads)

    f_wide()                                                       # fills learner._adam
    C.memmove(C.byref(narrow), C.byref(learner._adam), C.sizeof(narrow))

    def f_narrow():
        rc = L.evg_adam_step(env._h, C.byref(narrow), env._stream())
        assert rc == 0, L.evg_last_error()

    forms, names = [f_wide, f_narrow], ["(1) evg_adam_step_wide", "(2) evg_adam_step (one workgroup)"]
    for label, kw in (("default", {}), ("foreach=True", {"foreach": True}), ("fused=True", {"fused": True})):
        tnet = make_net(dev)
        try:
            opt = torch.optim.Adam(tnet.parameters(), lr=LR, **kw)
            for p, g in zip(tnet.parameters(), grads):
                p.grad = g.clone()
            opt.step()
        except (TypeError, RuntimeError, ValueError) as e:
            lines.append("  torch.optim.Adam(%s): not available in this torch (%s)" % (label, str(e).splitlines()[0]))
            continue
        forms.append(opt.step)
        names.append("(3) torch.optim.Adam(%s).step()" % label)
    res = alternate(forms, 200)
    lines.append("a) Adam over the 105-%d-132 network's four tensors (%d elements):" % (H1, sum(p.numel() for p in net.parameters())))
    for name, (med, lo, hi) in zip(names, res):
        lines.append("  %-42s %8.1f us  (%.1f .. %.1f, spread %.1f)" % (name, med, lo, hi, hi - lo))
    lines.append("  wide / one workgroup = %.3f (%s)" % (res[0][0] / res[1][0], verdict(res[0], res[1], "wide", "one workgroup")))
    for name, r in zip(names[2:], res[2:]):
        lines.append("  wide / %s = %.3f (%s)" % (name[4:], res[0][0] / r[0], verdict(res[0], r, "wide", "torch")))


def time_step(env, B, lines):
    dev = env.device
    torch.manual_seed(B)
    gen = torch.Generator(device=dev).manual_seed(B)
    state = (torch.randn((B, 105), generator=gen, device=dev) * 3.0).round()      # observation-like: small integers
    nxt = (torch.randn((B, 105), generator=gen, device=dev) * 3.0).round()
    action = torch.randint(0, 132, (B, 7), generator=gen, device=dev)
    rew = torch.rand((B,), generator=gen, device=dev)
    forms = []
    # (1) the device learner
    policy, target = make_net(dev), make_net(dev)
    learner = env.dqn_learner(policy, target, lr=LR, gamma=GAMMA)
    batch = (state, action, nxt, rew, None)
    forms.append(lambda: learner.step_on(batch))

    # (2), (3) the torch block of examples/dqn_training.py
    def torch_block(device_backward):
        pol, tgt = make_net(dev), make_net(dev)
        opt = torch.optim.Adam(pol.parameters(), lr=LR)
        qnet, tnet = env.dqn_qnet(pol), env.dqn_qnet(tgt)

        def step():
            q = qnet.with_grad(state) if device_backward else pol(state)
            predicted = q.gather(1, action)
            expected = tnet.rows(nxt).topk(7, 1)[0] * GAMMA + rew.unsqueeze(1).repeat(1, 7)
            loss = F.smooth_l1_loss(predicted, expected)
            opt.zero_grad()
            loss.backward()
            for p in pol.parameters():
                p.grad.data.clamp_(-1, 1)
            opt.step()
        return step

    forms += [torch_block(True), torch_block(False)]
    names = ["(1) learner.step_on", "(2) torch block, --device-backward", "(3) torch block, torch forward"]
    calls = 100 if B <= 1024 else 30
    res = alternate(forms, calls)
    for name, (med, lo, hi) in zip(names, res):
        lines.append("  %6d rows  %-36s %8.1f us  (%.1f .. %.1f, spread %.1f)" % (B, name, med, lo, hi, hi - lo))
    lines.append("  %6d rows  step_on / torch block (--device-backward) = %.3f (%s); step_on / torch block (torch forward) = %.3f (%s)" % (
        B, res[0][0] / res[1][0], verdict(res[0], res[1], "step_on", "torch block"), res[0][0] / res[2][0], verdict(res[0], res[2], "step_on", "torch block")))


def main(out=None):
    lines = ["device: %s, torch %s; %d alternating bursts per form (median, min .. max), warm-up %d calls of each" % (
        torch.cuda.get_device_name(0), torch.__version__, ROUNDS, WARM)]
    env = evg.EvergladesVecEnv(64, seed=1)
    time_adam(env, lines)
    lines.append("b) one optimize_model, h1 = %d:" % H1)
    for B in SIZES:
        time_step(env, B, lines)
    env.close()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
