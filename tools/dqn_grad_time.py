#!/usr/bin/env python3
"""Times optimize_model's policy forward + backward of the agents/DQN network on the MI355X (include/evg_dqn_grad.h): DqnQNet.with_grad against torch.

Forms, at B = 128 (the reference's BATCH_SIZE), 1 024, 16 384 and 65 536 rows, h1 = 528, the same parameters and the same dense upstream gradient:
  (1) torch: q = net(x); q.backward(gq) -- nn.Sequential(Linear(105, 528), ReLU, Linear(528, 132), ReLU) with autograd: the only way without the
      library, and the comparand;
  (2) DqnQNet.with_grad: q = qnet.with_grad(x); q.backward(gq) -- evg_dqn_qnet, then evg_dqn_qnet_backward behind autograd;
  (3) the backward entry point alone (evg_dqn_qnet_backward on a q computed before: the delta kernel, the weight-gradient kernel, the reduction).
The parameters' .grad are set to None before every call of (1) and (2), so that neither pays an accumulation.

Timing: stream time per call from device events around CALLS calls, after a warm-up of every form.  The forms ALTERNATE inside one process, ROUNDS
bursts each: the figure is the median of the bursts, the spread each form's own min .. max.  Beside the figures: the arithmetic floor of (3) at the
fp32 matrix rate of 256 CUs x 256 FLOP/clk x 2.4 GHz -- 2 x rows x 528 x (105 recomputed layer 1 + 132 d1 + 132 gW2 + 105 gW1) FLOP -- and the share
of it that (3) reaches.

    python tools/dqn_grad_time.py [out_file]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import everglades_amd as evg

ROUNDS, WARM = 9, 10
PEAK_TFLOPS = 256 * 256 * 2.4e9 / 1e12                            # 157.3: MI355X fp32 matrix (= vector) peak
H1 = 528
SIZES = (128, 1024, 16384, 65536)


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


def time_size(env, net, qnet, B, lines):
    dev = env.device
    gen = torch.Generator(device=dev).manual_seed(B)
    x = (torch.randn((B, 105), generator=gen, device=dev) * 3.0).round()      # observation-like: small integers
    gq = torch.randn((B, 132), generator=gen, device=dev) / B
    params = list(net.parameters())

    def clear():
        for p in params:
            p.grad = None

    def f_torch():
        clear()
        net(x).backward(gq)

    def f_device():
        clear()
        qnet.with_grad(x).backward(gq)

    q = qnet.rows(x).clone()
    ts = tuple(qnet._params())

    def f_entry():
        return qnet._backward(x, q, ts, gq, 0.0)

    f_torch()
    want = [p.grad.clone() for p in params]
    f_device()
    diff = max(float((p.grad - w).abs().max() / w.abs().max()) for p, w in zip(params, want))
    calls = 200 if B <= 1024 else 50 if B <= 16384 else 20
    res = alternate([f_torch, f_device, f_entry], calls)
    names = ["(1) torch net(x) + backward", "(2) with_grad(x) + backward", "(3) evg_dqn_qnet_backward alone"]
    flop = 2.0 * B * H1 * (105 + 132 + 132 + 105)
    floor = flop / (PEAK_TFLOPS * 1e12) * 1e6
    lines.append("%d rows, h1 = %d: backward %.2f GFLOP, floor %.1f us at %.1f TFLOP/s; max |with_grad .grad - torch .grad| / max |.grad| = %.3g" % (
        B, H1, flop / 1e9, floor, PEAK_TFLOPS, diff))
    for name, (med, lo, hi) in zip(names, res):
        lines.append("  %6d rows  %-34s %8.1f us  (%.1f .. %.1f, spread %.1f)" % (B, name, med, lo, hi, hi - lo))
    (t_med, t_lo, t_hi), (d_med, d_lo, d_hi), (e_med, _, _) = res
    lines.append("  %6d rows  with_grad / torch = %.2f (%s); floor / (3) = %.0f %%" % (
        B, d_med / t_med, "with_grad faster" if d_hi < t_lo else "torch faster" if t_hi < d_lo else "inside the spreads", 100 * floor / e_med))


def main(out=None):
    lines = ["device: %s, torch %s; %d alternating bursts per form (median, min .. max), warm-up %d calls of each" % (
        torch.cuda.get_device_name(0), torch.__version__, ROUNDS, WARM)]
    env = evg.EvergladesVecEnv(64, seed=1)
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(105, H1), torch.nn.ReLU(), torch.nn.Linear(H1, 132), torch.nn.ReLU()).to(env.device)
    qnet = env.dqn_qnet(net)
    for B in SIZES:
        time_size(env, net, qnet, B, lines)
    env.close()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
