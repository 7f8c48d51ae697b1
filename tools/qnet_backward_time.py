#!/usr/bin/env python3
"""Times the policy forward plus backward of optimize_model on the MI355X: torch (policy(x).gather(1, a).sum().backward(): the path every caller has
without this feature) against SmartQNet.with_grad / MinimizedQNet.with_grad (the fp32 evaluator's forward and the device's backward pass,
include/evg_qnet_grad.h) on the same operands.

Timing: stream time per call from device events around CALLS calls, after a warm-up of every shape.  The two forms ALTERNATE inside one process,
ROUNDS bursts each: the figure is the median of the bursts, the spread torch's own min .. max in the same run; the device form counts as faster
only where it wins by more than that spread.  B in 256, 1 024, 16 384, 65 536 rows of [B, 59]; networks 59-60-60-5 and 59-80-11.  The parameters'
.grad is set to None before every call in both forms (zero_grad's default), so neither pays an accumulation.

    python tools/qnet_backward_time.py [out_file]
"""
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import everglades_amd as evg

CALLS, ROUNDS, WARM = 200, 9, 30
BATCHES = (256, 1024, 16384, 65536)


def make_policy(kind, dev):
    torch.manual_seed(1)
    lin, relu = torch.nn.Linear, torch.nn.ReLU
    if kind == "smart":
        return torch.nn.Sequential(lin(59, 60), relu(), lin(60, 60), relu(), lin(60, 5)).to(dev)
    return torch.nn.Sequential(lin(59, 80), relu(), lin(80, 11), relu()).to(dev)


def burst(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                    # us per call


def alternate(f, g):
    for _ in range(WARM):
        f()
        g()
    torch.cuda.synchronize()
    t = ([], [])
    for _ in range(ROUNDS):
        t[0].append(burst(f))
        t[1].append(burst(g))
    return tuple((statistics.median(v), min(v), max(v)) for v in t)


def resource_usage():
    try:
        out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc"), "resource-usage", "FLAGS_EXTRA=-DEVG_GRAD"],
                             capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.SubprocessError) as e:
        return ["resource usage: not available (%s)" % e]
    lines = []
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = block.split()[0]
        if "qnet_grad" in name:
            u = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
            lines.append("%s: VGPRs %s, AGPRs %s, scratch %s, VGPR spill %s, SGPR spill %s, LDS %s B, occupancy %s waves/SIMD" % (
                name, u.get("VGPRs"), u.get("AGPRs"), u.get("ScratchSize [bytes/lane]"), u.get("VGPRs Spill"), u.get("SGPRs Spill"),
                u.get("LDS Size [bytes/block]"), u.get("Occupancy [waves/SIMD]")))
    return lines or ["resource usage: no backward kernel in the output"]


def main(out=None, with_resources=True):
    lines = ["device: %s, torch %s; policy forward + backward, %d calls per burst, %d alternating bursts per form (median, min .. max), warm-up %d "
             "calls of each" % (torch.cuda.get_device_name(0), torch.__version__, CALLS, ROUNDS, WARM)]
    env = evg.EvergladesVecEnv(256, seed=1)
    dev = env.device
    for kind in ("smart", "mini"):
        policy = make_policy(kind, dev)
        params = list(policy.parameters())
        net = (env.smart_qnet if kind == "smart" else env.minimized_qnet)(policy)
        width = net.OUT
        for B in BATCHES:
            g = torch.Generator(device="cpu").manual_seed(B)
            x = torch.rand((B, 59), generator=g).to(dev)
            a = torch.randint(0, width, (B, 1), generator=g).to(dev)

            def clear():
                for p in params:
                    p.grad = None

            def torch_form():
                clear()
                policy(x).gather(1, a).sum().backward()

            def device_form():
                clear()
                net.with_grad(x).gather(1, a).sum().backward()

            torch_form()
            want = [p.grad.clone() for p in params]
            device_form()
            err = max(float((p.grad - w).abs().max() / w.abs().max().clamp_min(1e-30)) for p, w in zip(params, want))
            (t_med, t_lo, t_hi), (d_med, d_lo, d_hi) = alternate(torch_form, device_form)
            spread = t_hi - t_lo
            verdict = "faster by more than torch's spread" if t_med - d_med > spread else (
                "slower by more than torch's spread" if d_med - t_med > spread else "within torch's spread")
            lines.append("%-5s B %6d   torch %7.1f us (%.1f .. %.1f, spread %.1f)   with_grad %7.1f us (%.1f .. %.1f)   %.2fx, %+.1f us: %s   "
                         "[max |grad difference| / max |grad| %.1e]" % (kind, B, t_med, t_lo, t_hi, spread, d_med, d_lo, d_hi, t_med / d_med,
                                                                         t_med - d_med, verdict, err))
    env.close()
    if with_resources:
        lines += resource_usage()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None, with_resources="--no-resources" not in sys.argv[1:])
