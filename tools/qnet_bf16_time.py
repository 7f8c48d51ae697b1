#!/usr/bin/env python3
"""Times the two Q networks' forward in both precisions on the MI355X -- the fp32 evaluators (evg_smart_qnet, evg_minimized_qnet) against the bf16
matrix-core ones (evg_smart_qnet_bf16, evg_minimized_qnet_bf16) -- and says how often the two precisions act alike.

Timing: stream time per call from device events around CALLS calls, after a warm-up of every shape.  The two precisions ALTERNATE inside one
process, ROUNDS rounds each: the figure is the median of the rounds, the spread their min .. max, so a difference can be held against the fp32
evaluator's own run-to-run spread in the same run.  Smart_State 59-60-60-5 and Minimized 59-80-11; compact [N, 34] + [N, 12, 13], two seats
[N, 2, ...] with a weight set per seat, expanded [N * 12, 59]; at 65 536 envs (786 432 expanded rows) and at 4 096.

Agreement (information, not an acceptance criterion): on the features of a real seeded game (random orders, ENVS_AGREE envs, TURNS_AGREE turns) and a
seeded random network, the share of envs whose decoded order rows are identical under both precisions (smart_actions / minimized_get_action at
epsilon 0) and the share of (env, swarm) rows with an equal argmax.

    python tools/qnet_bf16_time.py [out_file]
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
ENVS_AGREE, TURNS_AGREE = 16384, 40
BYTES_IN, BYTES_OUT = 760, {"smart": 240, "mini": 528}           # per env-seat in the compact layout
HBM_TBS = 8.0                                                     # MI355X peak HBM bandwidth, TB/s


def random_params(kind, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sizes = (59, 60, 60, 5) if kind == "smart" else (59, 80, 11)
    p = []
    for k, h in zip(sizes[:-1], sizes[1:]):                       # nn.Linear's default initialisation: U(-1 / sqrt(k), 1 / sqrt(k))
        p += [((torch.rand((h, k), generator=g) * 2 - 1) / k ** 0.5).to(dev), ((torch.rand((h,), generator=g) * 2 - 1) / k ** 0.5).to(dev)]
    return tuple(p)


def burst(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls                    # us per call


def alternate(f32, b16):
    """-> ((median, min, max) of fp32, the same of bf16): ROUNDS bursts of each, alternating"""
    for _ in range(WARM):
        f32()
        b16()
    torch.cuda.synchronize()
    t = ([], [])
    for _ in range(ROUNDS):
        t[0].append(burst(f32))
        t[1].append(burst(b16))
    return tuple((statistics.median(v), min(v), max(v)) for v in t)


def resource_usage():
    try:
        out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc"), "resource-usage", "FLAGS_EXTRA=-DEVG_BF16"],
                             capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.SubprocessError) as e:
        return ["resource usage: not available (%s)" % e]
    lines = []
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = block.split()[0]
        if "qnet_bf16" in name:
            u = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
            lines.append("%s: VGPRs %s, AGPRs %s, scratch %s, VGPR spill %s, SGPR spill %s, LDS %s B, occupancy %s waves/SIMD" % (
                name, u.get("VGPRs"), u.get("AGPRs"), u.get("ScratchSize [bytes/lane]"), u.get("VGPRs Spill"), u.get("SGPRs Spill"),
                u.get("LDS Size [bytes/block]"), u.get("Occupancy [waves/SIMD]")))
    return lines or ["resource usage: no bf16 kernel in the output"]


def time_family(env, kind, lines):
    N, dev = env.num_envs, env.device
    make = env.smart_qnet if kind == "smart" else env.minimized_qnet
    out_w = 5 if kind == "smart" else 11
    p0, p1 = random_params(kind, 1, dev), random_params(kind, 2, dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    shared, swarm = torch.rand((N, 34), generator=g).to(dev), torch.rand((N, 12, 13), generator=g).to(dev)
    shared2, swarm2 = torch.rand((N, 2, 34), generator=g).to(dev), torch.rand((N, 2, 12, 13), generator=g).to(dev)
    x = env.expand_smart_state(shared, swarm).reshape(N * 12, 59).contiguous()
    q, q2, qx = (torch.empty(s + (out_w,), device=dev) for s in ((N, 12), (N, 2, 12), (N * 12,)))
    nets = {prec: (make(p0, final_relu=False, precision=prec), make((p0, p1), final_relu=False, precision=prec)) for prec in ("fp32", "bf16")}
    shapes = [("compact [N,34]+[N,12,13]", lambda n: n[0](shared, swarm, out=q), 1),
              ("two seats [N,2,...]", lambda n: n[1](shared2, swarm2, out=q2), 2),
              ("expanded [%d,59]" % (N * 12), lambda n: n[0].expanded(x, out=qx), None)]
    for name, call, seats in shapes:
        (f_med, f_lo, f_hi), (b_med, b_lo, b_hi) = alternate(lambda: call(nets["fp32"]), lambda: call(nets["bf16"]))
        line = "%-5s %6d envs  %-26s fp32 %7.1f us (%.1f .. %.1f, spread %.1f)   bf16 %7.1f us (%.1f .. %.1f)   %.2fx, %.1f us saved" % (
            kind, N, name, f_med, f_lo, f_hi, f_hi - f_lo, b_med, b_lo, b_hi, f_med / b_med, f_med - b_med)
        if seats:
            floor = N * seats * (BYTES_IN + BYTES_OUT[kind]) / (HBM_TBS * 1e12) * 1e6
            line += "   [bytes / peak HBM: %.1f us; bf16 at %.1fx of it]" % (floor, b_med / floor)
        lines.append(line)


def agreement(lines):
    N = ENVS_AGREE
    env = evg.EvergladesVecEnv(N, seed=2026, auto_reset=True)
    env.reset()
    for _ in range(TURNS_AGREE):
        env.step(env.random_actions())
    obs = env.observe_seat(0).clone()
    shared, swarm = env.smart_state_compact(-1, obs)
    for kind in ("smart", "mini"):
        make = env.smart_qnet if kind == "smart" else env.minimized_qnet
        p = random_params(kind, 7, env.device)
        qf = make(p, final_relu=False, precision="fp32")(shared, swarm)
        qb = make(p, final_relu=False, precision="bf16")(shared, swarm)
        if kind == "smart":
            rf, rb = env.smart_actions(qf, 0, obs).clone(), env.smart_actions(qb, 0, obs).clone()
        else:
            rf, rb = env.minimized_get_action(qf, 0.0, seat=0).clone(), env.minimized_get_action(qb, 0.0, seat=0).clone()
        same_rows = (rf == rb).reshape(N, -1).all(1).float().mean().item()
        same_argmax = (qf.argmax(-1) == qb.argmax(-1)).float().mean().item()
        err = (qf - qb).abs().max().item()
        lines.append("%-5s agreement on a seeded game (%d envs after %d random turns, seeded random network): identical order rows in %.2f%% of envs, "
                     "equal argmax in %.2f%% of (env, swarm) rows; max |Q_fp32 - Q_bf16| = %.3g (max |Q| %.3g)" % (
                         kind, N, TURNS_AGREE, 100 * same_rows, 100 * same_argmax, err, qf.abs().max().item()))
    env.close()


def main(out=None):
    lines = ["device: %s, torch %s; %d calls per burst, %d alternating rounds per precision (median, min .. max), warm-up %d calls of each" % (
        torch.cuda.get_device_name(0), torch.__version__, CALLS, ROUNDS, WARM)]
    for N in (65536, 4096):
        env = evg.EvergladesVecEnv(N, seed=1, auto_reset=True)
        env.reset()
        for kind in ("smart", "mini"):
            time_family(env, kind, lines)
        env.close()
    agreement(lines)
    lines += resource_usage()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
