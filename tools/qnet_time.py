#!/usr/bin/env python3
"""Times the Smart_State Q network's forward pass on the MI355X (device events around >= 200 calls, after a warm-up), 59-60-60-5:
  - evg_smart_qnet alone: compact [N, 34] + [N, 12, 13], two-seat [N, 2, ...], expanded [N * 12, 59];
  - the torch forwards it replaces: examples/smart_state_loop.py's make_network on the compact pair (one seat and both seats), and an nn.Sequential on
    expand_smart_state's [N, 12, 59];
  - the learner's turn (network + step_vs_q + record) and the self-play turn (networks + step_q), torch network against device network;
  - the kernel's line of `make resource-usage`.

    python tools/qnet_time.py [envs] [out_file]
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch
import everglades_amd as evg
from smart_state_loop import make_network

REPS = 300
FMA_COMPACT = 34 * 60 + 12 * (13 * 60 + 60 * 60 + 60 * 5)          # per env (the one-hot term is an add)


def timed(fn, reps=REPS, warm=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps                     # us per call


def resource_usage():
    try:
        out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc"), "resource-usage"], capture_output=True,
                             text=True, timeout=600)
    except (OSError, subprocess.SubprocessError) as e:
        return ["resource usage: not available (%s)" % e]
    lines = []
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = block.split()[0]
        if "qnet" in name:
            u = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
            lines.append("%s: VGPRs %s, AGPRs %s, scratch %s, VGPR spill %s, SGPR spill %s, LDS %s B, occupancy %s waves/SIMD" % (
                name, u.get("VGPRs"), u.get("AGPRs"), u.get("ScratchSize [bytes/lane]"), u.get("VGPRs Spill"), u.get("SGPRs Spill"),
                u.get("LDS Size [bytes/block]"), u.get("Occupancy [waves/SIMD]")))
    return lines or ["resource usage: no qnet kernel in the output"]


def main(N=65536, out=None):
    lines = ["device: %s, envs %d, torch %s, %d calls per figure after a warm-up" % (torch.cuda.get_device_name(0), N, torch.__version__, REPS)]
    env = evg.EvergladesVecEnv(N, seed=1, auto_reset=True)
    env.reset()
    dev = env.device
    g = torch.Generator(device="cpu").manual_seed(0)
    shared, swarm = env.smart_state_compact(-1, env.observe_seat(0))
    shared2 = torch.rand((N, 2, 34), generator=g).to(dev)
    swarm2 = torch.rand((N, 2, 12, 13), generator=g).to(dev)
    x = env.expand_smart_state(shared, swarm).contiguous()
    nets = (make_network(dev, 0), make_network(dev, 1))
    qn = env.smart_qnet(nets[0].params, final_relu=False)
    qpair = env.smart_qnet((nets[0].params, nets[1].params), final_relu=False)
    q, q2, qx = torch.empty((N, 12, 5), device=dev), torch.empty((N, 2, 12, 5), device=dev), torch.empty((N * 12, 5), device=dev)
    seq = torch.nn.Sequential(torch.nn.Linear(59, 60), torch.nn.ReLU(), torch.nn.Linear(60, 60), torch.nn.ReLU(), torch.nn.Linear(60, 5)).to(dev)
    xr = x.reshape(N * 12, 59)

    k_c = timed(lambda: qn(shared, swarm, out=q))
    k_s = timed(lambda: qpair(shared2, swarm2, out=q2))
    k_x = timed(lambda: qn.expanded(xr, out=qx))
    with torch.no_grad():
        t_c = timed(lambda: nets[0](shared, swarm))
        t_s = timed(lambda: torch.stack([nets[p](shared2[:, p].contiguous(), swarm2[:, p].contiguous()) for p in range(2)], dim=1))
        t_x = timed(lambda: seq(x))
    gf = lambda us, n_env: n_env * FMA_COMPACT * 2 / (us * 1e-6) / 1e12      # noqa: E731  (TFLOP/s of the compact chain)
    lines.append("kernel alone, compact [N,34]+[N,12,13]:     %7.1f us  (%.1f TFLOP/s of the compact chain's %.2f GFLOP)" % (
        k_c, gf(k_c, N), N * FMA_COMPACT * 2 / 1e9))
    lines.append("kernel alone, two seats [N,2,...]:          %7.1f us  (%.1f TFLOP/s)" % (k_s, gf(k_s, 2 * N)))
    lines.append("kernel alone, expanded [N*12,59]:           %7.1f us" % k_x)
    lines.append("torch, make_network on the compact pair:    %7.1f us  (kernel %.2fx faster)" % (t_c, t_c / k_c))
    lines.append("torch, make_network x 2 seats + stack:      %7.1f us  (kernel %.2fx faster)" % (t_s, t_s / k_s))
    lines.append("torch, nn.Sequential on expand_smart_state: %7.1f us  (kernel expanded %.2fx faster)" % (t_x, t_x / k_x))

    # the learner's turn: network + step_vs_q + record
    mem = env.smart_replay(8, n_step=1, gamma=0.999, shaping="reward_short_games", seats=0)
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    t = [0]

    def learner(device_net):
        def f():
            feats = mem.slot_features(t[0])
            if device_net:
                qq = qn(*feats, out=q)
            else:
                with torch.no_grad():
                    qq = nets[0](*feats)
            env.step_vs_q("swarm", qq, 0.1, seat=0, features=mem.slot_features(t[0] + 1), directions=mem.slot_directions(t[0]))
            mem.record()
            t[0] += 1
        return f

    l_t = timed(learner(False))
    mem.clear(); t[0] = 0
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    l_d = timed(learner(True))
    lines.append("learner turn (network + step_vs_q + record): torch network %.1f us, device network %.1f us" % (l_t, l_d))
    mem.check()

    # the self-play turn: both networks + step_q
    fs = (torch.empty((N, 2, 34), device=dev), torch.empty((N, 2, 12, 13), device=dev))
    for p in range(2):
        s_, w_ = env.smart_state_compact(p, env.obs)
        fs[0][:, p].copy_(s_)
        fs[1][:, p].copy_(w_)

    def selfplay(device_net):
        def f():
            if device_net:
                qq = qpair(*fs, out=q2)
            else:
                with torch.no_grad():
                    qq = torch.stack([nets[p](fs[0][:, p].contiguous(), fs[1][:, p].contiguous()) for p in range(2)], dim=1)
            env.step_q(qq, (0.1, 0.0), features=fs)
        return f

    s_t = timed(selfplay(False))
    s_d = timed(selfplay(True))
    lines.append("self-play turn (networks + step_q): torch networks %.1f us, device networks %.1f us" % (s_t, s_d))
    env.close()
    lines += resource_usage()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 65536, a[1] if len(a) > 1 else None)
