#!/usr/bin/env python3
"""Times the agents/DQN family's acting turn on the MI355X (include/evg_dqn.h): QNetwork(105 -> 528 -> 132), the decode and the exploring turn.

Forms, at 4 096 and 65 536 rows (envs), h1 = 528:
  (1) torch's net(obs) on the device -- nn.Sequential(Linear(105, 528), ReLU, Linear(528, 132), ReLU) under no_grad on the float32 observation rows:
      the only way without the library, and the comparand;
  (2) DqnQNet on the same rows (evg_dqn_qnet: one launch, the bit-exact fp32 chain);
  (3) dqn_get_action alone at epsilon 0.3 (evg_dqn_get_action; no comparand: there is no batched filter_actions anywhere else);
  (4) the acting turn: (2) on the seat's observation buffer + (3) + step_vs("random_actions").

Timing: stream time per call from device events around CALLS calls, after a warm-up of every form.  The forms ALTERNATE inside one process, ROUNDS
bursts each: the figure is the median of the bursts, the spread each form's own min .. max.  The expectation the numbers are held against: form (2) is
not slower than form (1) by more than form (1)'s spread, at either size.  The arithmetic floor of the chain is printed beside the figures: 2 x rows x
(105 x 528 + 528 x 132) FLOP, and the same with k padded to 108 and the output to 144, at the fp32 matrix rate of 256 CUs x 256 FLOP/clk x 2.4 GHz.

    python tools/dqn_time.py [out_file]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import everglades_amd as evg

ROUNDS, WARM = 9, 20
PEAK_TFLOPS = 256 * 256 * 2.4e9 / 1e12                            # 157.3: MI355X fp32 matrix (= vector) peak
H1 = 528


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


def time_size(N, lines):
    env = evg.EvergladesVecEnv(N, seed=1, auto_reset=True)
    env.reset()
    for _ in range(10):                                           # observations of a game under way
        env.step(env.random_actions())
    dev = env.device
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(105, H1), torch.nn.ReLU(), torch.nn.Linear(H1, 132), torch.nn.ReLU()).to(dev)
    qnet = env.dqn_qnet(net)
    obs_seat = env.observe_seat(0)
    x = obs_seat.float().clone()
    q = torch.empty((N, 132), device=dev)
    explored = torch.zeros(N, dtype=torch.uint8, device=dev)
    state = {"obs": obs_seat}

    def f_torch():
        with torch.no_grad():
            return net(x)

    def f_dqn():
        return qnet.rows(x, out=q)

    def f_head():
        return env.dqn_get_action(q, 0.3, seat=0, explored=explored)

    def f_turn():
        rows = env.dqn_get_action(qnet(state["obs"], out=q), 0.3, seat=0, explored=explored)
        state["obs"] = env.step_vs("random_actions", rows, seat=0)[0]

    with torch.no_grad():
        diff = (net(x) - qnet.rows(x)).abs().max().item()
    calls = 200 if N <= 4096 else 100
    res = alternate([f_torch, f_dqn, f_head, f_turn], calls)
    names = ["(1) torch net(obs)", "(2) DqnQNet", "(3) dqn_get_action", "(4) acting turn (2)+(3)+step_vs"]
    flop, flop_pad = 2.0 * N * (105 * H1 + H1 * 132), 2.0 * N * (108 * H1 + H1 * 144)
    floor, floor_pad = flop / (PEAK_TFLOPS * 1e12) * 1e6, flop_pad / (PEAK_TFLOPS * 1e12) * 1e6
    lines.append("%d rows, h1 = %d: %.2f GFLOP (%.2f padded): floor %.1f us (%.1f us padded) at %.1f TFLOP/s; max |torch - DqnQNet| = %.3g" % (
        N, H1, flop / 1e9, flop_pad / 1e9, floor, floor_pad, PEAK_TFLOPS, diff))
    for name, (med, lo, hi) in zip(names, res):
        lines.append("  %6d rows  %-34s %8.1f us  (%.1f .. %.1f, spread %.1f)" % (N, name, med, lo, hi, hi - lo))
    (t_med, t_lo, t_hi), (d_med, _, _) = res[0], res[1]
    lines.append("  %6d rows  DqnQNet / torch = %.2f; floor / DqnQNet = %.0f %% (padded floor: %.0f %%); expectation (2) <= (1) + spread of (1) = %.1f us: %s" % (
        N, d_med / t_med, 100 * floor / d_med, 100 * floor_pad / d_med, t_med + (t_hi - t_lo), "met" if d_med <= t_med + (t_hi - t_lo) else "MISSED"))
    env.close()


def main(out=None):
    lines = ["device: %s, torch %s; %d alternating bursts per form (median, min .. max), warm-up %d calls of each" % (
        torch.cuda.get_device_name(0), torch.__version__, ROUNDS, WARM)]
    for N in (4096, 65536):
        time_size(N, lines)
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
