#!/usr/bin/env python3
"""Times one optimize step on the MI355X: the training example's optimize_model with the device networks and --device-backward (the target forward
and the policy forward + backward are the library's, the TD target, the loss, the clamps and Adam are torch's: the fastest form without the learner)
against DqnLearner.step_on (include/evg_learn.h: every stage a launch of the library) on the same batch.

Timing: stream time per call from device events around CALLS calls, after a warm-up of every shape.  The two forms ALTERNATE inside one process,
ROUNDS bursts each: the figure is the median of the bursts, the spread the example form's own min .. max in the same run.  The condition a row must
meet: step_on is not slower than the example's form by more than that spread.  B in 256, 1 024, 16 384; networks 59-60-60-5 and 59-80-11; the batch
is gathered once from a played memory.  Each form trains its own copy of the policy, so neither sees the other's steps.  Launches per step are counted
with torch's profiler over one call of each form.

    python tools/learner_step_time.py [out_file]
"""
import copy
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import torch
import everglades_amd as evg
import smart_state_training as smart_example
import minimized_training as mini_example

CALLS, ROUNDS, WARM = 100, 9, 20
BATCHES = (256, 1024, 16384)


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


def launches(fn):
    """device kernels and copies one call starts"""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:                                       # the figure is a side note: the timing stands without it
        return "n/a (%s)" % type(e).__name__


def resource_usage():
    try:
        out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "everglades-ai-wargame_amd", "csrc"), "resource-usage",
                              "FLAGS_EXTRA=-DEVG_GRAD -DEVG_LEARN"], capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.SubprocessError) as e:
        return ["resource usage: not available (%s)" % e]
    lines = []
    for block in re.split(r"remark: Function Name: ", out.stdout + out.stderr)[1:]:
        name = block.split()[0]
        if "evg_learn_" in name:
            u = dict(re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[", block))
            lines.append("%s: VGPRs %s, AGPRs %s, scratch %s, VGPR spill %s, SGPR spill %s, LDS %s B, occupancy %s waves/SIMD" % (
                name, u.get("VGPRs"), u.get("AGPRs"), u.get("ScratchSize [bytes/lane]"), u.get("VGPRs Spill"), u.get("SGPRs Spill"),
                u.get("LDS Size [bytes/block]"), u.get("Occupancy [waves/SIMD]")))
    return lines or ["resource usage: no learner kernel in the output"]


def played(kind, envs=4096, turns=12):
    """an env, the example's two networks and a memory filled by `turns` turns of step_vs_q"""
    env = evg.EvergladesVecEnv(envs, seed=1, auto_reset=True)
    ex = smart_example if kind == "smart" else mini_example
    policy, target = ex.make_qnet(env.device, 0), ex.make_qnet(env.device, 1)
    mem = env.smart_replay(8, n_step=ex.N_STEP, gamma=ex.GAMMA, shaping="reward_short_games" if kind == "smart" else "custom", seats=0)
    act = (env.smart_qnet if kind == "smart" else env.minimized_qnet)(policy)
    env.reset()
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    for t in range(turns):
        q = act(*mem.slot_features(t))
        if kind == "smart":
            env.step_vs_q("swarm_agent", q, 0.3, seat=0, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
            mem.record()
        else:
            env.step_vs_q("random_actions", q, 0.3, seat=0, features=mem.slot_features(t + 1), actions_out=mem.slot_directions(t))
            mem.record(shaped=(env.reward[:, 0] / 10000.0).contiguous())
    return env, policy, target, mem


def main(out=None, with_resources=True):
    lines = ["device: %s, torch %s; one optimize step, %d calls per burst, %d alternating bursts per form (median, min .. max), warm-up %d calls of "
             "each" % (torch.cuda.get_device_name(0), torch.__version__, CALLS, ROUNDS, WARM)]
    failed = []
    for kind in ("smart", "mini"):
        env, policy, target, mem = played(kind)
        make_net = env.smart_qnet if kind == "smart" else env.minimized_qnet
        ex = smart_example if kind == "smart" else mini_example             # the learning rate, gamma and n_step are the example's own
        for B in BATCHES:
            batch = tuple(t.clone() for t in mem.sample(B, seed=B))
            # the example's form: its own copy of the policy, torch's Adam, the device target forward and the device backward
            p_example = copy.deepcopy(policy)
            opt = torch.optim.Adam(p_example.parameters(), lr=ex.LR)
            target_eval, policy_forward = make_net(target).expanded, make_net(p_example).with_grad
            if kind == "smart":
                example_form = lambda: smart_example.optimize_model(p_example, target, opt, batch, target_eval, policy_forward=policy_forward)
            else:
                example_form = lambda: mini_example.optimize_model(p_example, target_eval, opt, batch, policy_forward=policy_forward)
            p_learner = copy.deepcopy(policy)
            learner = (env.smart_learner if kind == "smart" else env.minimized_learner)(p_learner, target, mem, lr=ex.LR, gamma=ex.GAMMA, n_step=ex.N_STEP, clamp=1.0)
            learner_form = lambda: learner.step_on(batch)
            l_example, l_learner = float(example_form()), float(learner_form())
            n_example, n_learner = launches(example_form), launches(learner_form)
            (e_med, e_lo, e_hi), (d_med, d_lo, d_hi) = alternate(example_form, learner_form)
            spread = e_hi - e_lo
            ok = d_med - e_med <= spread
            if not ok:
                failed.append((kind, B))
            lines.append("%-5s B %6d   example (device nets + backward) %7.1f us (%.1f .. %.1f, spread %.1f), %s launches   learner.step_on %7.1f us "
                         "(%.1f .. %.1f), %s launches   %.2fx, %+.1f us: %s   [first loss %.6g / %.6g]" % (
                             kind, B, e_med, e_lo, e_hi, spread, n_example, d_med, d_lo, d_hi, n_learner, e_med / d_med, e_med - d_med,
                             "not slower than the example's form by more than its spread" if ok else "SLOWER than the example's form by more than its spread",
                             l_example, l_learner))
        env.close()
    lines.append("condition (step_on not slower than the example's form by more than that form's spread, every row): %s" % (
        "met" if not failed else "NOT met in %s" % failed))
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
