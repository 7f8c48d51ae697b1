#!/usr/bin/env python3
"""Stream time of the populations' grouped bf16 forward (include/evg_pop_bf16.h) against the forms it replaces, alternating in one process on one device.

  acting   [envs] envs (default 65 536, then 4 096), two seats, teams of 4 with the uniform draw of clear(), 59-60-60-5 and 59-80-11:
             bf16_grouped   SmartQPopulationBf16 / QPopulationBf16 (shared, swarm)
             fp32_grouped   SmartQPopulation / QPopulation (shared, swarm): the form it replaces (the baseline)
             bf16_plain     one plain two-seat bf16 launch, one weight set per seat: the floor, reported only
  target   expanded layout, 12 B rows for B = 1 024 and 16 384, K = 4, through PopulationLearner.next_forward:
             bf16_grouped   one grouped bf16 call
             bf16_K_take    target_precision="bf16": K whole-batch bf16 launches plus K take_rows (the baseline)
             fp32_grouped   one grouped fp32 call (a second baseline)
  step     one PopulationLearner.step_on (max_mean) at B = 256, 1 024 and 16 384 with "bf16_grouped", "bf16" and "fp32" targets: reported only

The protocol of tools/qnet_bf16_time.py: a burst is CALLS calls between two stream events, BURSTS bursts per form, the forms alternating; each figure is
the median over the bursts, with the baseline's own min .. max.  A row holds when the new form's median is not above the baseline's by more than the
baseline's spread (max - min) in the same run.  Redirect to profiles/r22_b_population_bf16_time.txt.

    python tools/population_bf16_time.py [calls] [bursts]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

K = 4


def burst(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls


def net(kind, dev, seed):
    torch.manual_seed(seed)
    L, R = torch.nn.Linear, torch.nn.ReLU
    layers = [L(59, 60), R(), L(60, 60), R(), L(60, 5), R()] if kind == "smart" else [L(59, 80), R(), L(80, 11), R()]
    return torch.nn.Sequential(*layers).to(dev)


def measure(title, forms, baselines, calls, bursts, judged=True):
    """forms: [(name, fn)], the first one the new form; baselines: the names it is judged against.  -> True if every judged row holds"""
    for _, fn in forms:
        burst(fn, 20)
    res = {k: [] for k, _ in forms}
    for _ in range(bursts):
        for k, fn in forms:
            res[k].append(burst(fn, calls))
    print(title)
    for k, v in res.items():
        print("    %-14s median %9.2f us   min %9.2f   max %9.2f" % (k, statistics.median(v), min(v), max(v)))
    new = statistics.median(res[forms[0][0]])
    ok = True
    for b in baselines:
        base, spread = statistics.median(res[b]), max(res[b]) - min(res[b])
        holds = new <= base + spread
        ok = ok and (holds or not judged)
        print("    %s / %s = %.3f (%s's spread %.2f us)%s" % (forms[0][0], b, new / base, b, spread,
                                                             ": holds" if holds and judged else (": DOES NOT HOLD" if judged else "")))
    sys.stdout.flush()
    return ok


def acting(N, calls, bursts):
    env = evg.EvergladesVecEnv(N, seed=5, auto_reset=True)
    obs = env.reset()
    dev = env.device
    shared, swarm = torch.zeros((N, 2, 34), device=dev), torch.zeros((N, 2, 12, 13), device=dev)
    for p in range(2):
        s, w = env.smart_state_compact(p, obs)
        shared[:, p].copy_(s)
        swarm[:, p].copy_(w)
    g = torch.Generator(device="cpu").manual_seed(0)
    swarm.add_(torch.randn(swarm.shape, generator=g).to(dev) * 0.1)                       # rows that differ from env to env
    ok = True
    for kind in ("smart", "mini"):
        teams = [[net(kind, dev, 10 * p + m) for m in range(K)] for p in range(2)]
        make, single = (env.smart_q_population, env.smart_qnet) if kind == "smart" else (env.q_population, env.minimized_qnet)
        new, old = make(teams[0], teams[1], precision="bf16"), make(teams[0], teams[1])
        plain = single((teams[0][0], teams[1][0]), precision="bf16")
        q = torch.zeros((N, 2, 12, new.OUT), device=dev)
        forms = [("bf16_grouped", lambda: new(shared, swarm, out=q)), ("fp32_grouped", lambda: old(shared, swarm, out=q)),
                 ("bf16_plain", lambda: plain(shared, swarm, out=q))]
        ok = measure("acting, %s, %d envs x 2 seats, teams of %d (rows per member, seat 0: %s)" % (
            kind, N, K, torch.bincount(new.member[:, 0].long(), minlength=K).tolist()), forms, ["fp32_grouped"], calls, bursts) and ok
        new.check()
    env.close()
    return ok


def learners(env, kind, mode="max_mean"):
    dev = env.device
    make = env.smart_population_learner if kind == "smart" else env.minimized_population_learner
    out = {}
    for precision in ("bf16_grouped", "bf16", "fp32"):
        pol, tgt = [net(kind, dev, m) for m in range(K)], [net(kind, dev, 100 + m) for m in range(K)]
        out[precision] = make(pol, tgt, lr=1e-4, mode=mode, target_precision=precision)
    return out


def target_and_step(calls, bursts):
    env = evg.EvergladesVecEnv(64, seed=5)
    env.reset()
    dev = env.device
    g = torch.Generator(device="cpu").manual_seed(1)
    ok = True
    for kind in ("smart", "mini"):
        L = learners(env, kind)
        OUT = L["fp32"].OUT
        for B in (1024, 16384):
            nxt = torch.rand((B, 12, 59), generator=g).to(dev)
            ids = torch.randint(0, K, (B,), generator=g).to(torch.uint8).to(dev)
            forms = []
            for name, key in (("bf16_grouped", "bf16_grouped"), ("bf16_K_take", "bf16"), ("fp32_grouped", "fp32")):
                lrn = L[key]
                b = lrn._buffers(B)
                ids12 = lrn.expand_ids(ids, b["ids12"])
                forms.append((name, (lambda lrn=lrn, b=b, ids12=ids12: lrn.next_forward("target", nxt, ids12, b["q_next"], b["q_one"]))))
            ok = measure("target, %s, B = %d (12 B = %d expanded rows), K = %d" % (kind, B, 12 * B, K), forms, ["bf16_K_take", "fp32_grouped"], calls,
                         bursts) and ok
            torch.cuda.synchronize()
            assert torch.equal(L["bf16_grouped"].q_next, L["bf16"].q_next), "the two bf16 forms of the target disagree"
        for B in (256, 1024, 16384):
            batch = (torch.rand((B, 59), generator=g).to(dev), torch.randint(0, OUT, (B,), generator=g).to(dev), torch.rand((B, 12, 59), generator=g).to(dev),
                     torch.randn((B,), generator=g).to(dev), (torch.rand((B,), generator=g) < 0.8).to(dev))
            ids = torch.randint(0, K, (B,), generator=g).to(torch.uint8).to(dev)
            forms = [(key, (lambda lrn=L[key]: lrn.step_on(batch, ids))) for key in ("bf16_grouped", "bf16", "fp32")]
            measure("learner step, %s, B = %d, K = %d (reported only)" % (kind, B, K), forms, ["bf16", "fp32"], calls, bursts, judged=False)
    env.close()
    return ok


def main(calls=200, bursts=9):
    print("%s; %d calls per burst, %d bursts per form, alternating" % (torch.cuda.get_device_name(0), calls, bursts))
    ok = True
    for N in (65536, 4096):
        ok = acting(N, calls, bursts) and ok
    ok = target_and_step(calls, bursts) and ok
    print("every judged row holds: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    a = sys.argv[1:]
    sys.exit(main(int(a[0]) if a else 200, int(a[1]) if len(a) > 1 else 9))
