#!/usr/bin/env python3
"""Stream time of Smart_State self-royale's forward at 65 536 envs, two seats, (h1, h2) = (60, 60), teams of 4 and a uniform assignment, alternating in
one process on one device (tools/population_time.py's protocol and cases, for the 59-60-60-5 network):

  pop          (a) SmartQPopulation(shared, swarm): the bucket pass + the grouped forward, every env through its own member
  plain        (b) one plain two-seat SmartQNet call -- the floor: the same rows, one weight set per seat
  four_where   (c) what a consumer runs without the grouped forward: four plain two-seat calls and the torch.where merges

and, with a library built from the parent commit (parent_lib), the three plain Smart_State kernels' launches -- compact one seat, compact two seats and
expanded, whose instruction streams this change leaves as they were -- through this build, through the parent's library, and through the parent's
library a second time (the parent-versus-parent spread of the same run).

Each figure is the median over ROUNDS alternations of the mean of a window of calls between two stream events; a window is sized per case, from a
calibration run after the warm-up, to last at least WINDOW_MS of stream time.  Prints one line per round, then median, min and max per case, and whether
(a) was below (c) in every round; redirect to profiles/r16_b_smart_population_time.txt.  short=1: a few calls of (a), (b) and (c) only, for a kernel
trace (the split between the bucket pass and the forward).

    python tools/smart_population_time.py [envs] [rounds] [window_ms] [parent_lib] [short]
"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

K, H1, H2 = 4, 60, 60


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def make_net(dev, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(59, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2), torch.nn.ReLU(), torch.nn.Linear(H2, 5),
                               torch.nn.ReLU()).to(dev)


def parent_calls(path, env, two, one, shared, swarm, out2, sh1, sw1, out1, x, outx):
    """evg_smart_qnet of the library at `path` (an older build: it lacks this build's newer entry points, so it is bound here by hand, with a handle of its
    own) for the three layouts, on the same tensors"""
    _lib = evg._lib
    P = C.CDLL(os.path.abspath(path))
    vp = C.c_void_p
    P.evg_create.argtypes = [C.POINTER(_lib.EvgConfig), C.POINTER(vp)]
    P.evg_smart_qnet.argtypes = [vp, C.POINTER(_lib.EvgQnet), C.c_int, C.c_int64, vp, vp, vp, vp]
    cfg = _lib.EvgConfig()
    cfg.struct_size, cfg.abi_version, cfg.num_envs, cfg.device_id = C.sizeof(_lib.EvgConfig), _lib.ABI_VERSION, 64, env.device.index
    cfg.seed, cfg.obs_dtype, cfg.auto_reset, cfg.rng_mode, cfg.tables = 5, _lib.OBS_F32, 1, _lib.RNG_KEYED_PHILOX, env.tables
    h = vp()
    assert P.evg_create(C.byref(cfg), C.byref(h)) == 0, "evg_create of the parent library failed"
    N = shared.shape[0]

    def seats():
        assert P.evg_smart_qnet(h, C.byref(two._descriptor(2)), _lib.QNET_COMPACT_SEATS, N, vp(shared.data_ptr()), vp(swarm.data_ptr()),
                                vp(out2.data_ptr()), env._stream()) == 0

    def compact():
        assert P.evg_smart_qnet(h, C.byref(one._descriptor(1)), _lib.QNET_COMPACT, N, vp(sh1.data_ptr()), vp(sw1.data_ptr()), vp(out1.data_ptr()),
                                env._stream()) == 0

    def expanded():
        assert P.evg_smart_qnet(h, C.byref(one._descriptor(1)), _lib.QNET_EXPANDED, x.shape[0], vp(x.data_ptr()), None, vp(outx.data_ptr()),
                                env._stream()) == 0
    return compact, seats, expanded


def main(N=65536, rounds=9, window_ms=300, parent_lib=None, short=False):
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
    x = torch.randn((N * 12, 59), generator=g).to(dev)
    sh1, sw1 = shared[:, 0].contiguous(), swarm[:, 0].contiguous()
    teams = [[make_net(dev, 10 * p + m) for m in range(K)] for p in range(2)]
    pop = env.smart_q_population(teams[0], teams[1])                                       # clear(): a uniform draw per env and seat
    plain = [env.smart_qnet((teams[0][m], teams[1][m])) for m in range(K)]
    one = env.smart_qnet(teams[0][0])
    q, qm = (torch.zeros((N, 2, 12, 5), device=dev) for _ in range(2))
    q1 = torch.zeros((N, 12, 5), device=dev)
    qx = torch.zeros((N * 12, 5), device=dev)
    parts = [torch.zeros((N, 2, 12, 5), device=dev) for _ in range(K)]
    member = pop.member
    print("rows per member: seat 0 %s seat 1 %s" % tuple(torch.bincount(member[:, p].long(), minlength=K).tolist() for p in range(2)), flush=True)

    def four_where():
        for m in range(K):
            plain[m](shared, swarm, out=parts[m])
        torch.where((member == 0)[:, :, None, None], parts[0], parts[1], out=qm)
        for m in range(2, K):
            torch.where((member == m)[:, :, None, None], parts[m], qm, out=qm)

    cases = [("pop", lambda: pop(shared, swarm, out=q)), ("plain", lambda: plain[0](shared, swarm, out=parts[0])), ("four_where", four_where)]
    four_where()
    pop(shared, swarm, out=q)
    torch.cuda.synchronize()
    assert torch.equal(q, qm), "the grouped forward and the merged plain launches disagree"
    if short:
        for k, fn in cases:
            print("%s %.2f us" % (k, timed(fn, 50)), flush=True)
        env.close()
        return 0
    cases += [("compact_new", lambda: one(sh1, sw1, out=q1)), ("seats_new", lambda: plain[0](shared, swarm, out=parts[0])),
              ("expanded_new", lambda: one.expanded(x, out=qx))]
    if parent_lib:
        olds = parent_calls(parent_lib, env, plain[0], one, shared, swarm, parts[0], sh1, sw1, q1, x, qx)
        for tag in ("parent", "parent_again"):
            for name, fn in zip(("compact_", "seats_", "expanded_"), olds):
                cases.append((name + tag, fn))
    reps = {}
    for k, fn in cases:
        timed(fn, 100)
        reps[k] = max(50, int(window_ms * 1000.0 / timed(fn, 100)) + 1)
    print("%d envs, %d rounds, calls per window: " % (N, rounds) + "  ".join("%s %d" % (k, reps[k]) for k, _ in cases), flush=True)
    res = {k: [] for k, _ in cases}
    for r in range(rounds):
        for k, fn in cases:
            res[k].append(timed(fn, reps[k]))
        print("round %d: " % r + "  ".join("%s %.2f us" % (k, res[k][-1]) for k, _ in cases), flush=True)
    for k, v in res.items():
        print("%-22s median %.2f us  min %.2f  max %.2f" % (k, statistics.median(v), min(v), max(v)))
    below = all(a < c for a, c in zip(res["pop"], res["four_where"]))
    print("pop / plain (medians) %.3f; pop / four_where %.3f; pop below four_where in every round: %s" % (
        statistics.median(res["pop"]) / statistics.median(res["plain"]), statistics.median(res["pop"]) / statistics.median(res["four_where"]), below))
    pop.check()
    env.close()
    return 0 if below else 1


if __name__ == "__main__":
    a = sys.argv[1:]
    sys.exit(main(int(a[0]) if a else 65536, int(a[1]) if len(a) > 1 else 9, int(a[2]) if len(a) > 2 else 300,
                  a[3] if len(a) > 3 and a[3] not in ("", "-") else None, len(a) > 4 and a[4] in ("1", "short")))
