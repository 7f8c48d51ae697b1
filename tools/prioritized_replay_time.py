#!/usr/bin/env python3
"""Times a prioritized sample plus the priority update on the MI355X (device events around many calls, after a warm-up), in alternating rounds of
  (a) the library:  evg_replay_sample_prioritized + evg_replay_update_priorities (PrioritizedSmartReplay.sample / update_priorities);
  (b) the floor:    evg_replay_sample, the uniform draw over the same memory (no weights, no update);
  (c) torch:        the same step written with torch on a per-row priority tensor [slots, N, S, 7] the consumer keeps: effective weights (wmax where
                    never updated), torch.multinomial with replacement, index -> {slot, env, seat, row} arithmetic, importance weights, evg_replay_gather
                    for the batch, index_put of priority ** alpha and the running maximum.  Which rows are transitions, and their number, are handed to
                    it precomputed (in a training loop they change every turn and would have to be recomputed from the order rows: not charged here).
The bar: (a) is not slower than (c) in any round.

    python tools/prioritized_replay_time.py [envs] [batch] [out_file]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg

ALPHA, BETA, ROUNDS, REPS = 0.6, 0.4, 5, 200


def timed(fn, reps, warm=20):
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


def valid_rows(mem):
    """bool [slots, N, S, 7] on the device: the order rows that are transitions (first row of each swarm in 0..11, direction != 0, in a record that
    holds transitions)."""
    d = mem.directions.reshape(mem.slots, mem.N, mem.S, 7, 2)
    sw, dr = d[..., 0], d[..., 1]
    ok = (sw >= 0) & (sw < 12)
    first = torch.ones_like(ok)
    for r in range(1, 7):
        for q in range(r):
            first[..., r] &= ~(ok[..., q] & (sw[..., q] == sw[..., r]))
    return ok & first & (dr != 0) & (mem.counts.reshape(mem.slots, mem.N, mem.S) > 0)[..., None]


def main(N=65536, B=1024, out=None):
    lines = ["device: %s, envs %d, capacity_turns 8, batch %d, alpha %.1f, beta %.1f, torch %s; %d rounds x %d calls"
             % (torch.cuda.get_device_name(0), N, B, ALPHA, BETA, torch.__version__, ROUNDS, REPS)]
    env = evg.EvergladesVecEnv(N, seed=1)
    env.reset()
    dev = env.device
    mem = env.prioritized_replay(8, alpha=ALPHA, n_step=1, gamma=0.999, shaping="reward_short_games", seats=0)
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))
    q = torch.randn((N, 12, 5), device=dev)
    for t in range(12):
        env.step_vs_q("swarm", q, 0.1, seat=0, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        mem.record()
    T = int(mem.size().item())
    lines.append("memory: %d transitions in %d records" % (T, mem.slots * N * mem.S))
    g = torch.Generator(device=dev).manual_seed(2)
    pri = (torch.randn((B,), device=dev, generator=g).abs() + 1e-5).contiguous()
    # give both forms the same history: one large batch of priorities
    big = mem.sample(65536, seed=1, beta=BETA)[6].clone()
    big_pri = (torch.randn((65536,), device=dev, generator=g).abs() + 1e-5).contiguous()
    mem.update_priorities(big, big_pri)

    def library():
        o = mem.sample(B, seed=3, beta=BETA)
        mem.update_priorities(o[6], pri)

    def uniform():
        mem.uniform_sample(B, seed=3)

    # the torch formulation's own state
    valid = valid_rows(mem).reshape(-1)
    validf = valid.to(torch.float32)
    prio = torch.zeros_like(validf)
    bl = big.long()
    prio[((bl[:, 0] * N + bl[:, 1]) * mem.S + bl[:, 2]) * 7 + bl[:, 3]] = big_pri ** ALPHA
    wmax = torch.maximum(torch.ones((), device=dev), prio.max())
    NS, S = N * mem.S, mem.S

    def torch_form():
        nonlocal wmax
        w = torch.where(prio != 0, prio, wmax) * validf
        idx = torch.multinomial(w, B, replacement=True)
        rec, row = idx // 7, idx % 7
        slot, es = rec // NS, rec % NS
        handles = torch.stack([slot, es // S, es % S, row], 1).to(torch.int32)
        p = w[idx] / w.sum()
        wts = (T * p) ** -BETA
        wts = wts / wts.max()
        batch = mem.gather(handles)
        neww = pri ** ALPHA
        prio[idx] = neww
        wmax = torch.maximum(wmax, neww.max())
        return batch, wts, handles

    rows, ok = [], True
    for r in range(ROUNDS):
        a, b, c = timed(library, REPS), timed(uniform, REPS), timed(torch_form, REPS)
        ok = ok and a <= c
        rows.append((a, b, c))
        lines.append("round %d: library sample + update %.1f us | uniform sample (floor) %.1f us | torch formulation %.1f us | library / torch %.2f"
                     % (r, a, b, c, a / c))
    lines.append("library not slower than the torch formulation in any round: %s" % ok)
    mem.check()
    env.close()
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    return rows


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 65536, int(a[1]) if len(a) > 1 else 1024, a[2] if len(a) > 2 else None)
