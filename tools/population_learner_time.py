#!/usr/bin/env python3
"""Times self-royale's learning block for ONE seat's team of K = 4 on the MI355X: the torch loop of examples/smart_state_self_royale.py (and its
Minimized twin) as it stood before the population learner -- the grouped target forward, then per member a torch forward of the whole batch, a masked
Huber loss, backward(), the clamp loop and an optim.Adam step -- against one PopulationLearner.step_on (include/evg_pop_learn.h) on the same batch.

Timing as tools/learner_step_time.py: stream time per call from device events around CALLS calls, after a warm-up; the two forms ALTERNATE inside
one process, ROUNDS bursts each; the figure is the median of the bursts, the spread the baseline's own min .. max in the same run.  The condition a
row must meet: step_on is not slower than the baseline by more than that spread.  B in 256, 1 024, 16 384; networks 59-60-60-5 and 59-80-11; the
batch is sampled once from a played memory and `who` gives each transition one of the four members (seeded, uniform).  Each form trains its own
copies of the policies.

    python tools/population_learner_time.py [out_file]
"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import torch.nn.functional as F
import smart_state_training as smart_example
import minimized_training as mini_example
import learner_step_time as single

K = 4
BATCHES = (256, 1024, 16384)


def baseline_block(policies, opts, tpop, batch, who, scale):
    """the example's learning block for seat 0, one masked optimize_model per member"""
    swarm_obs, action, next_state, reward, not_done = batch
    with torch.no_grad():
        nxt = tpop.expanded(next_state, who, 0)
        nxt = torch.where(not_done[:, None, None], nxt, torch.zeros_like(nxt))
        estimated = nxt.amax(2).mean(1) * scale + reward
    row = []
    for m in range(len(policies)):
        mine = (who == m).to(estimated.dtype)
        predicted = policies[m](swarm_obs).gather(1, action.unsqueeze(1)).squeeze(1)
        loss = (F.smooth_l1_loss(predicted, estimated, reduction="none") * mine).sum() / mine.sum().clamp(min=1.0)
        opts[m].zero_grad()
        loss.backward()
        for w in policies[m].parameters():
            w.grad.data.clamp_(-1, 1)
        opts[m].step()
        row.append(loss.detach())
    return torch.stack(row)


def main(out=None):
    lines = ["device: %s, torch %s; self-royale's learning block for one seat's team of %d, %d calls per burst, %d alternating bursts per form "
             "(median, min .. max), warm-up %d calls of each" % (torch.cuda.get_device_name(0), torch.__version__, K, single.CALLS, single.ROUNDS, single.WARM)]
    failed = []
    for kind in ("smart", "mini"):
        env, _, _, mem = single.played(kind)
        ex = smart_example if kind == "smart" else mini_example
        team = [ex.make_qnet(env.device, m) for m in range(K)]
        targets = [ex.make_qnet(env.device, 10 + m) for m in range(K)]
        for B in BATCHES:
            batch = tuple(t.clone() for t in mem.sample(B, seed=B))
            who = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(B), dtype=torch.int64).to(torch.uint8).to(env.device)
            p_base = [copy.deepcopy(n) for n in team]
            opts = [torch.optim.Adam(n.parameters(), lr=ex.LR) for n in p_base]
            tpop = (env.smart_q_population if kind == "smart" else env.q_population)(targets, targets, max_rows=12 * B)
            base_form = lambda: baseline_block(p_base, opts, tpop, batch, who, ex.GAMMA ** ex.N_STEP)
            p_new = [copy.deepcopy(n) for n in team]
            make = env.smart_population_learner if kind == "smart" else env.minimized_population_learner
            learner = make(p_new, targets, lr=ex.LR, gamma=ex.GAMMA, n_step=ex.N_STEP, mode="max_mean", clamp=1.0)
            new_form = lambda: learner.step_on(batch, who)
            l_base, l_new = base_form().tolist(), new_form().tolist()
            n_base, n_new = single.launches(base_form), single.launches(new_form)
            (b_med, b_lo, b_hi), (d_med, d_lo, d_hi) = single.alternate(base_form, new_form)
            spread = b_hi - b_lo
            ok = d_med - b_med <= spread
            if not ok:
                failed.append((kind, B))
            lines.append("%-5s B %6d   torch loop over %d members %8.1f us (%.1f .. %.1f, spread %.1f), %s launches   PopulationLearner.step_on %7.1f us "
                         "(%.1f .. %.1f), %s launches   %.2fx, %+.1f us: %s   [first losses %s / %s]" % (
                             kind, B, K, b_med, b_lo, b_hi, spread, n_base, d_med, d_lo, d_hi, n_new, b_med / d_med, b_med - d_med,
                             "not slower than the torch loop by more than its spread" if ok else "SLOWER than the torch loop by more than its spread",
                             " ".join("%.5g" % v for v in l_base), " ".join("%.5g" % v for v in l_new)))
        env.close()
    lines.append("condition (step_on not slower than the torch loop by more than that loop's spread, every row): %s" % (
        "met" if not failed else "NOT met in %s" % failed))
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
