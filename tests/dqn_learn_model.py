"""Host model of the agents/DQN family's TD head (include/evg_dqn_learn.h: evg_dqn_td_head) in numpy, twice:

  td_head(...)    -> dict(estimated, td, gq, priorities, rows, loss) in float64 ("exact": every operation in double on the fp32 operands; the top-7
                     selection compares exactly, so it is the same in both)
  td_head32(...)  -> the same keys in the header's fp32 operation order, the loss summed in the header's order: bit for bit what the device computes

For Adam the tests import tests/learner_model.adam32 unchanged: evg_adam_step_wide is evg_adam_step per element.

top7(q_next) is the seven largest of a row WITH multiplicity, descending (a stable sort of the negated row: which index a tie came from is immaterial).
An action outside 0..131 reads nothing: its td is 0, so it adds 0 to the row's loss, to gq and to the priority.
gq starts from 0.0f and adds the pairs' g in ascending j, so duplicates add as gather's backward does."""
import numpy as np

F32 = np.float32
OUT, K = 132, 7
MODES = ("huber", "squared")
MAX_BLOCKS, SLOTS = 1024, 16                                # EVG_DQN_TD_MAX_BLOCKS, samples per workgroup and sweep
MAX_BATCH = 1 << 20


def top7(q_next):
    """[B, 132] -> [B, 7], the dtype of q_next"""
    q = np.asarray(q_next)
    return -np.sort(-q, axis=1, kind="stable")[:, :K]


def _operands(q_pred, action, q_next, reward, not_done, weights, dtype):
    q_pred, q_next, reward = (np.asarray(a, F32).astype(dtype) for a in (q_pred, q_next, reward))
    action = np.asarray(action, np.int64)
    B = q_pred.shape[0]
    assert q_pred.shape == (B, OUT) and q_next.shape == (B, OUT) and action.shape == (B, K) and reward.shape == (B,)
    nd = np.ones(B, bool) if not_done is None else np.asarray(not_done).astype(bool)
    w = None if weights is None else np.asarray(weights, F32).astype(dtype)
    return q_pred, action, q_next, reward, nd, w, B


def td_head(q_pred, action, q_next, reward, not_done, weights, gamma, mode):
    """float64 on the fp32 operands; gamma is taken as its fp32 value"""
    assert mode in MODES
    q_pred, action, q_next, reward, nd, w, B = _operands(q_pred, action, q_next, reward, not_done, weights, np.float64)
    gamma = float(F32(gamma))
    n = top7(q_next)
    est = np.where(nd[:, None], n * gamma, 0.0) + reward[:, None]
    valid = (action >= 0) & (action < OUT)
    qa = np.take_along_axis(q_pred, np.clip(action, 0, OUT - 1), 1)
    td = np.where(valid, qa - est, 0.0)
    ad = np.abs(td)
    ww = np.ones((B, 1)) if w is None else w[:, None]
    if mode == "squared":
        e, g = td * td * ww, 2.0 * td * ww / (K * B)
    else:
        e, g = ww * np.where(ad < 1.0, 0.5 * td * td, ad - 0.5), ww * np.clip(td, -1.0, 1.0) / (K * B)
    rows = e.sum(1)
    prio = (rows if mode == "squared" else ad.sum(1)) / 7.0 + float(F32(1e-5))
    gq = np.zeros((B, OUT))
    for j in range(K):
        np.add.at(gq, (np.arange(B)[valid[:, j]], action[valid[:, j], j]), g[valid[:, j], j])
    return {"estimated": est, "td": td, "gq": gq, "priorities": prio, "rows": rows, "loss": rows.sum() / (K * B)}


def loss_order32(rows, B):
    """sum of the fp32 rows [B] in the header's order, divided by (float)(7B): workgroup g of G takes the 16-sample groups g, g + G, ...; a slot (b % 16)
    adds its samples ascending, the workgroup its 16 slots ascending; lane l adds the partials l, l + 64, ...; the 64 lanes ascending"""
    rows = np.asarray(rows, F32)
    chunks = (B + SLOTS - 1) // SLOTS
    G = min(chunks, MAX_BLOCKS)
    pad = np.zeros(chunks * SLOTS, F32)
    pad[:B] = rows
    pad = pad.reshape(chunks, SLOTS)
    partial = np.zeros(G, F32)
    for g in range(G):
        acc = np.zeros(SLOTS, F32)
        for c in range(g, chunks, G):
            live = np.arange(SLOTS) + c * SLOTS < B
            acc = np.where(live, acc + pad[c], acc).astype(F32)
        s = acc[0]
        for k in range(1, SLOTS):
            s = F32(s + acc[k])
        partial[g] = s
    lanes = np.zeros(64, F32)
    for l in range(64):
        s = F32(0.0)
        for i in range(l, G, 64):
            s = F32(s + partial[i])
        lanes[l] = s
    t = lanes[0]
    for k in range(1, 64):
        t = F32(t + lanes[k])
    return F32(t / F32(K * B))


def td_head32(q_pred, action, q_next, reward, not_done, weights, gamma, mode):
    """the header's fp32 operation order, every statement one fp32 operation"""
    assert mode in MODES
    q_pred, action, q_next, reward, nd, w, B = _operands(q_pred, action, q_next, reward, not_done, weights, F32)
    gamma, f7B = F32(gamma), F32(K * B)
    n = top7(q_next)
    prod = np.where(nd[:, None], (n * gamma).astype(F32), F32(0.0)).astype(F32)
    est = (prod + reward[:, None]).astype(F32)
    valid = (action >= 0) & (action < OUT)
    qa = np.take_along_axis(q_pred, np.clip(action, 0, OUT - 1), 1)
    td = np.where(valid, (qa - est).astype(F32), F32(0.0)).astype(F32)
    ad = np.abs(td)
    if mode == "squared":
        e = (td * td).astype(F32)
        g = (F32(2.0) * td).astype(F32)
        if w is not None:
            e = (e * w[:, None]).astype(F32)
            g = (g * w[:, None]).astype(F32)
    else:
        e = np.where(ad < 1.0, ((F32(0.5) * td).astype(F32) * td).astype(F32), (ad - F32(0.5)).astype(F32)).astype(F32)
        g = np.clip(td, F32(-1.0), F32(1.0)).astype(F32)
        if w is not None:
            e = (w[:, None] * e).astype(F32)
            g = (w[:, None] * g).astype(F32)
    g = (g / f7B).astype(F32)
    rows, sad = e[:, 0], ad[:, 0]
    for j in range(1, K):
        rows = (rows + e[:, j]).astype(F32)
        sad = (sad + ad[:, j]).astype(F32)
    prio = (((rows if mode == "squared" else sad) / F32(7.0)).astype(F32) + F32(1e-5)).astype(F32)
    gq = np.zeros((B, OUT), F32)
    for j in range(K):                                      # j ascending; within one j every (b, action) pair is distinct
        idx = (np.arange(B)[valid[:, j]], action[valid[:, j], j])
        gq[idx] = (gq[idx] + g[valid[:, j], j]).astype(F32)
    return {"estimated": est, "td": td, "gq": gq, "priorities": prio, "rows": rows, "loss": loss_order32(rows, B)}
