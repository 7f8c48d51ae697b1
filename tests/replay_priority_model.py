"""Host model of prioritized sampling over the device replay memory (everglades_amd.PrioritizedSmartReplay, include/evg.h evg_replay_priority): numpy for
the plane, Python ints for the draw.  Built on replay_model.ReplayModel, whose dirs / meta / count say which transitions exist and in which order.

Semantics (agents/DQN/PrioritizedMemory.py sample / update_priorities, with three documented differences):
  - plane float32 [slots, N, S, 8]: entry k < 7 the weight priority ** alpha of the record's k-th transition (0 = never updated), entry 7 the stamp of
    the record the entries belong to; a stale stamp means every transition of the record counts as never updated;
  - a never-updated transition weighs wmax -- the largest weight stored since the last clear, 1 after it -- as of the draw (difference 1);
  - an update keeps the LARGEST of several priorities for one transition (difference 2);
  - draws use integer weights q = max(1, floor(w * 2 ** (32 - e))), frexp(wmax) = (m, e): probabilities q / Q (difference 3)."""
import math

import numpy as np

import rng_spec
from replay_model import row_mask

PDRAW_DOMAIN = 7            # counter word 3 of the prioritized draws
S_EMPTY, S_BAD_HANDLE, S_BAD_PRIORITY = 1, 2, 4
FLT_MIN = np.float32(1.17549435e-38)
FLT_MAX = np.float32(3.402823466e+38)


def stamp(turn, episode):
    """uint32 stamp of a record's meta {turn, episode}."""
    return (np.uint32(0x80000000) | ((np.asarray(episode).astype(np.uint32) & np.uint32(0x7FFFFF)) << np.uint32(8))
            | (np.asarray(turn).astype(np.uint32) & np.uint32(0xFF))).astype(np.uint32)


def weight(priority, alpha):
    """float32 weights of float32 priorities: (float) pow((double) p, (double) alpha); alpha 1 gives p, alpha 0 gives 1; never below FLT_MIN."""
    p = np.asarray(priority, np.float32)
    alpha = float(np.float32(alpha))
    if alpha == 1.0:
        w = p.copy()
    elif alpha == 0.0:
        w = np.ones_like(p)
    else:
        w = np.power(p.astype(np.float64), alpha).astype(np.float32)
    return np.maximum(w, FLT_MIN)


def quantise(w, wmax):
    """uint64 integer weights of float32 effective weights w under the running maximum wmax."""
    e = math.frexp(float(np.float32(wmax)))[1]
    q = np.floor(np.ldexp(np.asarray(w, np.float32).astype(np.float64), 32 - e)).astype(np.uint64)
    return np.maximum(q, np.uint64(1))


def philox_words01(n, call, seed):
    """words 0 and 1 of Philox((i, call_lo, call_hi, PDRAW_DOMAIN), seed) for i < n, vectorised (rng_spec.philox4x32_10 states the rounds)."""
    M = np.uint64(rng_spec.MASK)
    k0, k1 = rng_spec._key(seed)
    call = int(call) & 0xFFFFFFFFFFFFFFFF
    c0 = np.arange(n, dtype=np.uint64)
    c1 = np.full(n, call & rng_spec.MASK, np.uint64)
    c2 = np.full(n, call >> 32, np.uint64)
    c3 = np.full(n, PDRAW_DOMAIN, np.uint64)
    for r in range(10):
        if r:
            k0, k1 = (k0 + rng_spec.W0) & rng_spec.MASK, (k1 + rng_spec.W1) & rng_spec.MASK
        p0, p1 = np.uint64(rng_spec.M0) * c0, np.uint64(rng_spec.M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & M, p0 & M
    return c0, c1


class PriorityModel(object):
    def __init__(self, base, alpha):
        """base: a ReplayModel (or anything with slots, N, S, dirs [slots, N, S, 7, 2], meta [slots, N, S, 4], count [slots, N, S])."""
        self.base, self.alpha = base, float(np.float32(alpha))
        self.clear()

    def clear(self):
        b = self.base
        self.plane = np.zeros((b.slots, b.N, b.S, 8), np.float32)
        self.wmax = np.float32(1.0)
        self.status = 0

    def load(self, plane, wmax):
        """Take the plane and wmax read back from the device."""
        self.plane = np.ascontiguousarray(plane, np.float32).reshape(self.plane.shape).copy()
        self.wmax = np.float32(wmax)

    # ------------------------------------------------------------------ which transitions exist
    def valid(self):
        """bool [slots, N, S, 7]: the order rows that are transitions of the memory."""
        b = self.base
        return row_mask(b.dirs) & (b.count > 0)[..., None]

    def stamps(self):
        return stamp(self.base.meta[..., 0], self.base.meta[..., 1])

    def transitions(self):
        """Every transition in record order: slot, env, seat, row, rank (the row's rank among its record's transitions)."""
        v = self.valid()
        k, e, s, r = np.nonzero(v)
        rank = (np.cumsum(v, -1) - 1)[k, e, s, r]
        return k, e, s, r, rank

    # ------------------------------------------------------------------ update
    def update(self, handles, priorities):
        """The two launches of evg_replay_update_priorities: reset (stale rows whole, else the entry), then the maximum of the weights' bits."""
        b = self.base
        h = np.asarray(handles, np.int64).reshape(-1, 4)
        p = np.asarray(priorities, np.float32).reshape(-1)
        ok = (h[:, 0] >= 0) & (h[:, 0] < b.slots) & (h[:, 1] >= 0) & (h[:, 1] < b.N) & (h[:, 2] >= 0) & (h[:, 2] < b.S) & (h[:, 3] >= 0) & (h[:, 3] < 7)
        v = self.valid()
        hc = np.where(ok[:, None], h, 0)
        ok &= v[hc[:, 0], hc[:, 1], hc[:, 2], hc[:, 3]]
        with np.errstate(invalid="ignore"):
            good = (p > 0) & (p <= FLT_MAX)
        if (~ok).any():
            self.status |= S_BAD_HANDLE
        if (~good).any():
            self.status |= S_BAD_PRIORITY
        acc = ok & good
        h, p = h[acc], p[acc]
        if not len(h):
            return
        rank = (np.cumsum(v, -1) - 1)[h[:, 0], h[:, 1], h[:, 2], h[:, 3]]
        rec = (h[:, 0] * b.N + h[:, 1]) * b.S + h[:, 2]
        u = self.plane.reshape(-1, 8).view(np.uint32)
        st = self.stamps().reshape(-1)
        stale = np.unique(rec[u[rec, 7] != st[rec]])
        u[stale, :7] = 0
        u[stale, 7] = st[stale]
        u[rec, rank] = 0
        w = weight(p, self.alpha)
        np.maximum.at(u, (rec, rank), w.view(np.uint32))
        self.wmax = np.maximum(self.wmax, w.max())

    # ------------------------------------------------------------------ draw
    def effective(self):
        """float32 effective weight of every transition in record order: the stored one, or wmax where never updated or the row's stamp is stale."""
        k, e, s, r, rank = self.transitions()
        fresh = self.plane.view(np.uint32)[k, e, s, 7] == self.stamps()[k, e, s]
        w = self.plane[k, e, s, rank]
        return np.where(fresh & (w != 0), w, self.wmax).astype(np.float32)

    def q(self):
        return quantise(self.effective(), self.wmax)

    def probabilities(self):
        q = self.q()
        return q.astype(np.float64) / float(int(q.sum(dtype=np.uint64)))

    def draw(self, seed, call, batch):
        """(handles int32 [batch, 4], index of each drawn transition in record order): draw i takes u = (word0 << 32) | word1 of its Philox block and
        the transition that holds position (u * Q) >> 64."""
        q = self.q()
        assert len(q) > 0
        cum = np.cumsum(q, dtype=np.uint64)
        Q = int(cum[-1])
        w0, w1 = philox_words01(int(batch), call, seed)
        t = [(((int(a) << 32) | int(c)) * Q) >> 64 for a, c in zip(w0, w1)]
        idx = np.searchsorted(cum, np.array(t, np.uint64), side="right")
        k, e, s, r, _ = self.transitions()
        return np.stack([k[idx], e[idx], s[idx], r[idx]], 1).astype(np.int32), idx

    def weights(self, idx, beta):
        """float64 importance weights of the drawn transitions: (T q / Q) ** -beta over the batch's largest."""
        q = self.q()
        T, Q = len(q), int(q.sum(dtype=np.uint64))
        w = np.power(T * q[idx].astype(np.float64) / float(Q), -float(np.float32(beta)))
        return w / w.max()
