"""Host model of prioritized sampling over the agents/DQN family's device replay memory (everglades_amd.PrioritizedDqnReplay,
include/evg_dqn_replay.h evg_dqn_replay_priority): numpy for the weights and stamps, Python ints for the draw.  Built on
dqn_replay_model.DqnReplayModel, whose valid / meta say which records exist and in which order; the stamp, the weight, the quantisation and the Philox
words are those of tests/replay_priority_model.py (include/evg_replay_priority.h's rules, unchanged), restated for ONE weight per record:

  - weights float32 [slots, N] (0 = never updated), stamps uint32 [slots, N]: a stale stamp means the record counts as never updated;
  - a never-updated record weighs wmax -- the largest weight stored since the last clear, 1 after it -- as of the draw;
  - an update keeps the LARGEST of several priorities for one record;
  - draws use integer weights q = max(1, floor(w * 2 ** (32 - e))), frexp(wmax) = (m, e): probabilities q / Q."""
import numpy as np

from replay_priority_model import FLT_MAX, philox_words01, quantise, stamp, weight

S_BAD_HANDLE, S_BAD_PRIORITY = 2, 4


class DqnPriorityModel(object):
    def __init__(self, base, alpha):
        self.base, self.alpha = base, float(np.float32(alpha))
        self.clear()

    def clear(self):
        b = self.base
        self.weights = np.zeros((b.slots, b.N), np.float32)
        self.stamps = np.zeros((b.slots, b.N), np.uint32)
        self.wmax = np.float32(1.0)
        self.status = 0

    def load(self, weights, stamps, wmax):
        """Take the weights, stamps and wmax read back from the device."""
        self.weights = np.ascontiguousarray(weights, np.float32).reshape(self.weights.shape).copy()
        self.stamps = np.ascontiguousarray(stamps).view(np.uint32).reshape(self.stamps.shape).copy()
        self.wmax = np.float32(wmax)

    def record_stamps(self):
        return stamp(self.base.meta[..., 0], self.base.meta[..., 1])

    def update(self, handles, priorities):
        """The two launches of evg_dqn_replay_update_priorities: reset (weight 0, the record's stamp), then the maximum of the weights' bits."""
        b = self.base
        h = np.asarray(handles, np.int64).reshape(-1, 4)
        p = np.asarray(priorities, np.float32).reshape(-1)
        ok = (h[:, 0] >= 0) & (h[:, 0] < b.slots) & (h[:, 1] >= 0) & (h[:, 1] < b.N) & (h[:, 2] == 0) & (h[:, 3] == 0)
        hc = np.where(ok[:, None], h, 0)
        ok &= b.valid[hc[:, 0], hc[:, 1]] != 0
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
        k, e = h[:, 0], h[:, 1]
        self.weights[k, e] = 0
        self.stamps[k, e] = self.record_stamps()[k, e]
        w = weight(p, self.alpha)
        np.maximum.at(self.weights.view(np.uint32), (k, e), w.view(np.uint32))
        self.wmax = np.maximum(self.wmax, w.max())

    def effective(self):
        """float32 effective weight of every valid record in (slot, env) order: the stored one, or wmax where never updated or the stamp is stale."""
        k, e = np.nonzero(self.base.valid)
        fresh = self.stamps[k, e] == self.record_stamps()[k, e]
        w = self.weights[k, e]
        return np.where(fresh & (w != 0), w, self.wmax).astype(np.float32)

    def q(self):
        return quantise(self.effective(), self.wmax)

    def probabilities(self):
        q = self.q()
        return q.astype(np.float64) / float(int(q.sum(dtype=np.uint64)))

    def draw(self, seed, call, batch):
        """(handles int32 [batch, 4], index of each drawn record in (slot, env) order): draw i takes u = (word0 << 32) | word1 of its Philox block and
        the record that holds position (u * Q) >> 64."""
        q = self.q()
        assert len(q) > 0
        cum = np.cumsum(q, dtype=np.uint64)
        Q = int(cum[-1])
        w0, w1 = philox_words01(int(batch), call, seed)
        t = [(((int(a) << 32) | int(c)) * Q) >> 64 for a, c in zip(w0, w1)]
        idx = np.searchsorted(cum, np.array(t, np.uint64), side="right")
        return self.base.handles()[idx], idx

    def importance(self, idx, beta):
        """float64 importance weights of the drawn records: (T q / Q) ** -beta over the batch's largest."""
        q = self.q()
        T, Q = len(q), int(q.sum(dtype=np.uint64))
        w = np.power(T * q[idx].astype(np.float64) / float(Q), -float(np.float32(beta)))
        return w / w.max()
