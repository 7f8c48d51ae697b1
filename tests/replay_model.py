"""Host model of the device replay memory (everglades_amd.SmartReplay, include/evg.h evg_replay_*): our own numpy restatement of what
agents/Smart_State/Multi_Step.py (NStepModule), utils/reward_shaping.py and DQNAgent.remember_game_state / optimize_model's batch compute, kept in the
device's ring layout so that the tests can compare the metadata record for record.  Vectorised over envs; one call of record() per turn."""
import numpy as np

import rng_spec

DRAW_DOMAIN = 5             # counter word 3 of the sample draws
SHAPES =["normalized_score", "basic_reward", "penalize_long_games", "reward_short_games", "transition", "custom"]
F_NOT_DONE, F_FINAL = 1, 2


def shape_base(fn, mine, theirs, done, turn):
    """utils/reward_shaping.py, float64, elementwise over envs."""
    won = mine > theirs
    if fn == 0:
        return mine.astype(np.float64)
    if fn == 1:
        return np.where(done & won, 1.0, 0.0)
    if fn == 2:
        return np.where(done, np.where(won, 100.0, -0.1), -0.001)
    return np.where(done, np.where(won, (150.0 - turn.astype(np.float64)) / 150.0, -1.0), 0.0)


def row_mask(dirs):
    """[..., 7, 2] {swarm, direction} -> bool [..., 7]: the rows that push a transition (first row of each swarm in 0..11, direction != 0)."""
    sw, d = dirs[..., 0], dirs[..., 1]
    ok = (sw >= 0) & (sw < 12)
    first = np.ones(sw.shape, bool)
    for r in range(1, 7):
        for q in range(r):
            first[..., r] &= ~(ok[..., q] & (sw[..., q] == sw[..., r]))
    return ok & first & (d != 0)


class ReplayModel(object):
    def __init__(self, N, S, H, n, gamma, shaping="normalized_score", seat=0, episode_base=0, auto_reset=True, turn0=None, episode0=None, frozen0=None):
        self.N, self.S, self.slots, self.n, self.seat, self.auto_reset = N, S, H + 1, n, seat, auto_reset
        self.gpow = [float(gamma) ** k for k in range(n)]
        if isinstance(shaping, (tuple, list)):
            self.code, self.fn_from, self.fn_to, self.K = 4, SHAPES.index(shaping[1]), SHAPES.index(shaping[2]), int(shaping[3])
        else:
            self.code, self.fn_from, self.fn_to, self.K = SHAPES.index(shaping), 0, 0, 1
        self.episode_base = int(episode_base)
        sl = self.slots
        self.rew = np.zeros((sl, N, S, 2), np.float64)
        self.meta = np.zeros((sl, N, S, 4), np.int32)
        self.count = np.zeros((sl, N, S), np.uint8)
        self.dirs = np.zeros((sl, N, S, 7, 2), np.int32)
        z = np.zeros(N, np.int32)
        self.ctr = np.stack([z if turn0 is None else np.asarray(turn0, np.int32), z if episode0 is None else np.asarray(episode0, np.int32), z,
                             z if frozen0 is None else np.asarray(frozen0, np.int32)], 1)
        self.turn = 0

    def _shaped(self, reward, done, custom):
        if self.code == 5:
            return np.asarray(custom, np.float32).reshape(self.N, self.S).astype(np.float64)
        out = np.zeros((self.N, self.S), np.float64)
        rw = np.asarray(reward, np.float32).astype(np.float64)
        turn, ep = self.ctr[:, 0], self.ctr[:, 1]
        for s in range(self.S):
            p = self.seat if self.S == 1 else s
            mine, theirs = rw[:, p], rw[:, 1 - p]
            if self.code == 4:
                game = (self.episode_base + 1 + ep.astype(np.int64)).astype(np.float64)
                ratio = np.minimum(1.0, game / float(self.K))
                r1 = shape_base(self.fn_from, mine, theirs, done, turn) * (1.0 - ratio)
                r2 = shape_base(self.fn_to, mine, theirs, done, turn) * ratio
                out[:, s] = r1 + r2
            else:
                out[:, s] = shape_base(self.code, mine, theirs, done, turn)
        return out

    def record(self, directions, reward, done, custom=None):
        """directions [N, S, 7, 2] (or [N, 7, 2] for S = 1) the step of this turn wrote; reward [N, 2] f32; done [N]."""
        sl, n, N, S = self.slots, self.n, self.N, self.S
        t = self.turn
        slot, nxt = t % sl, (t + 1) % sl
        done = np.asarray(done).astype(bool)
        self.meta[nxt] = 0
        self.count[nxt] = 0
        self.dirs[slot] = np.asarray(directions, np.int32).reshape(N, S, 7, 2)
        c = self.ctr.copy()
        act = c[:, 3] == 0
        shaped = self._shaped(reward, done, custom)
        self.rew[slot][act] = np.stack([shaped[act], np.zeros_like(shaped[act])], -1)
        self.meta[slot][act] = np.stack([np.broadcast_to(c[act, 0:1], (act.sum(), S)), np.broadcast_to(c[act, 1:2], (act.sum(), S)),
                                         np.zeros((act.sum(), S), np.int32), np.zeros((act.sum(), S), np.int32)], -1)
        self.count[slot][act] = 0

        def shaped_of(j):
            return shaped if j == 0 else self.rew[(slot - j) % sl][:, :, 0]

        def finalise(j, mask, flags):
            total = shaped_of(j).copy()
            for k in range(n):
                if k + 1 <= j:
                    total = total + self.gpow[k] * shaped_of(j - k - 1)
                else:
                    total = total + 0.0
            ks = (slot - j) % sl
            self.rew[ks][mask, :, 1] = total[mask]
            self.meta[ks][mask, :, 2] = flags
            self.count[ks][mask] = row_mask(self.dirs[ks][mask]).sum(-1)

        finalise(n, act & (c[:, 2] >= n), F_FINAL | F_NOT_DONE)
        d = act & done
        for j in range(n - 1, -1, -1):
            finalise(j, d & (c[:, 2] >= j), F_FINAL)
        nd = act & ~done
        self.ctr[d] = np.stack([np.zeros(d.sum(), np.int32), c[d, 1] + 1, np.zeros(d.sum(), np.int32),
                                np.full(d.sum(), 0 if self.auto_reset else 1, np.int32)], 1)
        self.ctr[nd] = np.stack([c[nd, 0] + 1, c[nd, 1], c[nd, 2] + 1, np.zeros(nd.sum(), np.int32)], 1)
        self.turn += 1

    def size(self):
        return int(self.count.sum(dtype=np.int64))

    def draw(self, seed, call, batch):
        """The handles int32 [batch, 4] {slot, env, seat, row} of sample(batch, seed) as call number `call`: draw i takes word 0 of
        Philox((i, call & 0xffffffff, call >> 32, DRAW_DOMAIN), seed), t = (word * total) >> 32, and names the t-th transition in record order."""
        tr = self.transitions()
        total = len(tr["slot"])
        assert total > 0
        key = rng_spec._key(seed)
        call = int(call) & 0xFFFFFFFFFFFFFFFF
        t = [(rng_spec.philox4x32_10((i, call & rng_spec.MASK, call >> 32, DRAW_DOMAIN), key)[0] * total) >> 32 for i in range(int(batch))]
        return np.stack([tr["slot"][t], tr["env"][t], tr["seat"][t], tr["row"][t]], 1).astype(np.int32)

    def transitions(self):
        """Every transition of the memory in the device's record order: dict of arrays slot, env, seat, row, swarm, action, next_slot (-1 where
        not_done is 0), reward (float64 sum), not_done."""
        valid = row_mask(self.dirs) & (self.count > 0)[..., None]             # [slots, N, S, 7]
        k, e, s, r = np.nonzero(valid)
        flags = self.meta[k, e, s, 2]
        nd = (flags & F_NOT_DONE) != 0
        return dict(slot=k.astype(np.int32), env=e.astype(np.int32), seat=s.astype(np.int32), row=r.astype(np.int32),
                    swarm=self.dirs[k, e, s, r, 0], action=(self.dirs[k, e, s, r, 1] - 1).astype(np.int64),
                    next_slot=np.where(nd, (k + self.n) % self.slots, -1).astype(np.int32), reward=self.rew[k, e, s, 1], not_done=nd)
