"""Host model of the agents/DQN family's device replay memory (everglades_amd.DqnReplay, include/evg_dqn_replay.h): our own numpy restatement of what
DQNAgent.remember_game_state, utils/reward_shaping.py, SimpleMemory.ReplayMemory and optimize_model's batch compute, kept in the device's ring layout
so that the tests can compare record for record.  Vectorised over envs; one call of record() per turn.

The draw rule (evg_replay_draw_kernel's): draw i of sample call `call` takes word 0 of Philox((i, call & 0xffffffff, call >> 32, 5), seed),
t = (word * total) >> 32 with `total` the number of valid records, and names the t-th valid record in (slot, env) order."""
import numpy as np

import rng_spec
from replay_model import DRAW_DOMAIN, SHAPES, shape_base

F_NOT_DONE = 1
S_EMPTY, S_BAD_HANDLE, S_BAD_ACTION = 1, 2, 8


def actions_valid(rows):
    """[..., 7, 2] {unit, node} -> bool [...]: all seven rows have unit in 0..11 and node in 0..10."""
    u, n = rows[..., 0], rows[..., 1]
    return ((u >= 0) & (u < 12) & (n >= 0) & (n < 11)).all(-1)


def unravel(rows):
    """remember_game_state: action[i][0] * 11 + action[i][1] -> int64 [..., 7]"""
    return rows[..., 0].astype(np.int64) * 11 + rows[..., 1].astype(np.int64)


class DqnReplayModel(object):
    def __init__(self, N, H, shaping="reward_short_games", seat=0, episode_base=0, auto_reset=True, turn0=None, episode0=None, frozen0=None):
        self.N, self.H, self.slots, self.seat, self.auto_reset = N, H, H + 1, seat, auto_reset
        if isinstance(shaping, (tuple, list)):
            self.code, self.fn_from, self.fn_to, self.K = 4, SHAPES.index(shaping[1]), SHAPES.index(shaping[2]), int(shaping[3])
        else:
            self.code, self.fn_from, self.fn_to, self.K = SHAPES.index(shaping), 0, 0, 1
        self.episode_base = int(episode_base)
        sl = self.slots
        self.rew = np.zeros((sl, N), np.float64)
        self.meta = np.zeros((sl, N, 4), np.int32)
        self.valid = np.zeros((sl, N), np.uint8)
        self.rows = np.zeros((sl, N, 7, 2), np.int32)
        self.turn_of = np.full(sl, -1, np.int64)                               # the caller's turn a slot's records belong to
        z = np.zeros(N, np.int32)
        self.ctr = np.stack([z if turn0 is None else np.asarray(turn0, np.int32), z if episode0 is None else np.asarray(episode0, np.int32), z,
                             z if frozen0 is None else np.asarray(frozen0, np.int32)], 1)
        self.turn = 0
        self.status = 0

    def _shaped(self, reward, done, custom):
        if self.code == 5:
            return np.asarray(custom, np.float32).reshape(self.N).astype(np.float64)
        rw = np.asarray(reward, np.float32).astype(np.float64)
        turn, ep = self.ctr[:, 0], self.ctr[:, 1]
        mine, theirs = rw[:, self.seat], rw[:, 1 - self.seat]
        if self.code == 4:
            game = (self.episode_base + 1 + ep.astype(np.int64)).astype(np.float64)
            ratio = np.minimum(1.0, game / float(self.K))
            r1 = shape_base(self.fn_from, mine, theirs, done, turn) * (1.0 - ratio)
            r2 = shape_base(self.fn_to, mine, theirs, done, turn) * ratio
            return r1 + r2
        return shape_base(self.code, mine, theirs, done, turn)

    def record(self, rows, reward, done, custom=None):
        """rows [N, 7, 2] {unit, node} played this turn; reward [N, 2] f32; done [N]."""
        sl = self.slots
        t = self.turn
        slot, nxt = t % sl, (t + 1) % sl
        done = np.asarray(done).astype(bool)
        self.meta[nxt] = 0
        self.valid[nxt] = 0
        self.rows[slot] = np.asarray(rows, np.int32).reshape(self.N, 7, 2)
        self.turn_of[slot] = t
        c = self.ctr.copy()
        act = c[:, 3] == 0
        shaped = self._shaped(reward, done, custom)
        ok = actions_valid(self.rows[slot])
        self.rew[slot][act] = shaped[act]
        self.meta[slot][act] = np.stack([c[act, 0], c[act, 1], np.where(done[act], 0, F_NOT_DONE).astype(np.int32), np.zeros(act.sum(), np.int32)], -1)
        self.valid[slot][act] = ok[act]
        if (act & ~ok).any():
            self.status |= S_BAD_ACTION
        d, nd = act & done, act & ~done
        self.ctr[d] = np.stack([np.zeros(d.sum(), np.int32), c[d, 1] + 1, np.zeros(d.sum(), np.int32),
                                np.full(d.sum(), 0 if self.auto_reset else 1, np.int32)], 1)
        self.ctr[nd] = np.stack([c[nd, 0] + 1, c[nd, 1], c[nd, 2] + 1, np.zeros(nd.sum(), np.int32)], 1)
        self.turn += 1

    def size(self):
        return int(self.valid.sum(dtype=np.int64))

    def records(self):
        """Every valid record in the device's (slot, env) order: dict of arrays slot, env, action [., 7] int64, reward float64, not_done."""
        k, e = np.nonzero(self.valid)
        return dict(slot=k.astype(np.int32), env=e.astype(np.int32), action=unravel(self.rows[k, e]), reward=self.rew[k, e],
                    not_done=(self.meta[k, e, 2] & F_NOT_DONE) != 0)

    def handles(self):
        r = self.records()
        z = np.zeros_like(r["slot"])
        return np.stack([r["slot"], r["env"], z, z], 1).astype(np.int32)

    def push_order(self):
        """The valid records in the order the reference's memory.push saw them: by the caller's turn, then env."""
        r = self.records()
        order = np.lexsort((r["env"], self.turn_of[r["slot"]]))
        return {k: v[order] for k, v in r.items()}

    def draw(self, seed, call, batch, first=0):
        """The handles int32 [batch, 4] {slot, env, 0, 0} of sample(batch, seed) as call number `call` (draws first .. batch - 1 of them); all -1 for
        an empty memory."""
        h = self.handles()
        total = len(h)
        if total == 0:
            self.status |= S_EMPTY
            return np.full((int(batch) - first, 4), -1, np.int32)
        key = rng_spec._key(seed)
        call = int(call) & 0xFFFFFFFFFFFFFFFF
        t = [(rng_spec.philox4x32_10((i, call & rng_spec.MASK, call >> 32, DRAW_DOMAIN), key)[0] * total) >> 32 for i in range(first, int(batch))]
        return h[t]

    def gather(self, handles, obs_ring, terminal_next=False):
        """optimize_model's batch for handles [B, 4], from the ring's observations obs_ring [slots, N, 105] (any dtype): (state f32, action i64 [B, 7],
        next_state f32, reward f32, not_done bool).  A handle that names no valid record gives zeros (and S_BAD_HANDLE unless it is all -1)."""
        handles = np.asarray(handles, np.int32)
        B = len(handles)
        state, nxt = np.zeros((B, 105), np.float32), np.zeros((B, 105), np.float32)
        action, reward, nd = np.zeros((B, 7), np.int64), np.zeros(B, np.float32), np.zeros(B, bool)
        for i, (k, e, s, r) in enumerate(handles):
            ok = 0 <= k < self.slots and 0 <= e < self.N and s == 0 and r == 0 and self.valid[k, e] != 0
            if not ok:
                if not (k == e == s == r == -1):
                    self.status |= S_BAD_HANDLE
                continue
            state[i] = obs_ring[k, e].astype(np.float32)
            action[i] = unravel(self.rows[k, e])
            reward[i] = np.float32(self.rew[k, e])
            nd[i] = bool(self.meta[k, e, 2] & F_NOT_DONE)
            if nd[i] or terminal_next:
                nxt[i] = obs_ring[(k + 1) % self.slots, e].astype(np.float32)
        return state, action, nxt, reward, nd
