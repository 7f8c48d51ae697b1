"""DqnReplay -- the agents/DQN family's replay memory of RAW OBSERVATIONS on the device (include/evg_dqn_replay.h, libevg_dqnreplay.so).

Replaces, per env, what DQNAgent.remember_game_state, SimpleMemory.ReplayMemory and the batch assembly of optimize_model do
(agents/DQN/DQNAgent.py:199-337, SimpleMemory.py).  The step writes each observation straight into the ring, the network reads it there, and it is
stored once: `state` of record t and `next_state` of record t - 1.

    mem = env.dqn_replay(capacity_turns=8, shaping="reward_short_games", seat=0)
    env.observe_seat(0, out=mem.slot_obs(0))                                         # record 0's observation
    for t in range(turns):
        rows = env.dqn_get_action(qnet(mem.slot_obs(t)), eps, seat=0, out=mem.slot_actions(t))
        env.step_vs("random_actions", rows, seat=0, out=mem.slot_obs(t + 1))
        mem.record()                                                                 # record t
        loss = learner.step(mem, 128, seed=t)                                        # or: state, action, next_state, reward, not_done = mem.sample(128, seed=t)

Documented differences from the reference: the capacity is counted in TURNS of all envs; sample() draws WITH replacement; with auto_reset the slot
behind a finishing step holds the next episode's first observation, so a terminal record carries not_done = False and a next_state of zeros (without
auto_reset, sample(..., terminal_next=True) returns the terminal observation unmasked).  A record whose seven rows are not all unit 0..11 / node 0..10
is no transition: it is never drawn or gathered and sets DQN_REPLAY_S_BAD_ACTION in status().
"""
import ctypes as C

from . import _lib


def _torch():
    import torch
    return torch


_SHAPES = {name: i for i, name in enumerate(_lib.SHAPE_NAMES)}


def check_options(capacity_turns, shaping, seat):
    """The host-side argument checks of DqnReplay (no device, no torch) -> (H, shaping code, from, to, K, seat)."""
    H = int(capacity_turns)
    if H < 1:
        raise ValueError("capacity_turns must be >= 1 (got %r)" % (capacity_turns,))
    if seat not in (0, 1):
        raise ValueError("seat must be 0 or 1 (got %r)" % (seat,))
    fn_from = fn_to = K = 0
    if isinstance(shaping, (tuple, list)):
        if len(shaping) != 4 or shaping[0] != "transition" or shaping[1] not in _SHAPES or shaping[2] not in _SHAPES or int(shaping[3]) < 1:
            raise ValueError("shaping must be a name or ('transition', from, to, K >= 1)")
        code, fn_from, fn_to, K = _SHAPES["transition"], _SHAPES[shaping[1]], _SHAPES[shaping[2]], int(shaping[3])
        if max(fn_from, fn_to) > _SHAPES["reward_short_games"]:
            raise ValueError("transition shapes between two of normalized_score, basic_reward, penalize_long_games, reward_short_games")
    elif shaping in _SHAPES and shaping != "transition":
        code = _SHAPES[shaping]
    else:
        raise ValueError("shaping must be one of %s or ('transition', from, to, K)" % (_lib.SHAPE_NAMES,))
    return H, code, fn_from, fn_to, K, int(seat)


class DqnReplay(object):
    def __init__(self, env, capacity_turns, shaping="reward_short_games", seat=0, episode_base=0):
        """capacity_turns H: the turns kept (records t - H + 1 .. t after record t).  shaping: as SmartReplay takes it.  Allocates everything once."""
        torch = _torch()
        H, code, fn_from, fn_to, K, seat = check_options(capacity_turns, shaping, seat)
        self.env = env
        self.R = _lib.load_dqn_replay()
        N, dev = env.num_envs, env.device
        self.N, self.H, self.slots, self.seat, self.shaping = N, H, H + 1, seat, shaping
        slots = H + 1
        elem = torch.empty((), dtype=env.obs_dtype).element_size()
        ostride, astride = _lib.dqn_replay_obs_stride(N, elem), _lib.dqn_replay_act_stride(N)
        with torch.cuda.device(dev):
            self._obs = torch.zeros((slots, ostride), dtype=torch.uint8, device=dev)
            self._actions = torch.zeros((slots, astride), dtype=torch.int32, device=dev)
            self.rewards = torch.zeros((slots, N), dtype=torch.float64, device=dev)
            self.meta = torch.zeros((slots, N, 4), dtype=torch.int32, device=dev)               # {turn, episode, flags, 0}
            self.valid = torch.zeros((slots, N), dtype=torch.uint8, device=dev)
            self.env_state = torch.zeros((N, 4), dtype=torch.int32, device=dev)
            self._scan = torch.zeros((_lib.dqn_replay_scan_ints(slots, N),), dtype=torch.int32, device=dev)
            self.ctl = torch.zeros((4,), dtype=torch.int64, device=dev)
        self._slot_obs = [self._obs[k, :N * _lib.OBS_LEN * elem].view(env.obs_dtype).view(N, _lib.OBS_LEN) for k in range(slots)]
        self._slot_actions = [self._actions[k, :N * 14].view(N, 7, 2) for k in range(slots)]
        d = _lib.EvgDqnReplay()
        d.struct_size = C.sizeof(d)
        d.slots, d.seat, d.shaping, d.shaping_from, d.shaping_to, d.transition_episodes, d.reserved = slots, seat, code, fn_from, fn_to, K, 0
        d.episode_base = int(episode_base)
        for field, t in (("obs", self._obs), ("actions", self._actions), ("reward", self.rewards), ("meta", self.meta), ("valid", self.valid),
                         ("env_state", self.env_state), ("scan", self._scan), ("ctl", self.ctl)):
            setattr(d, field, t.data_ptr())
        self._d = d
        self._out = {}
        self.turn = 0
        self.clear()

    # ------------------------------------------------------------------ ring
    def _check(self, rc):
        if rc:
            _lib.check(rc, self.R)

    def slot(self, t):
        return int(t) % self.slots

    def slot_obs(self, t):
        """[N, 105] view, in the env's obs_dtype, of turn t's slot: `out=` of env.observe_seat for record 0 and of the step of turn t - 1, and what the
        network of turn t reads."""
        return self._slot_obs[self.slot(t)]

    def slot_actions(self, t):
        """int32 [N, 7, 2] view of turn t's slot: `out=` of env.dqn_get_action; the rows played are record t's action."""
        return self._slot_actions[self.slot(t)]

    def clear(self):
        """Empty the memory and take every env's turn / episode counters from the handle's state (as the stream reaches the call); turn restarts at 0."""
        self._check(self.R.evg_dqn_replay_clear(self.env._h, C.byref(self._d), self.env._stream()))
        self.turn = 0

    def record(self, reward=None, done=None, shaped=None):
        """Record turn `self.turn` after its step (reward [N, 2] f32 and done [N] u8 default to the env's own output buffers), then advance the turn.
        shaped: float32 [N] for shaping="custom"."""
        env = self.env
        reward = env.reward if reward is None else reward
        done = env.done if done is None else done
        torch = _torch()
        env._user(reward, (self.N, 2), torch.float32, "reward")
        env._user(done, (self.N,), torch.uint8, "done")
        custom = None
        if shaped is not None:
            custom = env._user(shaped, (self.N,), torch.float32, "shaped")
        rc = self.R.evg_dqn_replay_record(env._h, C.byref(self._d), self.turn, C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()),
                                          env._ptr(custom), env._stream())
        self._check(rc)
        self.turn += 1

    # ------------------------------------------------------------------ batches
    def _outputs(self, B):
        out = self._out.get(B)
        if out is None:
            torch = _torch()
            dev = self.env.device
            with torch.cuda.device(dev):
                out = (torch.empty((B, _lib.OBS_LEN), dtype=torch.float32, device=dev), torch.empty((B, 7), dtype=torch.int64, device=dev),
                       torch.empty((B, _lib.OBS_LEN), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                       torch.empty((B,), dtype=torch.bool, device=dev), torch.empty((B, 4), dtype=torch.int32, device=dev))
            self._out[B] = out
        return out

    def _flags(self, terminal_next):
        if terminal_next and self.env.auto_reset:
            raise ValueError("terminal_next=True needs an env without auto_reset: with it the slot behind a finishing step holds the next episode's "
                             "first observation, not the terminal one")
        return _lib.DQN_REPLAY_TERMINAL_NEXT if terminal_next else 0

    def sample(self, batch_size, seed, return_handles=False, terminal_next=False):
        """optimize_model's operands, in DqnFamilyLearner.step_on's order, for `batch_size` records drawn uniformly with replacement: (state [B, 105]
        f32, action [B, 7] i64 = unit * 11 + node, next_state [B, 105] f32 -- zeros where not_done is False, unless terminal_next --, reward [B] f32,
        not_done [B] bool) and, with return_handles, the drawn handles int32 [B, 4] {slot, env, 0, 0}.  Draw i keys Philox(seed, call index, i); the
        call index is `sample_calls` (a device counter the call advances).  The tensors are the memory's own per-B buffers, overwritten by the next
        call with the same B.  An empty memory gives zeros and sets REPLAY_S_EMPTY in status()."""
        B = int(batch_size)
        if not 1 <= B <= _lib.DQN_REPLAY_MAX_BATCH:
            raise ValueError("batch_size must lie in 1..%d (got %d)" % (_lib.DQN_REPLAY_MAX_BATCH, B))
        flags = self._flags(terminal_next)
        o = self._outputs(B)
        p = [C.c_void_p(t.data_ptr()) for t in o]
        rc = self.R.evg_dqn_replay_sample(self.env._h, C.byref(self._d), B, int(seed) & 0xFFFFFFFFFFFFFFFF, flags, p[0], p[1], p[2], p[3], p[4], p[5],
                                          self.env._stream())
        self._check(rc)
        return o if return_handles else o[:5]

    def gather(self, handles, terminal_next=False):
        """The outputs of sample() for caller-chosen handles int32 [B, 4] {slot, env, 0, 0} (deterministic).  A handle that names no valid record gives
        zeros and sets REPLAY_S_BAD_HANDLE in status()."""
        torch = _torch()
        if not isinstance(handles, torch.Tensor) or handles.dim() != 2 or handles.shape[1] != 4 or not 1 <= handles.shape[0] <= _lib.DQN_REPLAY_MAX_BATCH:
            raise ValueError("handles must be an int32 tensor [B, 4] with B in 1..%d" % _lib.DQN_REPLAY_MAX_BATCH)
        B = int(handles.shape[0])
        self.env._user(handles, (B, 4), torch.int32, "handles")
        if handles.data_ptr() % 16:
            raise ValueError("handles must be 16-byte aligned")
        flags = self._flags(terminal_next)
        o = self._outputs(B)
        p = [C.c_void_p(t.data_ptr()) for t in o[:5]]
        rc = self.R.evg_dqn_replay_gather(self.env._h, C.byref(self._d), B, C.c_void_p(handles.data_ptr()), flags, p[0], p[1], p[2], p[3], p[4],
                                          self.env._stream())
        self._check(rc)
        return o[:5]

    def size(self):
        """int64 0-d device tensor: the number of valid records in the memory (counted on the device; no host read-back)."""
        self._check(self.R.evg_dqn_replay_size(self.env._h, C.byref(self._d), self.env._stream()))
        return self.ctl[2]

    @property
    def sample_calls(self):
        """int64 0-d device tensor: the call index the next sample() uses (assign it to repeat a draw)."""
        return self.ctl[0]

    def status(self):
        """The memory's sticky status bits (REPLAY_S_EMPTY, REPLAY_S_BAD_HANDLE, DQN_REPLAY_S_BAD_PRIORITY, DQN_REPLAY_S_BAD_ACTION); synchronises."""
        return int(self.ctl[1].item())

    def check(self):
        """Raise EvgError if a sample met an empty memory, a gather a bad handle or a record out-of-range order rows since the last clear()."""
        st = self.status()
        if st:
            what = [w for bit, w in ((_lib.REPLAY_S_EMPTY, "a sample from an empty memory"),
                                     (_lib.REPLAY_S_BAD_HANDLE, "a gather of a handle that names no valid record"),
                                     (_lib.DQN_REPLAY_S_BAD_ACTION, "a record whose order rows are not all unit 0..11 / node 0..10")) if st & bit]
            raise _lib.EvgError("DQN replay memory status %d: %s" % (st, ", ".join(what)))


def check_alpha(alpha):
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:                                                         # (NaN fails both comparisons)
        raise ValueError("alpha must lie in [0, 1] (got %r)" % (alpha,))
    return alpha


def check_beta(beta):
    beta = float(beta)
    if not 0.0 <= beta < float("inf"):
        raise ValueError("beta must be finite and >= 0 (got %r)" % (beta,))
    return beta


class PrioritizedDqnReplay(DqnReplay):
    """DqnReplay that also samples by priority (agents/DQN/PrioritizedMemory.py: sample / update_priorities over the same ring).

        mem = env.dqn_prioritized_replay(capacity_turns=8, alpha=0.6, shaping="reward_short_games")
        state, action, next_state, reward, not_done, weights, handles = mem.sample(128, seed=t, beta=0.4)
        mem.update_priorities(handles, priorities)              # or: loss = learner.step(mem, 128, seed=t, beta=0.4), which does both

    One weight priority ** alpha per record (float32 [slots, N]) and a stamp of the record it belongs to (int32 [slots, N]); a stale stamp means
    "never updated", so record() does not touch them.  PrioritizedSmartReplay's three documented rules hold unchanged: a never-updated record weighs
    wmax AS OF THE DRAW; when one update names a record more than once the LARGEST priority is kept; probabilities are q / Q with integer weights
    quantised to 2^-32 of wmax and floored at one unit, so that a host model reproduces every draw bit for bit."""

    def __init__(self, env, capacity_turns, alpha=0.6, **kw):
        torch = _torch()
        self.alpha = check_alpha(alpha)
        self._p = None
        DqnReplay.__init__(self, env, capacity_turns, **kw)
        dev = env.device
        with torch.cuda.device(dev):
            self.weights = torch.zeros((self.slots, self.N), dtype=torch.float32, device=dev)
            self.stamps = torch.zeros((self.slots, self.N), dtype=torch.int32, device=dev)
            self._pscan = torch.zeros((_lib.dqn_replay_pscan_words(self.slots, self.N),), dtype=torch.int64, device=dev)
            self.pctl = torch.zeros((4,), dtype=torch.int64, device=dev)
        p = _lib.EvgDqnReplayPriority()
        p.struct_size = C.sizeof(p)
        p.alpha, p.weight, p.stamp, p.pscan, p.pctl = self.alpha, self.weights.data_ptr(), self.stamps.data_ptr(), self._pscan.data_ptr(), self.pctl.data_ptr()
        self._p = p
        self._wout = {}
        self.clear()

    @property
    def priorities(self):
        """float32 [slots, N] view of the stored weights priority ** alpha (0 = never updated; valid only where `stamps` is the record's stamp)."""
        return self.weights

    @property
    def wmax(self):
        """float32 0-d device tensor: the largest weight stored since the last clear() (what a never-updated record weighs)."""
        return self.pctl[:1].view(_torch().float32)[0]

    def clear(self):
        """DqnReplay.clear(), and the weights back to "never updated" with wmax = 1."""
        DqnReplay.clear(self)
        if self._p is not None:
            self._check(self.R.evg_dqn_replay_priority_clear(self.env._h, C.byref(self._d), C.byref(self._p), self.env._stream()))

    def sample(self, batch_size, seed, beta=0.4, terminal_next=False):
        """DqnReplay.sample's five tensors for records drawn by weight, with replacement, then weights float32 [B] -- (T q / Q) ** -beta over the
        batch's largest; beta = 0 gives exactly 1 -- and the drawn handles int32 [B, 4] to hand back to update_priorities.  Shares the call counter
        `sample_calls` with `uniform_sample`."""
        B = int(batch_size)
        if not 1 <= B <= _lib.DQN_REPLAY_MAX_BATCH:
            raise ValueError("batch_size must lie in 1..%d (got %d)" % (_lib.DQN_REPLAY_MAX_BATCH, B))
        beta = check_beta(beta)
        flags = self._flags(terminal_next)
        o = self._outputs(B)
        w = self._wout.get(B)
        if w is None:
            torch = _torch()
            with torch.cuda.device(self.env.device):
                w = self._wout[B] = torch.empty((B,), dtype=torch.float32, device=self.env.device)
        p = [C.c_void_p(t.data_ptr()) for t in o]
        rc = self.R.evg_dqn_replay_sample_prioritized(self.env._h, C.byref(self._d), C.byref(self._p), B, int(seed) & 0xFFFFFFFFFFFFFFFF, flags, beta,
                                                      p[0], p[1], p[2], p[3], p[4], p[5], C.c_void_p(w.data_ptr()), self.env._stream())
        self._check(rc)
        return o[:5] + (w, o[5])

    def uniform_sample(self, batch_size, seed, return_handles=False, terminal_next=False):
        """DqnReplay.sample: the uniform draw over the same memory."""
        return DqnReplay.sample(self, batch_size, seed, return_handles, terminal_next)

    def update_priorities(self, handles, priorities):
        """handles int32 [B, 4] as sample() returned them, priorities float32 [B] (> 0 and finite; the TD head's own).  A bad priority or handle is
        skipped and sets DQN_REPLAY_S_BAD_PRIORITY / REPLAY_S_BAD_HANDLE in status()."""
        torch = _torch()
        if not isinstance(handles, torch.Tensor) or handles.dim() != 2 or handles.shape[1] != 4 or not 1 <= handles.shape[0] <= _lib.DQN_REPLAY_MAX_BATCH:
            raise ValueError("handles must be an int32 tensor [B, 4] with B in 1..%d" % _lib.DQN_REPLAY_MAX_BATCH)
        B = int(handles.shape[0])
        self.env._user(handles, (B, 4), torch.int32, "handles")
        self.env._user(priorities, (B,), torch.float32, "priorities")
        if handles.data_ptr() % 16:
            raise ValueError("handles must be 16-byte aligned")
        rc = self.R.evg_dqn_replay_update_priorities(self.env._h, C.byref(self._d), C.byref(self._p), B, C.c_void_p(handles.data_ptr()),
                                                     C.c_void_p(priorities.data_ptr()), self.env._stream())
        self._check(rc)

    def check(self):
        """DqnReplay.check(), and a priority update that met a bad priority."""
        if self.status() & _lib.DQN_REPLAY_S_BAD_PRIORITY:
            raise _lib.EvgError("DQN replay memory status %d: a priority update got a priority that is NaN, infinite or <= 0" % self.status())
        DqnReplay.check(self)
