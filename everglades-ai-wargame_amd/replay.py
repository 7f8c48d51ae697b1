"""SmartReplay -- the Smart_State learner's n-step replay memory on the device (include/evg.h, evg_replay_*).

Replaces, per env, what every Smart_State training script of the reference runs after env.step (dqn_smart_state_training.py:127-135,
dqn_smart_state_self_play.py:130-160): reward_shaping.*, DQNAgent.remember_game_state -> NStepModule.trackGameState, end_of_episode ->
NStepModule.addGameToReplayMemory and the batch of optimize_model (agents/Smart_State/DQNAgent.py:312-385, Multi_Step.py).  Two documented differences:
the capacity is counted in TURNS of all envs (not in transitions: one turn of 65 536 envs already holds more than the reference's MEMORY_SIZE), and
sample() draws WITH replacement (random.sample draws without).

    mem = env.smart_replay(capacity_turns=8, n_step=1, gamma=0.999, shaping="reward_short_games", seats=0)
    env.smart_state_compact(-1, env.observe_seat(0), *mem.slot_features(0))          # record 0's features
    for t in range(turns):
        q = net(*mem.slot_features(t))
        env.step_vs_q("swarm", q, eps, features=mem.slot_features(t + 1), directions=mem.slot_directions(t))
        mem.record()                                                                   # record t
        swarm_obs, action, next_state_swarms, reward, not_done = mem.sample(1024, seed=t)
"""
import ctypes as C

from . import _lib


def _torch():
    import torch
    return torch


_SHAPES = {name: i for i, name in enumerate(_lib.SHAPE_NAMES)}


class SmartReplay(object):
    def __init__(self, env, capacity_turns, n_step=1, gamma=0.999, shaping="normalized_score", seats=0, episode_base=0):
        """capacity_turns H: the turns kept (records t - H + 1 .. t after record t); H > n_step.  seats: 0 or 1 -- the learner's seat of a step_vs_q loop,
        one record per env -- or (0, 1): both seats of a step_q loop.  shaping: one of "normalized_score", "basic_reward", "penalize_long_games",
        "reward_short_games" (utils/reward_shaping.py), ("transition", from, to, K) -- transition(from, to, K, i_episode) with i_episode = episode_base + 1
        + the env's episode index on the handle --, or "custom" (record(shaped=...) hands float32 [N] / [N, 2] rewards).  Allocates everything once."""
        torch = _torch()
        self.env, self.L = env, env.L
        N, dev = env.num_envs, env.device
        H, n = int(capacity_turns), int(n_step)
        if n < 1:
            raise ValueError("n_step must be >= 1")
        if H <= n:
            raise ValueError("capacity_turns (%d) must exceed n_step (%d): a record is sampled together with its record n turns later" % (H, n))
        if seats in (0, 1):
            S, seat = 1, int(seats)
        elif tuple(seats) == (0, 1):
            S, seat = 2, 0
        else:
            raise ValueError("seats must be 0, 1 (the learner of step_vs_q) or (0, 1) (both seats of step_q)")
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
        self.N, self.S, self.seats, self.H, self.slots, self.n_step, self.gamma = N, S, seats, H, H + 1, n, float(gamma)
        self.shaping = shaping
        slots, R = H + 1, (H + 1) * N * S
        sstride, dstride = (N * S * 34 + 3) // 4 * 4, (N * S * 14 + 3) // 4 * 4           # EVG_REPLAY_SHARED_STRIDE / _DIRS_STRIDE
        with torch.cuda.device(dev):
            self._shared = torch.zeros((slots, sstride), dtype=torch.float32, device=dev)
            self.swarm = torch.zeros((slots, N, S, 12, 13) if S == 2 else (slots, N, 12, 13), dtype=torch.float32, device=dev)
            self._dirs = torch.zeros((slots, dstride), dtype=torch.int32, device=dev)
            self.rewards = torch.zeros((slots, N, S, 2), dtype=torch.float64, device=dev)      # {shaped, n-step sum}
            self.meta = torch.zeros((slots, N, S, 4), dtype=torch.int32, device=dev)           # {turn, episode, flags, 0}
            self.counts = torch.zeros((slots, N, S), dtype=torch.uint8, device=dev)
            self.env_state = torch.zeros((N, 4), dtype=torch.int32, device=dev)
            # gamma ** k by Python's float power on the host (a device pow may differ in the last bit)
            self.gamma_pow = torch.tensor([self.gamma ** k for k in range(n)], dtype=torch.float64, device=dev)
            self._scan = torch.zeros(((R + 3) // 4 + (R + 1023) // 1024,), dtype=torch.int32, device=dev)
            self.ctl = torch.zeros((4,), dtype=torch.int64, device=dev)
        fshape = (N, 2) if S == 2 else (N,)
        self.shared = self._shared[:, :N * S * 34].view((slots,) + fshape + (34,))
        self.directions = self._dirs[:, :N * S * 14].view((slots,) + fshape + (7, 2))
        d = _lib.EvgReplay()
        d.slots, d.num_seats, d.seat, d.n_step, d.shaping = slots, S, seat, n, code
        d.shaping_from, d.shaping_to, d.transition_episodes, d.episode_base = fn_from, fn_to, K, int(episode_base)
        for field, t in (("shared", self._shared), ("swarm", self.swarm), ("directions", self._dirs), ("reward", self.rewards), ("meta", self.meta),
                         ("count", self.counts), ("env_state", self.env_state), ("gamma_pow", self.gamma_pow), ("scan", self._scan), ("ctl", self.ctl)):
            setattr(d, field, t.data_ptr())
        self._d = d
        self._out = {}
        self.turn = 0
        self.clear()

    # ------------------------------------------------------------------ ring
    def _check(self, rc):
        if rc:
            _lib.check(rc, self.L)

    def slot(self, t):
        return int(t) % self.slots

    def slot_features(self, t):
        """(shared, swarm) views of record t's slot -- [N, 34], [N, 12, 13] (or [N, 2, ...] for both seats) -- to pass as `features=` to the step of turn
        t - 1 (or to smart_state_compact for record 0)."""
        k = self.slot(t)
        return self.shared[k], self.swarm[k]

    def slot_directions(self, t):
        """int32 [N, 7, 2] (or [N, 2, 7, 2]) view of record t's slot: `directions=` of the step of turn t."""
        return self.directions[self.slot(t)]

    def clear(self):
        """Empty the memory and take every env's turn / episode counters from the handle's state (as the stream reaches the call); turn restarts at 0."""
        self._check(self.L.evg_replay_clear(self.env._h, C.byref(self._d), self.env._stream()))
        self.turn = 0

    def record(self, reward=None, done=None, shaped=None):
        """Record turn `self.turn` after its step (reward [N, 2] f32 and done [N] u8 default to the env's own output buffers), then advance the turn.
        shaped: float32 [N] (one seat) or [N, 2] (both seats) for shaping="custom"."""
        env = self.env
        reward = env.reward if reward is None else reward
        done = env.done if done is None else done
        torch = _torch()
        env._user(reward, (self.N, 2), torch.float32, "reward")
        env._user(done, (self.N,), torch.uint8, "done")
        custom = None
        if shaped is not None:
            custom = env._user(shaped, (self.N, 2) if self.S == 2 else (self.N,), torch.float32, "shaped")
        rc = self.L.evg_replay_record(env._h, C.byref(self._d), self.turn, C.c_void_p(reward.data_ptr()), C.c_void_p(done.data_ptr()),
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
                out = (torch.empty((B, 59), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int64, device=dev),
                       torch.empty((B, 12, 59), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float32, device=dev),
                       torch.empty((B,), dtype=torch.bool, device=dev), torch.empty((B, 4), dtype=torch.int32, device=dev))
            self._out[B] = out
        return out

    def sample(self, batch_size, seed, return_handles=False):
        """optimize_model's operands for `batch_size` transitions drawn uniformly with replacement: (swarm_obs [B, 59] f32, action [B] i64,
        next_state_swarms [B, 12, 59] f32 -- zeros where not_done is False --, reward [B] f32, not_done [B] bool) and, with return_handles, the drawn
        handles int32 [B, 4] {slot, env, seat, row}.  Draw i keys Philox(seed, call index, i); the call index is `sample_calls` (a device counter the call
        advances).  The tensors are the memory's own per-B buffers, overwritten by the next call with the same B.  An empty memory gives zeros and sets
        REPLAY_S_EMPTY in status()."""
        B = int(batch_size)
        if B < 1:
            raise ValueError("batch_size must be >= 1")
        o = self._outputs(B)
        p = [C.c_void_p(t.data_ptr()) for t in o]
        rc = self.L.evg_replay_sample(self.env._h, C.byref(self._d), B, int(seed) & 0xFFFFFFFFFFFFFFFF, p[0], p[1], p[2], p[3], p[4], p[5],
                                      self.env._stream())
        self._check(rc)
        return o if return_handles else o[:5]

    def gather(self, handles):
        """The outputs of sample() for caller-chosen handles int32 [B, 4] {slot, env, seat, row} (deterministic).  A handle that names no transition gives
        zeros and sets REPLAY_S_BAD_HANDLE in status()."""
        torch = _torch()
        if not isinstance(handles, torch.Tensor) or handles.dim() != 2 or handles.shape[1] != 4 or handles.shape[0] < 1:
            raise ValueError("handles must be an int32 tensor [B, 4] with B >= 1")
        B = int(handles.shape[0])
        self.env._user(handles, (B, 4), torch.int32, "handles")
        if handles.data_ptr() % 16:
            raise ValueError("handles must be 16-byte aligned")
        o = self._outputs(B)
        p = [C.c_void_p(t.data_ptr()) for t in o[:5]]
        rc = self.L.evg_replay_gather(self.env._h, C.byref(self._d), B, C.c_void_p(handles.data_ptr()), p[0], p[1], p[2], p[3], p[4], self.env._stream())
        self._check(rc)
        return o[:5]

    def size(self):
        """int64 0-d device tensor: the number of transitions in the memory (counted on the device; no host read-back)."""
        self._check(self.L.evg_replay_size(self.env._h, C.byref(self._d), self.env._stream()))
        return self.ctl[2]

    @property
    def sample_calls(self):
        """int64 0-d device tensor: the call index the next sample() uses (assign it to repeat a draw)."""
        return self.ctl[0]

    def status(self):
        """The memory's sticky status bits (REPLAY_S_EMPTY, REPLAY_S_BAD_HANDLE, REPLAY_S_BAD_PRIORITY); synchronises."""
        return int(self.ctl[1].item())

    def check(self):
        """Raise EvgError if a sample met an empty memory or a gather a bad handle since the last clear()."""
        st = self.status()
        if st:
            what = [w for bit, w in ((_lib.REPLAY_S_EMPTY, "a sample from an empty memory"), (_lib.REPLAY_S_BAD_HANDLE, "a gather of a handle that names "
                                                                                                                         "no transition")) if st & bit]
            raise _lib.EvgError("replay memory status %d: %s" % (st, ", ".join(what)))


class PrioritizedSmartReplay(SmartReplay):
    """SmartReplay that also samples by priority (agents/DQN/PrioritizedMemory.py: sample / update_priorities; include/evg_replay_priority.h, whose three
    entry points libevg_priority.so exports beside those of libevg.so: it is loaded here and takes the env's handle).

        mem = env.prioritized_replay(capacity_turns=8, alpha=0.6, n_step=1, shaping="reward_short_games")
        swarm_obs, action, next_state_swarms, reward, not_done, weights, handles = mem.sample(1024, seed=t, beta=0.4)
        mem.update_priorities(handles, td.abs() + 1e-5)

    The library stores the priorities handed back and draws by them; the TD error and the weighted loss are the consumer's.  Three documented differences
    from the reference class, next to the two of SmartReplay: (1) a transition that was never updated weighs wmax, the largest weight ever stored since
    the last clear(), AS OF THE DRAW (the reference fixes priorities.max() over the current values at push time); (2) when one update names a transition
    several times the LARGEST priority is kept (the reference's loop keeps the last); (3) probabilities are q / Q with integer weights quantised to 2^-32
    of the maximum and floored at one unit, so that a host model reproduces every draw bit for bit and nothing is undrawable."""

    def __init__(self, env, capacity_turns, alpha=0.6, **kw):
        torch = _torch()
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:                                                     # (NaN fails both comparisons)
            raise ValueError("alpha must lie in [0, 1] (got %r)" % (alpha,))
        self.alpha = alpha
        self._p = None
        self.P = _lib.load_priority()                                                   # libevg_priority.so: the three entry points used below
        SmartReplay.__init__(self, env, capacity_turns, **kw)
        dev, R = env.device, self.slots * self.N * self.S
        with torch.cuda.device(dev):
            self._plane = torch.zeros((self.slots, self.N, self.S, 8), dtype=torch.float32, device=dev)
            self._pscan = torch.zeros(((R + 3) // 4 + 2 * ((R + 1023) // 1024),), dtype=torch.int64, device=dev)      # EVG_REPLAY_PSCAN_WORDS
            self.pctl = torch.zeros((4,), dtype=torch.int64, device=dev)
        p = _lib.EvgReplayPriority()
        p.alpha, p.plane, p.pscan, p.pctl = alpha, self._plane.data_ptr(), self._pscan.data_ptr(), self.pctl.data_ptr()
        self._p = p
        self._wout = {}
        self.clear()

    def _pcheck(self, rc):
        if rc:
            _lib.check(rc, self.P)

    @property
    def priorities(self):
        """float32 [slots, N, S, 8] view of the plane: entries 0..6 the weights priority ** alpha of a record's transitions (0 = never updated), entry 7
        the record's stamp as int bits."""
        return self._plane

    @property
    def wmax(self):
        """float32 0-d device tensor: the largest weight stored since the last clear() (what a never-updated transition weighs)."""
        return self.pctl[:1].view(_torch().float32)[0]

    def clear(self):
        """SmartReplay.clear(), and the plane back to "never updated" with wmax = 1."""
        SmartReplay.clear(self)
        if self._p is not None:
            self._pcheck(self.P.evg_replay_priority_clear(self.env._h, C.byref(self._d), C.byref(self._p), self.env._stream()))

    def sample(self, batch_size, seed, beta=0.4):
        """SmartReplay.sample's five tensors for transitions drawn by weight, with replacement, then weights float32 [B] -- (T q / Q) ** -beta over the
        batch's largest -- and the drawn handles int32 [B, 4] to hand back to update_priorities.  Shares the call counter `sample_calls` with uniform
        samples (`uniform_sample`)."""
        B = int(batch_size)
        if B < 1:
            raise ValueError("batch_size must be >= 1")
        beta = float(beta)
        if not 0.0 <= beta < float("inf"):
            raise ValueError("beta must be finite and >= 0 (got %r)" % (beta,))
        o = self._outputs(B)
        w = self._wout.get(B)
        if w is None:
            torch = _torch()
            with torch.cuda.device(self.env.device):
                w = self._wout[B] = torch.empty((B,), dtype=torch.float32, device=self.env.device)
        p = [C.c_void_p(t.data_ptr()) for t in o]
        rc = self.P.evg_replay_sample_prioritized(self.env._h, C.byref(self._d), B, int(seed) & 0xFFFFFFFFFFFFFFFF, p[0], p[1], p[2], p[3], p[4], p[5],
                                                  C.byref(self._p), beta, C.c_void_p(w.data_ptr()), self.env._stream())
        self._pcheck(rc)
        return o[:5] + (w, o[5])

    def uniform_sample(self, batch_size, seed, return_handles=False):
        """SmartReplay.sample: the uniform draw over the same memory."""
        return SmartReplay.sample(self, batch_size, seed, return_handles)

    def update_priorities(self, handles, priorities):
        """handles int32 [B, 4] as sample() returned them, priorities float32 [B] (> 0 and finite; e.g. |td| + 1e-5).  A bad priority or handle is
        skipped and sets REPLAY_S_BAD_PRIORITY / REPLAY_S_BAD_HANDLE in status()."""
        torch = _torch()
        if not isinstance(handles, torch.Tensor) or handles.dim() != 2 or handles.shape[1] != 4 or handles.shape[0] < 1:
            raise ValueError("handles must be an int32 tensor [B, 4] with B >= 1")
        B = int(handles.shape[0])
        self.env._user(handles, (B, 4), torch.int32, "handles")
        self.env._user(priorities, (B,), torch.float32, "priorities")
        if handles.data_ptr() % 16:
            raise ValueError("handles must be 16-byte aligned")
        rc = self.P.evg_replay_update_priorities(self.env._h, C.byref(self._d), C.byref(self._p), B, C.c_void_p(handles.data_ptr()),
                                                 C.c_void_p(priorities.data_ptr()), self.env._stream())
        self._pcheck(rc)

    def check(self):
        """SmartReplay.check(), and a priority update that met a bad priority."""
        if self.status() & _lib.REPLAY_S_BAD_PRIORITY:
            raise _lib.EvgError("replay memory status %d: a priority update got a priority that is NaN, infinite or <= 0" % self.status())
        SmartReplay.check(self)
