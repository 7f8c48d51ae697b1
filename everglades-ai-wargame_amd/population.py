"""QPopulation / SmartQPopulation -- self-royale: a per-env Q network drawn from a population each episode (include/evg.h, evg_population for the
Minimized 59-h1-11 network, evg_smart_population for the Smart_State 59-h1-h2-5 network; one surface, SmartQPopulation below).

The device form of agents/Minimized/training_scripts/dqn_self_royale.py: each seat has a team of networks, `random.choice(team)` picks the member that
plays an episode (:95-98), and only the members that played remember the game (:157-166) -- per ENV here: `member[e, p]` is the network of team p that
plays env e's current episode, redrawn when the episode ends.

    pop = env.q_population(team0, team1)                  # lists of whatever MinimizedQNet accepts; team1=None: team0 on both seats
    q = pop(shared, swarm, out=q)                         # [N, 2, 34], [N, 2, 12, 13] -> [N, 2, 12, 11]: row [e, p] through team p's member[e, p]
    env.step_q(q, eps, features=(shared, swarm), ...)     # the self-play turn, unchanged
    pop.end_of_turn(history=ring[slot])                   # behind the step: history, per-member tally, the draw for the envs that finished
    qt = pop.expanded(next_state_swarms, member, seat)    # the target networks on a sampled batch: [B, 12, 59], member [B] -> [B, 12, 11]

Every Q row equals, bit for bit, what MinimizedQNet writes for it with that member's weights.  The parameters are read in place on every call.  No
call synchronises with the host, and none allocates when `out` is given (expanded() keeps one id buffer per batch size).

The bucket pass's results stay readable after a forward of `rows` rows: `_bins[0 / 1, s]` are first / count of seat slot s's 17 bins, and slot s's stable
list begins at word `s * rows` of `_index`, with the rows of that call -- the layout follows the call (include/evg.h); `_index` is allocated as
[2, scratch_rows] only to bound it, and `_hist` is scratch.
"""
import ctypes as C

import numpy as np

from . import _lib
from .qnet import MinimizedQNet, SmartQNet


class QPopulation(object):
    OUT = _lib.MINI_QNET_OUT
    # what a population of another network family changes (SmartQPopulation): the evaluator of a member, the descriptor, its entry points' prefix,
    # the descriptor's weight tables in the order of the evaluator's _params(), and how the hidden sizes are named
    _NET, _DESC, _FN, _PARAMS, _SIZE_NAME = MinimizedQNet, _lib.EvgPopulation, "evg_population", ("w1", "b1", "w2", "b2"), "h1"

    @staticmethod
    def _size(net):
        """the hidden size(s) of a member's evaluator, as its _params() reports them"""
        return net.h1

    def _set_size(self, size, desc=None):
        self.h1 = size
        if desc is not None:
            desc.h1 = size

    def __init__(self, env, team0, team1=None, final_relu=None, max_rows=None):
        """team0 / team1: 1..16 members each (QNetwork modules, nn.Sequentials or 4-tuples of tensors with final_relu=...), all of one hidden size and
        one final_relu.  max_rows: the most rows a call evaluates (default 12 * num_envs: a batch of num_envs transitions in expanded()); the scratch
        grows on demand beyond it, which allocates.  The constructor ends with clear(): create it after env.reset()."""
        import torch
        self.env, self.L = env, env.L
        teams = [list(team0), list(team0 if team1 is None else team1)]
        for t in teams:
            if not 1 <= len(t) <= _lib.POP_MAX_MEMBERS:
                raise ValueError("a team has 1..%d members, got %d" % (_lib.POP_MAX_MEMBERS, len(t)))
        self.nets = [[self._NET(env, n, final_relu=final_relu) for n in t] for t in teams]
        flat = [n for t in self.nets for n in t]
        if any(n.pair for n in flat):
            raise ValueError("a member is one network, not a pair")
        if len({self._size(n) for n in flat}) != 1 or len({n.final_relu for n in flat}) != 1:
            raise ValueError("all members share the hidden size and the final ReLU (got %s %s, final_relu %s)" % (
                self._SIZE_NAME, sorted({self._size(n) for n in flat}), sorted({n.final_relu for n in flat})))
        self._hidden, self.final_relu = self._size(flat[0]), flat[0].final_relu
        self._set_size(self._hidden)
        self.num_members = (len(teams[0]), len(teams[1]))
        N = env.num_envs
        with torch.cuda.device(env.device):
            self.member = torch.zeros((N, 2), dtype=torch.uint8, device=env.device)              # the member of team p that plays env e
            self.counts = torch.zeros((2, 16, 4), dtype=torch.int64, device=env.device)          # games, wins, ties, losses, from the member's seat
            self._ctl = torch.zeros((2,), dtype=torch.int64, device=env.device)
            self._bins = torch.zeros((2, 2, _lib.POP_BINS), dtype=torch.int32, device=env.device)   # first, count
        d = self._DESC()
        d.struct_size = C.sizeof(self._DESC)
        self._set_size(self._hidden, d)
        d.final_relu = int(self.final_relu)
        d.num_members[0], d.num_members[1] = self.num_members
        d.member, d.counts, d.ctl = self.member.data_ptr(), self.counts.data_ptr(), self._ctl.data_ptr()
        d.first, d.count = self._bins[0].data_ptr(), self._bins[1].data_ptr()
        self._desc, self._ref = d, C.byref(d)
        self._ids = {}
        self._scratch(max(N, 12 * N) if max_rows is None else int(max_rows))
        self.clear()

    # ------------------------------------------------------------------ plumbing
    def _scratch(self, rows):
        import torch
        rows = max(int(rows), 1)
        with torch.cuda.device(self.env.device):
            self._index = torch.zeros((2, rows), dtype=torch.int32, device=self.env.device)
            self._hist = torch.zeros((2, _lib.POP_BINS, (rows + _lib.POP_BLOCK - 1) // _lib.POP_BLOCK), dtype=torch.int32, device=self.env.device)
        self._desc.index, self._desc.hist, self._desc.scratch_rows = self._index.data_ptr(), self._hist.data_ptr(), rows

    def reserve(self, rows):
        """scratch for forwards of up to `rows` rows.  -> the scratch tensors it replaced (a graph captured before the call still reads them: keep them
        while it lives), or None where the scratch was large enough"""
        if rows <= self._desc.scratch_rows:
            return None
        old = (self._index, self._hist)
        self._scratch(rows)
        return old

    def lists(self):
        """the bucket pass's results of the last forward for seat slot 0 (what expanded() uses): (index, first [17], count [17]), int32 views; member
        m's rows, ascending, are index[first[m] : first[m] + count[m]], bin 16 the rows of nobody.  `index` is replaced when the scratch grows."""
        return self._index, self._bins[0, 0], self._bins[1, 0]

    def _descriptor(self, rows):
        if not 1 <= rows <= _lib.POP_MAX_ROWS:
            raise ValueError("rows must lie in 1..2^24 (got %d)" % rows)
        if rows > self._desc.scratch_rows:
            self._scratch(rows)
        d = self._desc
        for p in range(2):
            for m, net in enumerate(self.nets[p]):
                ts, size = net._params(0)
                if size != self._hidden:
                    raise ValueError("the hidden size of member %d of team %d changed from %s to %s" % (m, p, self._hidden, size))
                for name, t in zip(self._PARAMS, ts):
                    getattr(d, name)[p][m] = t.data_ptr()
        return self._ref

    def _ids_of(self, member, lead, name="member"):
        """member ids for rows of shape `lead`: a uint8 tensor of that shape, or of lead[:-1] (one id per transition, repeated over its rows)"""
        import torch
        if not isinstance(member, torch.Tensor) or member.dtype != torch.uint8 or member.device != self.env.device:
            raise ValueError("%s must be a uint8 tensor on %s" % (name, self.env.device))
        if tuple(member.shape) == tuple(lead):
            if not member.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
            return member
        if len(lead) >= 2 and tuple(member.shape) == tuple(lead[:-1]):
            buf = self._ids.get(tuple(lead))
            if buf is None:
                buf = self._ids[tuple(lead)] = torch.empty(tuple(lead), dtype=torch.uint8, device=self.env.device)
            buf.copy_(member.unsqueeze(-1).expand(tuple(lead)))
            return buf
        raise ValueError("%s must have shape %s or %s, got %s" % (name, tuple(lead), tuple(lead[:-1]), tuple(member.shape)))

    def _out(self, out, shape):
        import torch
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.env.device)
        return self.nets[0][0]._input(out, shape, "out")

    def _launch(self, layout, rows, seat, member, in0, in1, out):
        ref = self._descriptor(rows)
        self.env._check(getattr(self.L, self._FN + "_qnet")(self.env._h, ref, layout, rows, int(seat), C.c_void_p(member.data_ptr()),
                                                            C.c_void_p(in0.data_ptr()), None if in1 is None else C.c_void_p(in1.data_ptr()),
                                                            C.c_void_p(out.data_ptr()), self.env._stream()))
        return out

    # ------------------------------------------------------------------ the forward
    def __call__(self, shared, swarm, out=None):
        """Both seats' Q of every env from the compact features: shared [N, 2, 34], swarm [N, 2, 12, 13] -> [N, 2, 12, 11], row [e, p] through member
        self.member[e, p] of team p (what step_q takes)."""
        N = self.env.num_envs
        chk = self.nets[0][0]._input
        chk(shared, (N, 2, 34), "shared")
        chk(swarm, (N, 2, 12, 13), "swarm")
        out = self._out(out, (N, 2, 12, self.OUT))
        return self._launch(_lib.QNET_COMPACT_SEATS, N, 0, self.member, shared, swarm, out)

    def seat(self, shared, swarm, member, seat, out=None):
        """One seat's compact features: shared [R, 34], swarm [R, 12, 13], member uint8 [R] -> [R, 12, 11], row r through member[r] of team `seat`."""
        chk = self.nets[0][0]._input
        if int(seat) not in (0, 1):
            raise ValueError("seat must be 0 or 1")
        R = shared.shape[0] if hasattr(shared, "shape") and len(shared.shape) == 2 else -1
        chk(shared, (R, 34), "shared")
        chk(swarm, (R, 12, 13), "swarm")
        member = self._ids_of(member, (R,))
        out = self._out(out, (R, 12, self.OUT))
        return self._launch(_lib.QNET_COMPACT, R, seat, member, shared, swarm, out)

    def expanded(self, x, member, seat, out=None):
        """Expanded rows: x [..., 59] -> [..., 11], every row through its member of team `seat` (the target networks on SmartReplay.sample's
        next_state_swarms [B, 12, 59]).  member: uint8 of x's leading shape, or without its last axis -- [B]: a transition's member for its 12 rows."""
        import torch
        if int(seat) not in (0, 1):
            raise ValueError("seat must be 0 or 1")
        if not isinstance(x, torch.Tensor) or x.dim() < 2 or x.shape[-1] != 59:
            raise ValueError("x must be a float32 tensor [..., 59]")
        self.nets[0][0]._input(x, tuple(x.shape), "x")
        lead = tuple(x.shape[:-1])
        member = self._ids_of(member, lead)
        out = self._out(out, lead + (self.OUT,))
        return self._launch(_lib.QNET_EXPANDED, x.numel() // 59, seat, member, x, None, out)

    # ------------------------------------------------------------------ the assignment
    def clear(self):
        """Counters and status zeroed; both seats' members of every env drawn for the env's current episode.  Enqueued on the current stream."""
        self.env._check(getattr(self.L, self._FN + "_clear")(self.env._h, self._ref, self.env._stream()))

    def _assign(self, mask, winner, history):
        import torch
        env, N = self.env, self.env.num_envs
        if mask is not None:
            if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.device == env.device):
                mask = torch.as_tensor(mask, device=env.device).to(torch.uint8).contiguous()
            if tuple(mask.shape) != (N,):
                raise ValueError("mask must have one entry per env")
        if winner is not None:
            env._user(winner, (N,), torch.int8, "winner")
        if history is not None:
            env._user(history, (N, 2), torch.uint8, "history")
        env._check(getattr(self.L, self._FN + "_assign")(env._h, self._ref, env._ptr(mask), env._ptr(winner), env._ptr(history), env._stream()))

    def end_of_turn(self, done=None, winner=None, history=None):
        """Behind a step: for the envs of `done` (default: the env's own done buffer) -- `history` uint8 [N, 2], if given, receives the members that
        played the finished episode; `winner` (default: the env's own winner buffer) is tallied for both seats' members; both are redrawn for the
        episode that begins.  With auto_reset the step has already started that episode; without it, reset(done) first or use assign_after_reset()."""
        self._assign(self.env.done if done is None else done, self.env.winner if winner is None else winner, history)

    def assign_after_reset(self, mask=None):
        """After an explicit env.reset(mask): draw the members of the envs of `mask` (None = all) for their new episode; nothing is tallied."""
        self._assign(mask, None, None)

    # ------------------------------------------------------------------ results
    @property
    def rows_per_member(self):
        """int32 [2, 16] (a view): how many rows of the LAST forward went through each member of seat slot 0 / 1 (one-seat forwards fill slot 0)."""
        return self._bins[1, :, :_lib.POP_MAX_MEMBERS]

    def status(self):
        """The sticky status bits (_lib.POP_S_BAD_MEMBER); synchronises."""
        return int(self._ctl[0].item())

    def check(self):
        """Raise EvgError if a status bit is set; synchronises."""
        st = self.status()
        if st:
            raise _lib.EvgError("population status %d: a member id was not below its team's size (its rows are zeros, its games untallied)" % st)

    def state(self):
        """The population's tensors as host arrays (np.savez-able); the networks are the caller's to save."""
        return dict(num_members=np.asarray(self.num_members, np.int32), member=self.member.cpu().numpy(), counts=self.counts.cpu().numpy(),
                    ctl=self._ctl.cpu().numpy())

    def load_state(self, st):
        """Restore state() onto a population created with the same team sizes (after env.restore())."""
        import torch
        if tuple(np.asarray(st["num_members"]).tolist()) != tuple(self.num_members):
            raise ValueError("load_state: the saved population has other team sizes")
        self.member.copy_(torch.as_tensor(np.asarray(st["member"], np.uint8)))
        self.counts.copy_(torch.as_tensor(np.asarray(st["counts"], np.int64)))
        self._ctl.copy_(torch.as_tensor(np.asarray(st["ctl"], np.int64)))


class SmartQPopulation(QPopulation):
    """Self-royale for the Smart_State agents (agents/Smart_State/training_scripts/dqn_smart_state_self_royale.py; include/evg.h,
    evg_smart_population): QPopulation's surface with members that are whatever SmartQNet accepts (59 -> h1 -> h2 -> 5, one (h1, h2) and one final_relu
    for all) and a head of 5 -- pop(shared, swarm) -> [N, 2, 12, 5] (what step_q takes), pop.seat(...) -> [R, 12, 5], pop.expanded(x, member, seat) ->
    [..., 5].  Every Q row equals, bit for bit, what SmartQNet writes for it with that member's weights.  The assignment is QPopulation's own -- the same
    kernels, the same draws: two populations with equal team sizes on one env hold the same members."""
    OUT = SmartQNet.OUT
    _NET, _DESC, _FN, _PARAMS, _SIZE_NAME = SmartQNet, _lib.EvgSmartPopulation, "evg_smart_population", ("w1", "b1", "w2", "b2", "w3", "b3"), "(h1, h2)"

    @staticmethod
    def _size(net):
        return (net.h1, net.h2)

    def _set_size(self, size, desc=None):
        self.h1, self.h2 = size
        if desc is not None:
            desc.h1, desc.h2 = size


class _Bf16Forward(object):
    """The grouped forward on the bf16 matrix cores (include/evg_pop_bf16.h, libevg_popbf16.so) in place of the fp32 launch: the one thing the two
    classes below change.  Assignment, clear, end_of_turn, lists(), state() and load_state() are the fp32 populations' own (libevg.so), so an fp32 and
    a bf16 population of equal team sizes on one env hold the same members.  A refused call's text is read from the library that refused it."""

    def _launch(self, layout, rows, seat, member, in0, in1, out):
        ref = self._descriptor(rows)
        B = _lib.load_popbf16()
        rc = getattr(B, self._FN + "_qnet_bf16")(self.env._h, ref, layout, rows, int(seat), C.c_void_p(member.data_ptr()), C.c_void_p(in0.data_ptr()),
                                                 None if in1 is None else C.c_void_p(in1.data_ptr()), C.c_void_p(out.data_ptr()), self.env._stream())
        if rc:
            _lib.check(rc, B)
        return out


class QPopulationBf16(_Bf16Forward, QPopulation):
    """QPopulation whose forwards run on the bf16 matrix cores (evg_population_qnet_bf16): the same four launches, the same published lists, bins and
    status.  Every Q row equals, bit for bit, what MinimizedQNetBf16 writes for it with that member's weights -- the numeric contract of
    include/evg_qnet_bf16.h per row, for the acting turn and for a team's target networks.  env.q_population(..., precision="bf16") makes one."""


class SmartQPopulationBf16(_Bf16Forward, SmartQPopulation):
    """SmartQPopulation on the bf16 matrix cores (evg_smart_population_qnet_bf16); see QPopulationBf16.  Every Q row equals, bit for bit, what
    SmartQNetBf16 writes for it with that member's weights.  env.smart_q_population(..., precision="bf16") makes one."""


def make(env, team0, team1, final_relu, max_rows, precision, fp32_cls, bf16_cls):
    """the population of env.q_population / env.smart_q_population for a precision: "fp32" (the bit-exact chain, the default) or "bf16" """
    if precision == "fp32":
        return fp32_cls(env, team0, team1, final_relu=final_relu, max_rows=max_rows)
    if precision == "bf16":
        return bf16_cls(env, team0, team1, final_relu=final_relu, max_rows=max_rows)
    raise ValueError('precision must be "fp32" or "bf16" (got %r)' % (precision,))
