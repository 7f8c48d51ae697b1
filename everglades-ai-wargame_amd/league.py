"""OpponentLeague -- a per-env scripted opponent, redrawn by weight each episode (include/evg.h, evg_league).

The device form of agents/Smart_State/training_scripts/dqn_smart_state_cycled_training_with_importance.py: every episode the opponent is
`random.choices(opposing_agents, opposing_agent_weights)[0]` from a list of scripted bots (:68-160, :210), games and wins are tallied per bot (:281-285)
and `updateAgentWeights` (:166-173) moves the weights towards the bots the learner loses to -- per ENV here, inside the step launch that ends the episode.
`resample=False` with a caller-written assignment is evaluate_all.py's shape: one learner against every bot at once, a win rate per bot.

The class owns the league's device tensors; `env.step_vs(league, ...)` / `env.step_vs_q(league, ...)` take it where they take a policy name.

One member may be "q": the caller's SECOND network instead of a bot (agents/Minimized/training_scripts/dqn_staggered_self_play.py, where seat 1 is drawn
once per episode from the second DQN or a scripted bot).  Such a league is played by `env.step_q(q [N, 2, 12, 11], ..., league=league)` only
(evg_step_league_minimized_q), which decodes that member's rows from q[:, 1 - seat].
"""
import ctypes as C

import numpy as np

from . import _lib


class OpponentLeague(object):
    def __init__(self, env, members, weights=None, seat=0, resample=True):
        """members: names from _lib.POLICY_NAMES (or their aliases) or EVG_POLICY_* ids, 1..16 of them; ids may repeat -- repeated ids are distinct
        members with their own agent objects and counters.  At most one member may be the string "q": the caller's second network (`q_member` is its
        index, -1 without one; the descriptor holds EVG_POLICY_NO_ACTION for it, a bot that is never consulted).  weights: one float per member (default 1.0 each).  seat: the CALLER's seat; the league plays
        1 - seat.  The constructor ends with clear(): create the league after env.reset(), or call assign_after_reset() after it."""
        import torch
        members = list(members)
        qs = [i for i, m in enumerate(members) if isinstance(m, str) and m == "q"]
        if len(qs) > 1:
            raise ValueError("a league has at most one \"q\" member (the caller's second network), got %d" % len(qs))
        self.q_member = qs[0] if qs else -1
        ids = [env.POLICIES["no_action"] if i == self.q_member else (env.POLICIES[m] if isinstance(m, str) else int(m)) for i, m in enumerate(members)]
        if not 1 <= len(ids) <= _lib.LEAGUE_MAX_MEMBERS:
            raise ValueError("a league has 1..%d members, got %d" % (_lib.LEAGUE_MAX_MEMBERS, len(ids)))
        if any(i < 0 or i >= len(_lib.POLICY_NAMES) for i in ids):
            raise ValueError("league members must be EVG_POLICY_* ids or names, got %r" % (list(members),))
        if int(seat) not in (0, 1):
            raise ValueError("seat must be 0 or 1")
        self.env, self.members, self.seat, self.resample = env, ids, int(seat), bool(resample)
        M, N = len(ids), env.num_envs
        w = np.ones(M, np.float64) if weights is None else np.asarray(weights, np.float64)
        if w.shape != (M,):
            raise ValueError("weights must have one entry per member")
        with torch.cuda.device(env.device):
            self.weights = torch.as_tensor(w, device=env.device).contiguous()                        # float64 [M], read when an episode starts
            self.assign = torch.zeros((N,), dtype=torch.uint8, device=env.device)                    # the member every env plays
            self.objects = torch.zeros((M, 3, N), dtype=torch.int32, device=env.device)              # uint32 words: the members' agent objects not live
            self.counts = torch.zeros((M, 4), dtype=torch.int64, device=env.device)                  # games, wins, ties, losses (the caller's seat's view)
            self._ctl = torch.zeros((2,), dtype=torch.int64, device=env.device)
        d = _lib.EvgLeague()
        d.num_members, d.seat, d.resample = M, self.seat, int(self.resample)
        for i, pid in enumerate(ids):
            d.members[i] = pid
        d.weights, d.assign, d.objects = self.weights.data_ptr(), self.assign.data_ptr(), self.objects.data_ptr()
        d.counts, d.ctl = self.counts.data_ptr(), self._ctl.data_ptr()
        self._desc = d
        self._ref = C.byref(d)
        self.clear()

    def clear(self):
        """Every member's object of every env fresh (as after scripted_reset), the env's live objects of the league seat too; counters and status zeroed;
        with resample every env's member drawn for its current episode.  Enqueued on the current stream."""
        self.env._check(self.env.L.evg_league_clear(self.env._h, self._ref, self.env._stream()))

    def assign_after_reset(self, mask=None):
        """After an explicit env.reset(mask): draw the member of the envs of `mask` (None = all) for their new episode and swap their agent objects.
        A no-op with resample=False."""
        import torch
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.env.device).to(torch.uint8).contiguous()
            if tuple(m.shape) != (self.env.num_envs,):
                raise ValueError("mask must have one entry per env")
        self.env._check(self.env.L.evg_league_assign(self.env._h, self._ref, self.env._ptr(m), self.env._stream()))

    def reweight(self, out=None):
        """updateAgentWeights on the device: 1.0 where games == 0, else 1.0 - wins / games + 0.05, into `out` (default: the league's own weights, which
        the next episode starts then read).  No host synchronisation."""
        import torch
        out = self.weights if out is None else self.env._user(out, (len(self.members),), torch.float64, "out")
        self.env._check(self.env.L.evg_league_importance(self.env._h, self._ref, self.env._ptr(out), self.env._stream()))
        return out

    def status(self):
        """The sticky status bits (_lib.LEAGUE_S_BAD_WEIGHTS, _lib.LEAGUE_S_BAD_ASSIGN); synchronises."""
        return int(self._ctl[0].item())

    def state(self):
        """The league's tensors as host arrays (np.savez-able).  The CURRENT members' objects are the env's live ones: save env.checkpoint() with it."""
        return dict(members=np.asarray(self.members, np.int32), seat=np.int32(self.seat), resample=np.int32(self.resample),
                    weights=self.weights.cpu().numpy(), assign=self.assign.cpu().numpy(), objects=self.objects.cpu().numpy().view(np.uint32),
                    counts=self.counts.cpu().numpy(), ctl=self._ctl.cpu().numpy())

    def load_state(self, st):
        """Restore state() onto a league created with the same members, seat and resample (after env.restore(), which restores the live objects)."""
        import torch
        if list(np.asarray(st["members"]).tolist()) != self.members or int(st["seat"]) != self.seat or bool(st["resample"]) != self.resample:
            raise ValueError("load_state: the saved league has other members, seat or resample")
        self.weights.copy_(torch.as_tensor(np.asarray(st["weights"], np.float64)))
        self.assign.copy_(torch.as_tensor(np.asarray(st["assign"], np.uint8)))
        self.objects.copy_(torch.as_tensor(np.ascontiguousarray(st["objects"], np.uint32).view(np.int32)))
        self.counts.copy_(torch.as_tensor(np.asarray(st["counts"], np.int64)))
        self._ctl.copy_(torch.as_tensor(np.asarray(st["ctl"], np.int64)))
