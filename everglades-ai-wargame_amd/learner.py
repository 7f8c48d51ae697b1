"""DqnLearner -- optimize_model on the device: sample -> target forward -> policy forward -> TD head -> backward -> Adam, a chain of launches with no
torch op between the replay memory and the updated parameters (include/evg_learn.h, libevg_learn.so).

    learner = env.smart_learner(policy, target, mem, lr=1e-4, gamma=0.999, n_step=1, mode="max_mean", clamp=1.0)     # or env.minimized_learner(...)
    loss = learner.step(batch_size, seed)            # mem.sample -> ... -> the policy's parameters updated in place; a 0-d device tensor, no read-back
    loss = learner.step_on(batch)                    # the same from caller-supplied sample() / gather() tensors
    loss, priorities = learner.step_on(batch, weights=w)
    learner.sync_target()                            # target.load_state_dict(policy.state_dict())

What a step computes is agents/Smart_State/DQNAgent.py:336-385 (mode "max_mean": amax over actions, mean over swarms), the Blind agents' target
("max_max") or agents/Minimized_Rainbow/DQNAgent.py:279-327 ("double_mean": the policy network selects the next action, the target network values it):
smooth_l1_loss, every summed gradient clamped to [-clamp, clamp], one torch.optim.Adam step (weight_decay 0, no amsgrad).  fresh_state=True is the
reference's habit of constructing optim.Adam anew inside every optimize_model call: every step starts from zero moments and step count.

The networks stay the consumer's modules (or tuples of tensors): parameters are read and updated in place, whichever tensors the modules hold at the
call, so every SmartQNet / MinimizedQNet bound to them sees the step.  The learner owns the gradient buffers (the parameters' .grad is not touched), the
moments m and v, the control block ctl {int64 step, double beta1 ** step, double beta2 ** step} and the stage buffers of the last step, all attributes:
q_pred, q_next, q_select, gq, estimated, priorities, loss, grads.  Buffers are allocated at the first call with a given batch size; after that a step
allocates nothing, runs no torch op and does not synchronise, so it can sit inside a captured torch.cuda.graph.  `lr` is read at every step.
"""
import ctypes as C

from . import _lib


def _torch():
    import torch
    return torch


class DqnLearner(object):
    def __init__(self, env, kind, policy, target, mem, lr=1e-4, gamma=0.999, n_step=1, mode="max_mean", clamp=1.0, fresh_state=False,
                 target_precision="fp32", betas=(0.9, 0.999), eps=1e-8, beta=0.4, final_relu=None):
        torch = _torch()
        if kind not in ("smart", "minimized"):
            raise ValueError('kind must be "smart" or "minimized" (got %r)' % (kind,))
        if mode not in _lib.TD_MODES:
            raise ValueError("mode must be one of %s (got %r)" % (", ".join(sorted(_lib.TD_MODES)), mode))
        if isinstance(policy, (tuple, list)) and len(policy) == 2 or isinstance(target, (tuple, list)) and len(target) == 2:
            raise ValueError("a learner trains one network, not a pair")
        make = env.smart_qnet if kind == "smart" else env.minimized_qnet
        self.env, self.kind, self.mode, self.mem = env, kind, mode, mem
        self.G = _lib.load_learn()
        self.policy_net = make(policy, final_relu=final_relu)                     # fp32: the gradient is defined on the fp32 chain
        self.target_net = make(target, final_relu=final_relu, precision=target_precision)
        self.select_net = make(policy, final_relu=final_relu, precision=target_precision) if mode == "double_mean" else None
        self.OUT = self.policy_net.OUT
        n_step = int(n_step)
        if n_step < 1:
            raise ValueError("n_step must be >= 1")
        self.lr, self.gamma, self.n_step, self.betas, self.eps, self.beta = float(lr), float(gamma), n_step, (float(betas[0]), float(betas[1])), float(eps), float(beta)
        self.scale = self.gamma ** n_step
        self.clamp = 0.0 if clamp is None else float(clamp)
        self.fresh_state = bool(fresh_state)
        self.prioritized = hasattr(mem, "update_priorities")
        ts, _ = self.policy_net._params(0)
        dev = env.device
        with torch.cuda.device(dev):
            self.grads = [torch.zeros_like(t, memory_format=torch.contiguous_format).detach() for t in ts]
            self.m = [torch.zeros_like(g) for g in self.grads]
            self.v = [torch.zeros_like(g) for g in self.grads]
            self.ctl = torch.zeros((4,), dtype=torch.int64, device=dev)               # EVG_ADAM_CTL_BYTES
            self.ctl.view(torch.float64)[1:3] = 1.0
            self.loss = torch.zeros((1,), dtype=torch.float32, device=dev)
            self._loss0 = self.loss.view(())
            self._td_ws = torch.empty((_lib.TD_HEAD_WORKSPACE_BYTES // 4,), dtype=torch.float32, device=dev)
            self._grad_ws = torch.empty((_lib.QNET_GRAD_MAX_BLOCKS * self.policy_net._GRAD_PARTIAL,), dtype=torch.float32, device=dev)
        self._bufs = {}
        self.q_pred = self.q_next = self.q_select = self.gq = self.estimated = self.priorities = None
        self._td = _lib.EvgTdHeadArgs()
        self._td.struct_size = C.sizeof(self._td)
        self._adam = _lib.EvgAdamArgs()
        self._adam.struct_size = C.sizeof(self._adam)
        self._nd = type(self.policy_net._d)()                                         # the backward's network descriptor: one set
        self._nd.struct_size = C.sizeof(self._nd)
        self._gs = self.policy_net._GRAD_STRUCT()
        self._gs.struct_size = C.sizeof(self._gs)
        self._names = [n for n, _ in self._gs._fields_[2:]]
        for n, g in zip(self._names, self.grads):
            setattr(self._gs, n, g.data_ptr())
        self._backward = getattr(self.G, self.policy_net._GRAD_ENTRY)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            torch = _torch()
            dev = self.env.device
            with torch.cuda.device(dev):
                f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
                b = {"q_pred": f(B, self.OUT), "q_next": f(B, 12, self.OUT), "q_select": f(B, 12, self.OUT) if self.select_net is not None else None,
                     "gq": f(B, self.OUT), "estimated": f(B), "priorities": f(B)}
            self._bufs[B] = b
        self.q_pred, self.q_next, self.q_select = b["q_pred"], b["q_next"], b["q_select"]
        self.gq, self.estimated, self.priorities = b["gq"], b["estimated"], b["priorities"]
        return b

    def _lcheck(self, rc):
        if rc:
            _lib.check(rc, self.G)

    # ------------------------------------------------------------------ the stages (each one entry point; the tests call them singly)
    def td_head(self, q_pred, action, q_next, q_select, reward, not_done, weights, gq, loss, priorities, estimated, mode=None, scale=None):
        """evg_td_head on the given device tensors (None for an absent optional one)."""
        d = self._td
        B = int(action.shape[0])
        d.mode = _lib.TD_MODES[self.mode if mode is None else mode]
        d.batch, d.out, d.scale = B, int(q_pred.shape[-1]), self.scale if scale is None else scale
        p = lambda t: None if t is None else t.data_ptr()
        d.q_pred, d.action, d.q_next, d.q_select, d.reward, d.not_done, d.weights = p(q_pred), p(action), p(q_next), p(q_select), p(reward), p(not_done), p(weights)
        d.gq, d.loss, d.priorities, d.estimated = p(gq), p(loss), p(priorities), p(estimated)
        d.workspace, d.workspace_bytes = self._td_ws.data_ptr(), self._td_ws.numel() * 4
        self._lcheck(self.G.evg_td_head(self.env._h, C.byref(d), self.env._stream()))

    def backward(self, x, gq):
        """the family's backward entry point with the learner's clamp: the gradients of the policy's parameters, as they are now, into self.grads"""
        ts, hh = self.policy_net._params(0)
        d = self._nd
        for n, t in zip(self._names, ts):
            getattr(d, n)[0] = t.data_ptr()
        d.h1, d.final_relu, d.num_sets = ts[0].shape[0], int(self.policy_net.final_relu), 1
        if hasattr(d, "h2"):
            d.h2 = ts[2].shape[0]
        self._lcheck(self._backward(self.env._h, C.byref(d), x.numel() // 59, C.c_void_p(x.data_ptr()), C.c_void_p(gq.data_ptr()), C.byref(self._gs),
                                    C.c_void_p(self._grad_ws.data_ptr()), self._grad_ws.numel() * 4, self.clamp, self.env._stream()))
        return ts

    def adam_step(self, params=None, grads=None, clamp=0.0):
        """evg_adam_step over the policy's parameters (or `params`) with self.grads (or `grads`), self.m, self.v and self.ctl"""
        ts = self.policy_net._params(0)[0] if params is None else params
        gs = self.grads if grads is None else grads
        a = self._adam
        a.n, a.lr, a.beta1, a.beta2, a.eps, a.clamp, a.fresh_state = len(ts), self.lr, self.betas[0], self.betas[1], self.eps, clamp, int(self.fresh_state)
        a.ctl = self.ctl.data_ptr()
        for i, (t, g, m, v) in enumerate(zip(ts, gs, self.m, self.v)):
            if tuple(g.shape) != tuple(t.shape):
                raise ValueError("the network's shapes changed: parameter %d is %s, its gradient buffer %s" % (i, tuple(t.shape), tuple(g.shape)))
            e = a.t[i]
            e.param, e.grad, e.m, e.v, e.count = t.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), t.numel()
        self._lcheck(self.G.evg_adam_step(self.env._h, C.byref(a), self.env._stream()))

    # ------------------------------------------------------------------ a step
    def step_on(self, batch, weights=None):
        """One optimize_model on (swarm_obs [B, 59], action [B] i64, next_state_swarms [B, 12, 59], reward [B], not_done [B] bool) as SmartReplay.sample /
        gather return them.  -> loss (0-d device tensor; the learner's own buffer, overwritten by the next step); with `weights` (float32 [B], the
        importance weights of a prioritized batch) -> (loss, priorities [B] = |td| + 1e-5, the learner's buffer)."""
        torch = _torch()
        swarm_obs, action, next_state, reward, not_done = batch
        B = int(action.shape[0])
        if not 1 <= B <= _lib.TD_HEAD_MAX_BATCH:
            raise ValueError("the batch size must lie in 1..2^20 (got %d)" % B)
        u = self.env._user
        u(swarm_obs, (B, 59), torch.float32, "swarm_obs")
        u(action, (B,), torch.int64, "action")
        u(next_state, (B, 12, 59), torch.float32, "next_state_swarms")
        u(reward, (B,), torch.float32, "reward")
        u(not_done, (B,), torch.bool, "not_done")
        if weights is not None:
            u(weights, (B,), torch.float32, "weights")
        b = self._buffers(B)
        self.target_net.expanded(next_state, out=b["q_next"])
        if self.select_net is not None:
            self.select_net.expanded(next_state, out=b["q_select"])
        self.policy_net.expanded(swarm_obs, out=b["q_pred"])
        self.td_head(b["q_pred"], action, b["q_next"], b["q_select"], reward, not_done, weights, b["gq"], self.loss, b["priorities"], b["estimated"])
        ts = self.backward(swarm_obs, b["gq"])
        self.adam_step(ts)
        return self._loss0 if weights is None else (self._loss0, b["priorities"])

    def step(self, batch_size, seed):
        """mem.sample(batch_size, seed) -> step_on; for a prioritized memory the draw is by priority with beta=self.beta, the loss is weighted by the
        importance weights and |td| + 1e-5 goes back through update_priorities.  -> loss."""
        if self.prioritized:
            out = self.mem.sample(batch_size, seed, beta=self.beta)
            loss, priorities = self.step_on(out[:5], weights=out[5])
            self.mem.update_priorities(out[6], priorities)
            return loss
        return self.step_on(self.mem.sample(batch_size, seed))

    # ------------------------------------------------------------------ the rest of an optimizer
    def sync_target(self):
        """target.load_state_dict(policy.state_dict()): the target's tensors overwritten in place"""
        torch = _torch()
        with torch.no_grad():
            for t, p in zip(self.target_net._params(0)[0], self.policy_net._params(0)[0]):
                t.copy_(p)

    def state_dict(self):
        """Adam's state: copies of m, v and ctl, and the step count (a host integer: synchronises)"""
        return {"step": int(self.ctl[0].item()), "ctl": self.ctl.clone(), "m": [t.clone() for t in self.m], "v": [t.clone() for t in self.v]}

    def load_state_dict(self, sd):
        torch = _torch()
        if len(sd["m"]) != len(self.m) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(list(sd["m"]) + list(sd["v"]), self.m + self.v)):
            raise ValueError("the state's shapes are not this learner's")
        with torch.no_grad():
            self.ctl.copy_(sd["ctl"])
            for dst, src in zip(self.m + self.v, list(sd["m"]) + list(sd["v"])):
                dst.copy_(src)
