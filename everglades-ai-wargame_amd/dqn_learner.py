"""DqnFamilyLearner -- optimize_model of the reference's base family, agents/DQN, on the device: target forward -> policy forward -> top-7 TD head ->
backward -> grid-wide Adam, a chain of launches with no torch op between the batch tensors and the updated parameters (include/evg_dqn_learn.h,
libevg_dqnlearn.so).

    learner = env.dqn_learner(policy, target, lr=1e-4, gamma=0.99, mode="huber", clamp=1.0)
    loss = learner.step_on((state, action, next_state, reward, not_done))        # the policy's parameters updated in place; a 0-d device tensor
    loss, priorities = learner.step_on(batch, weights=w)
    loss = learner.step(mem, 128, seed=t)                                        # the batch drawn from a DqnReplay (env.dqn_replay)
    learner.sync_target()                                                        # target.load_state_dict(policy.state_dict())

What a step computes is agents/DQN/DQNAgent.py:220-290 (mode "huber": gather of the row's seven unravelled actions against target_net(next).topk(7)
* gamma + reward, smooth_l1_loss over the B x 7 pairs, every summed gradient clamped to [-clamp, clamp], one torch.optim.Adam step) or, with
mode="squared" and clamp=None, :294-337 (prioritized_optimize_model: ((q - expected) ** 2 * weights).mean(), priorities row mean + 1e-5).  not_done
may be None: optimize_model has no mask.  fresh_state=True starts every step from zero moments and step count.

The ownership rules are DqnLearner's: the networks stay the consumer's modules (or 4-tuples of tensors), parameters are read and updated in place,
whichever tensors the modules hold at the call; the learner owns the gradient buffers (the parameters' .grad is not touched), the moments m and v, the
control block ctl {int64 step, double beta1 ** step, double beta2 ** step} and the stage buffers of the last step, all attributes: q_pred, q_next, gq,
estimated, priorities, loss, grads.  Buffers are allocated at the first call with a given batch size; after that a step allocates nothing, runs no torch
op and does not synchronise; the chain is linear on one stream, so it can sit inside a captured torch.cuda.graph.  `lr` is read at every step.
"""
import ctypes as C

from . import _lib


def _torch():
    import torch
    return torch


def check_options(mode, clamp, lr, gamma, betas, eps):
    """The host-side argument checks of DqnFamilyLearner (no device, no torch) -> (mode id, clamp as the entry points take it)."""
    if mode not in _lib.DQN_TD_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(sorted(_lib.DQN_TD_MODES)), mode))
    if isinstance(clamp, bool) or (clamp is not None and not (isinstance(clamp, (int, float)) and 0.0 < float(clamp) < float("inf"))):
        raise ValueError("clamp must be None or a finite number > 0 (got %r)" % (clamp,))
    for name, value in (("lr", lr), ("gamma", gamma), ("eps", eps)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value or abs(value) == float("inf"):
            raise ValueError("%s must be a finite number (got %r)" % (name, value))
    if not eps > 0:
        raise ValueError("eps must be > 0 (got %r)" % (eps,))
    if len(betas) != 2 or not all(isinstance(b, (int, float)) and not isinstance(b, bool) and 0.0 <= b < 1.0 for b in betas):
        raise ValueError("betas must be two numbers in [0, 1) (got %r)" % (betas,))
    return _lib.DQN_TD_MODES[mode], 0.0 if clamp is None else float(clamp)


def check_batch_size(B):
    if not 1 <= B <= _lib.DQN_GRAD_MAX_ROWS:
        raise ValueError("the batch size must lie in 1..%d (got %d)" % (_lib.DQN_GRAD_MAX_ROWS, B))
    return B


class DqnFamilyLearner(object):
    def __init__(self, env, policy, target, lr=1e-4, gamma=0.99, mode="huber", clamp=1.0, fresh_state=False, betas=(0.9, 0.999), eps=1e-8,
                 final_relu=None):
        torch = _torch()
        self._mode, self.clamp = check_options(mode, clamp, lr, gamma, betas, eps)
        self.env, self.mode = env, mode
        self.G = _lib.load_dqn_learn()
        self.policy_net = env.dqn_qnet(policy, final_relu=final_relu)
        self.target_net = env.dqn_qnet(target, final_relu=final_relu)
        if self.target_net.h1 != self.policy_net.h1 or self.target_net.final_relu != self.policy_net.final_relu:
            raise ValueError("policy and target must be the same network shape (h1 %d / %d, final_relu %s / %s)" % (
                self.policy_net.h1, self.target_net.h1, self.policy_net.final_relu, self.target_net.final_relu))
        self.OUT, self.IN, self.h1 = self.policy_net.OUT, self.policy_net.IN, self.policy_net.h1
        self.lr, self.gamma, self.betas, self.eps = float(lr), float(gamma), (float(betas[0]), float(betas[1])), float(eps)
        self.fresh_state = bool(fresh_state)
        ts = self.policy_net._params()
        dev = env.device
        with torch.cuda.device(dev):
            self.grads = [torch.zeros_like(t, memory_format=torch.contiguous_format).detach() for t in ts]
            self.m = [torch.zeros_like(g) for g in self.grads]
            self.v = [torch.zeros_like(g) for g in self.grads]
            self.ctl = torch.zeros((4,), dtype=torch.int64, device=dev)               # EVG_ADAM_CTL_BYTES
            self.ctl.view(torch.float64)[1:3] = 1.0
            self.loss = torch.zeros((1,), dtype=torch.float32, device=dev)
            self._loss0 = self.loss.view(())
            self._td_ws = torch.empty((_lib.DQN_TD_WORKSPACE_BYTES // 4,), dtype=torch.float32, device=dev)
        self._bufs = {}
        self.q_pred = self.q_next = self.gq = self.estimated = self.priorities = None
        self._td = _lib.EvgDqnTdHeadArgs()
        self._td.struct_size = C.sizeof(self._td)
        self._adam = _lib.EvgAdamArgs()
        self._adam.struct_size = C.sizeof(self._adam)
        self._nd = _lib.EvgDqnNet()
        self._nd.struct_size = C.sizeof(self._nd)
        self._gs = _lib.EvgDqnGrads()
        self._gs.struct_size = C.sizeof(self._gs)
        self._gs.w1, self._gs.b1, self._gs.w2, self._gs.b2 = (g.data_ptr() for g in self.grads)

    # ------------------------------------------------------------------ buffers
    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            torch = _torch()
            dev = self.env.device
            with torch.cuda.device(dev):
                f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
                b = {"q_pred": f(B, self.OUT), "q_next": f(B, self.OUT), "gq": f(B, self.OUT), "estimated": f(B, _lib.DQN_TD_ACTIONS), "priorities": f(B),
                     "grad_ws": torch.empty((_lib.dqn_grad_workspace_bytes(B, self.h1) // 4,), dtype=torch.float32, device=dev)}
            self._bufs[B] = b
        self.q_pred, self.q_next, self.gq, self.estimated, self.priorities = b["q_pred"], b["q_next"], b["gq"], b["estimated"], b["priorities"]
        return b

    def _lcheck(self, rc):
        if rc:
            _lib.check(rc, self.G)

    # ------------------------------------------------------------------ the stages (each one entry point; the tests call them singly)
    def td_head(self, q_pred, action, q_next, reward, not_done, weights, gq, loss, priorities, estimated, mode=None, gamma=None):
        """evg_dqn_td_head on the given device tensors (None for an absent optional one)."""
        d = self._td
        d.mode = self._mode if mode is None else _lib.DQN_TD_MODES[mode]
        d.batch, d.gamma = int(action.shape[0]), self.gamma if gamma is None else gamma
        p = lambda t: None if t is None else t.data_ptr()
        d.q_pred, d.action, d.q_next, d.reward, d.not_done, d.weights = p(q_pred), p(action), p(q_next), p(reward), p(not_done), p(weights)
        d.gq, d.loss, d.priorities, d.estimated = p(gq), p(loss), p(priorities), p(estimated)
        d.workspace, d.workspace_bytes = self._td_ws.data_ptr(), self._td_ws.numel() * 4
        self._lcheck(self.G.evg_dqn_td_head(self.env._h, C.byref(d), self.env._stream()))

    def backward(self, x, q, gq, workspace=None):
        """evg_dqn_qnet_backward with the learner's clamp: the gradients of the policy's parameters, as they are now, into self.grads.  q: the policy
        forward's output for x (its signs are read with final_relu)."""
        ts = self.policy_net._params()
        rows = x.numel() // self.IN
        ws = self._buffers(rows)["grad_ws"] if workspace is None else workspace
        d = self._nd
        d.w1, d.b1, d.w2, d.b2 = (t.data_ptr() for t in ts)
        d.h1, d.final_relu, d.reserved = self.h1, int(self.policy_net.final_relu), 0
        self._lcheck(self.G.evg_dqn_qnet_backward(self.env._h, C.byref(d), rows, C.c_void_p(x.data_ptr()), C.c_void_p(q.data_ptr()),
                                                  C.c_void_p(gq.data_ptr()), C.byref(self._gs), C.c_void_p(ws.data_ptr()), ws.numel() * 4, self.clamp,
                                                  self.env._stream()))
        return ts

    def adam_step(self, params=None, grads=None, clamp=0.0):
        """evg_adam_step_wide over the policy's parameters (or `params`) with self.grads (or `grads`), self.m, self.v and self.ctl"""
        ts = self.policy_net._params() if params is None else params
        gs = self.grads if grads is None else grads
        a = self._adam
        a.n, a.lr, a.beta1, a.beta2, a.eps, a.clamp, a.fresh_state = len(ts), self.lr, self.betas[0], self.betas[1], self.eps, clamp, int(self.fresh_state)
        a.ctl = self.ctl.data_ptr()
        for i, (t, g, m, v) in enumerate(zip(ts, gs, self.m, self.v)):
            if tuple(g.shape) != tuple(t.shape):
                raise ValueError("the network's shapes changed: parameter %d is %s, its gradient buffer %s" % (i, tuple(t.shape), tuple(g.shape)))
            e = a.t[i]
            e.param, e.grad, e.m, e.v, e.count = t.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), t.numel()
        self._lcheck(self.G.evg_adam_step_wide(self.env._h, C.byref(a), self.env._stream()))

    # ------------------------------------------------------------------ a step
    def step_on(self, batch, weights=None):
        """One optimize_model on (state [B, 105] f32, action [B, 7] i64, next_state [B, 105] f32, reward [B] f32, not_done [B] bool or None).
        -> loss (0-d device tensor; the learner's own buffer, overwritten by the next step); with `weights` (float32 [B], the importance weights of a
        prioritized batch) -> (loss, priorities [B], the learner's buffer)."""
        torch = _torch()
        state, action, next_state, reward, not_done = batch
        if not isinstance(action, torch.Tensor) or action.dim() != 2:
            raise ValueError("action must be an int64 tensor [B, 7]")
        B = check_batch_size(int(action.shape[0]))
        u = self.env._user
        u(state, (B, self.IN), torch.float32, "state")
        u(action, (B, _lib.DQN_TD_ACTIONS), torch.int64, "action")
        u(next_state, (B, self.IN), torch.float32, "next_state")
        u(reward, (B,), torch.float32, "reward")
        if not_done is not None:
            u(not_done, (B,), torch.bool, "not_done")
        if weights is not None:
            u(weights, (B,), torch.float32, "weights")
        b = self._buffers(B)
        self.target_net.rows(next_state, out=b["q_next"])
        self.policy_net.rows(state, out=b["q_pred"])
        self.td_head(b["q_pred"], action, b["q_next"], reward, not_done, weights, b["gq"], self.loss, b["priorities"], b["estimated"])
        ts = self.backward(state, b["q_pred"], b["gq"], b["grad_ws"])
        self.adam_step(ts)
        return self._loss0 if weights is None else (self._loss0, b["priorities"])

    def step(self, mem, batch_size, seed, beta=None):
        """One optimize_model on `batch_size` transitions drawn from a DqnReplay (env.dqn_replay): mem.sample(batch_size, seed), then step_on with the
        memory's not_done (prioritized_optimize_model's (1 - done) rule; a terminal record's next_state is zeros).  With a PrioritizedDqnReplay and a
        `beta`: mem.sample(batch_size, seed, beta), step_on with its importance weights, then mem.update_priorities(handles, self.priorities) with the
        TD head's own priorities (duplicate handles keep the largest); beta=None draws uniformly from it (uniform_sample).  -> loss.  After the first
        call with a given batch size it allocates nothing, runs no torch op and does not synchronise; a captured step replays bit for bit when
        mem.sample_calls is set back to the value it had."""
        if beta is None:
            uniform = getattr(mem, "uniform_sample", None)
            return self.step_on((uniform or mem.sample)(batch_size, seed))
        if not hasattr(mem, "update_priorities"):
            raise ValueError("beta needs a prioritized memory (env.dqn_prioritized_replay)")
        out = mem.sample(batch_size, seed, beta)
        loss, priorities = self.step_on(out[:5], weights=out[5])
        mem.update_priorities(out[6], priorities)
        return loss

    # ------------------------------------------------------------------ the rest of an optimizer
    def sync_target(self):
        """target.load_state_dict(policy.state_dict()): the target's tensors overwritten in place"""
        torch = _torch()
        with torch.no_grad():
            for t, p in zip(self.target_net._params(), self.policy_net._params()):
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
