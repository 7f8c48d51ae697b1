"""PopulationLearner -- self-royale: one device learner step trains every member of one team from one sampled batch, each transition routed to the
member that played it (include/evg_pop_learn.h, libevg_poplearn.so).

    learner = env.smart_population_learner(policies, targets, lr=1e-4, gamma=0.999, n_step=1, mode="max_mean", clamp=1.0)   # or minimized_...
    loss = learner.step_on(batch, member)            # batch: the five tensors of SmartReplay.sample / gather; member: uint8 [B] on the device
    loss, priorities = learner.step_on(batch, member, weights=w)
    learner.sync_target()                            # every member's target.load_state_dict(policy.state_dict()); sync_target([0, 2]) for some

`policies` and `targets` are one team: lists of K networks (1 <= K <= 16) as smart_qnet() / minimized_qnet() take them, all of one hidden size and one
final_relu.  A learner serves one seat's team; a two-seat royale makes two learners and passes each the other seat's rows with an id >= K (255).

For member m let R_m be the rows with member[b] == m, ascending, and c_m their number.  Member m receives exactly one DqnLearner.step_on on the rows
R_m: the target from ITS target network, in "double_mean" the action chosen by its own policy, the Huber loss divided by c_m, gradients clamped to
[-clamp, clamp] after the sum, one Adam step on its own moments and control block.  A member with c_m = 0 gets loss[m] = 0 and zero gradients and takes
NO Adam step: its parameters, m, v and control block stay bit-identical (an agent that did not play does not call optimize_model).  A row whose id is
>= K belongs to nobody: a zero gq row, priority 0, in no loss, no gradient and no count.

A step is: the target population's grouped forward on next_state_swarms -> (double_mean: the selecting population's) -> the policy population's on
swarm_obs, whose bucket pass leaves the per-member lists the next three launches read -> evg_td_head_grouped -> evg_*population_backward ->
evg_adam_step_grouped.  The populations are private SmartQPopulation / QPopulation objects over the caller's modules: parameters are read and updated
in place, whichever tensors the modules hold at the call.  Their sticky "id names nobody" status bit is expected here and is no error of the learner.

The learner owns, all attributes: q_pred, q_next, q_select, gq, estimated, priorities, loss [K], counts [K] (int32: c_m of the last step, a view of the
policy population's bins), grads[m], m[m], v[m] (lists of the member's tensors) and ctl [K, 4] int64 (a 32-byte control block per member).  Buffers are
allocated at the first call with a given batch size; after that a step allocates nothing, runs no torch op and does not synchronise, so it can sit
inside a captured torch.cuda.graph.  `lr` is read at every step.  There is no step(batch_size, seed): the ring that records who played a transition is
the caller's, and a prioritized memory is served through weights= and the returned priorities.

target_precision="bf16_grouped" evaluates the target (and, in "double_mean", the selecting) networks on the bf16 matrix cores (include/evg_qnet_bf16.h)
with one grouped forward each (include/evg_pop_bf16.h): target_pop and select_pop are SmartQPopulationBf16 / QPopulationBf16, target_nets and
select_nets stay None, and a step has the launches of "fp32".  Every q_next row is bit-equal to the member's own bf16 evaluator.  Measured (DESIGN.md,
"Population forwards, bf16"): faster than "bf16" at every batch size; against "fp32" faster at B = 16 384 and not at B <= 1 024, where the target
forward sits on its fixed part.

target_precision="bf16" is the older form of the same numbers, without populations for the targets (target_pop and select_pop are None): each member's
SmartQNetBf16 / MinimizedQNetBf16 (target_nets, select_nets) evaluates the whole batch into one scratch buffer and evg_pop_learn_take_rows keeps that
member's rows -- 2 K launches in place of one grouped forward, K times the forward's arithmetic, q_next bit-identical to "bf16_grouped".  The policy
forward, the backward and Adam are fp32 whatever the setting.
"""
import ctypes as C

from . import _lib


def _torch():
    import torch
    return torch


def _hidden_of(net):
    """the hidden sizes of a network given as a module or as a tuple of tensors, from its weights' shapes alone (None if it cannot be told here)"""
    try:
        ts = list(net.parameters()) if hasattr(net, "parameters") else list(net)
        return tuple(int(t.shape[0]) for t in ts[0:len(ts) - 2:2])
    except Exception:
        return None


class PopulationLearner(object):
    def __init__(self, env, kind, policies, targets, lr=1e-4, gamma=0.999, n_step=1, mode="max_mean", clamp=1.0, fresh_state=False,
                 target_precision="fp32", betas=(0.9, 0.999), eps=1e-8, final_relu=None):
        torch = _torch()
        if kind not in ("smart", "minimized"):
            raise ValueError('kind must be "smart" or "minimized" (got %r)' % (kind,))
        if mode not in _lib.TD_MODES:
            raise ValueError("mode must be one of %s (got %r)" % (", ".join(sorted(_lib.TD_MODES)), mode))
        if target_precision not in ("fp32", "bf16", "bf16_grouped"):
            raise ValueError('target_precision must be "fp32" or "bf16" or "bf16_grouped" (got %r)' % (target_precision,))
        if not isinstance(policies, (list, tuple)) or not isinstance(targets, (list, tuple)):
            raise ValueError("policies and targets are lists of networks: one team")
        policies, targets = list(policies), list(targets)
        if not 1 <= len(policies) <= _lib.POP_MAX_MEMBERS or len(targets) != len(policies):
            raise ValueError("a team has 1..%d members and as many targets as policies (got %d policies, %d targets)" % (
                _lib.POP_MAX_MEMBERS, len(policies), len(targets)))
        tensors = 6 if kind == "smart" else 4
        for n in policies + targets:
            if isinstance(n, (tuple, list)) and len(n) == 2:
                raise ValueError("a member is one network, not a pair")
            if isinstance(n, (tuple, list)) and len(n) != tensors:
                raise ValueError("a member given as tensors is the %d tensors of its family (got %d)" % (tensors, len(n)))
        sizes = {_hidden_of(n) for n in policies + targets} - {None}
        if len(sizes) > 1:
            raise ValueError("all members share the hidden size (got %s)" % sorted(sizes))
        n_step = int(n_step)
        if n_step < 1:
            raise ValueError("n_step must be >= 1")
        from .population import QPopulation, QPopulationBf16, SmartQPopulation, SmartQPopulationBf16
        Pop = SmartQPopulation if kind == "smart" else QPopulation
        NextPop = Pop if target_precision == "fp32" else (SmartQPopulationBf16 if kind == "smart" else QPopulationBf16)
        self.env, self.kind, self.mode, self.K = env, kind, mode, len(policies)
        self.G = _lib.load_poplearn()
        self.policy_pop = Pop(env, policies, None, final_relu=final_relu, max_rows=1)
        self.target_precision = target_precision
        self.target_pop = self.select_pop = self.target_nets = self.select_nets = None
        if target_precision in ("fp32", "bf16_grouped"):                              # one grouped forward each, at that precision
            self.target_pop = NextPop(env, targets, None, final_relu=final_relu, max_rows=1)
            if mode == "double_mean":
                self.select_pop = NextPop(env, policies, None, final_relu=final_relu, max_rows=1)
            self._targets = self.target_pop.nets[0]
        else:                                                                         # one bf16 evaluator per member; take_rows merges them
            make = env.smart_qnet if kind == "smart" else env.minimized_qnet
            self.target_nets = self._targets = [make(n, final_relu=final_relu, precision="bf16") for n in targets]
            if mode == "double_mean":
                self.select_nets = [make(n, final_relu=final_relu, precision="bf16") for n in policies]
            for n in self.target_nets:
                if n._params(0)[1] != self.policy_pop._hidden or n.final_relu != self.policy_pop.final_relu:
                    raise ValueError("all members share the hidden size and the final ReLU (a target has %s, final_relu %s)" % (
                        n._params(0)[1], n.final_relu))
        self.OUT = self.policy_pop.OUT
        self.lr, self.gamma, self.n_step, self.betas, self.eps = float(lr), float(gamma), n_step, (float(betas[0]), float(betas[1])), float(eps)
        self.scale = self.gamma ** n_step
        self.clamp = 0.0 if clamp is None else float(clamp)
        self.fresh_state = bool(fresh_state)
        K, dev = self.K, env.device
        nets = self.policy_pop.nets[0]
        partial = _lib.SMART_QNET_GRAD_PARTIAL if kind == "smart" else _lib.MINI_QNET_GRAD_PARTIAL
        with torch.cuda.device(dev):
            self.grads = [[torch.zeros_like(t, memory_format=torch.contiguous_format).detach() for t in net._params(0)[0]] for net in nets]
            self.m = [[torch.zeros_like(g) for g in gs] for gs in self.grads]
            self.v = [[torch.zeros_like(g) for g in gs] for gs in self.grads]
            self.ctl = torch.zeros((K, 4), dtype=torch.int64, device=dev)                 # K blocks of EVG_ADAM_CTL_BYTES
            self.ctl.view(torch.float64)[:, 1:3] = 1.0
            self.loss = torch.zeros((K,), dtype=torch.float32, device=dev)
            self._td_ws = torch.empty((_lib.TD_HEAD_GROUPED_WORKSPACE_BYTES // 4,), dtype=torch.float32, device=dev)
            self._grad_ws = torch.empty((_lib.POP_LEARN_MAX_PARTIALS * partial,), dtype=torch.float32, device=dev)
        self._bufs, self._kept = {}, []
        self.q_pred = self.q_next = self.q_select = self.gq = self.estimated = self.priorities = None
        self._td = _lib.EvgTdHeadGroupedArgs()
        self._td.struct_size, self._td.td.struct_size = C.sizeof(self._td), C.sizeof(self._td.td)
        self._bw = _lib.EvgPopBackwardArgs()
        self._bw.struct_size = C.sizeof(self._bw)
        self._adam = _lib.EvgAdamGroupedArgs()
        self._adam.struct_size = C.sizeof(self._adam)
        self._backward = self.G.evg_smart_population_backward if kind == "smart" else self.G.evg_population_backward

    # ------------------------------------------------------------------ buffers
    @property
    def counts(self):
        """int32 [K] (a view): c_m of the last policy forward"""
        return self.policy_pop.lists()[2][:self.K]

    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            torch = _torch()
            dev = self.env.device
            for pop, rows in ((self.policy_pop, B), (self.target_pop, 12 * B), (self.select_pop, 12 * B)):
                old = pop.reserve(rows) if pop is not None else None
                if old is not None:
                    self._kept.append(old)                          # (a graph captured at a smaller batch keeps reading its own lists)
            with torch.cuda.device(dev):
                f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
                b = {"q_pred": f(B, self.OUT), "q_next": f(B, 12, self.OUT), "q_select": f(B, 12, self.OUT) if self.select_pop is not None else None,
                     "gq": f(B, self.OUT), "estimated": f(B), "priorities": f(B), "ids12": torch.zeros((B, 12), dtype=torch.uint8, device=dev),
                     "q_one": f(B, 12, self.OUT) if self.target_nets is not None else None}
                if self.select_nets is not None:
                    b["q_select"] = f(B, 12, self.OUT)
            self._bufs[B] = b
        self.q_pred, self.q_next, self.q_select = b["q_pred"], b["q_next"], b["q_select"]
        self.gq, self.estimated, self.priorities = b["gq"], b["estimated"], b["priorities"]
        return b

    def _lcheck(self, rc):
        if rc:
            _lib.check(rc, self.G)

    def _lists(self, l, B):
        l.index, l.first, l.count = (t.data_ptr() for t in self.policy_pop.lists())
        l.num_members, l.batch = self.K, B

    def _member_params(self):
        out = []
        for mb, net in enumerate(self.policy_pop.nets[0]):
            ts, size = net._params(0)
            if size != self.policy_pop._hidden:
                raise ValueError("the hidden size of member %d changed from %s to %s" % (mb, self.policy_pop._hidden, size))
            out.append(ts)
        return out

    # ------------------------------------------------------------------ the stages (each one entry point; the tests call them singly)
    def expand_ids(self, member, out):
        """evg_pop_learn_expand_ids: member uint8 [B] -> out uint8 [B, 12], a transition's id for each of its next-state rows"""
        self._lcheck(self.G.evg_pop_learn_expand_ids(self.env._h, C.c_void_p(member.data_ptr()), int(member.shape[0]), 12, C.c_void_p(out.data_ptr()),
                                                     self.env._stream()))
        return out

    def take_rows(self, src, ids, member, out):
        """evg_pop_learn_take_rows: out[r] = src[r] where ids[r] == member, zeros where ids[r] >= K, untouched elsewhere (src, out [..., OUT]; ids uint8)"""
        self._lcheck(self.G.evg_pop_learn_take_rows(self.env._h, C.c_void_p(src.data_ptr()), C.c_void_p(ids.data_ptr()), int(member), self.K,
                                                    int(ids.numel()), int(src.shape[-1]), C.c_void_p(out.data_ptr()), self.env._stream()))
        return out

    def next_forward(self, which, next_state, ids12, out, scratch=None):
        """q of the next-state rows through each row's own member of `which` ("target" or "select") at target_precision: one grouped forward ("fp32",
        "bf16_grouped"), or ("bf16") per member a whole-batch bf16 forward into `scratch` and take_rows"""
        pop, nets = (self.target_pop, self.target_nets) if which == "target" else (self.select_pop, self.select_nets)
        if pop is not None:
            return pop.expanded(next_state, ids12, 0, out=out)
        for mb, net in enumerate(nets):
            net.expanded(next_state, out=scratch)
            self.take_rows(scratch, ids12, mb, out)
        return out

    def policy_forward(self, swarm_obs, member, out):
        """the policy population's grouped forward; its bucket pass leaves the lists that td_head, backward and adam_step read"""
        return self.policy_pop.expanded(swarm_obs, member, 0, out=out)

    def td_head(self, q_pred, action, q_next, q_select, reward, not_done, weights, gq, loss, priorities, estimated, mode=None, scale=None):
        """evg_td_head_grouped on the given device tensors (None for an absent optional one), with the lists of the last policy_forward"""
        g = self._td
        d = g.td
        B = int(action.shape[0])
        d.mode = _lib.TD_MODES[self.mode if mode is None else mode]
        d.batch, d.out, d.scale = B, int(q_pred.shape[-1]), self.scale if scale is None else scale
        p = lambda t: None if t is None else t.data_ptr()
        d.q_pred, d.action, d.q_next, d.q_select, d.reward, d.not_done, d.weights = p(q_pred), p(action), p(q_next), p(q_select), p(reward), p(not_done), p(weights)
        d.gq, d.loss, d.priorities, d.estimated = p(gq), p(loss), p(priorities), p(estimated)
        d.workspace, d.workspace_bytes = self._td_ws.data_ptr(), self._td_ws.numel() * 4
        self._lists(g.lists, B)
        self._lcheck(self.G.evg_td_head_grouped(self.env._h, C.byref(g), self.env._stream()))

    def backward(self, x, gq):
        """the family's grouped backward with the learner's clamp: every member's gradients, from its rows of the last policy_forward, into self.grads"""
        params = self._member_params()
        a = self._bw
        B = x.numel() // 59
        hidden = self.policy_pop._hidden
        a.h1, a.h2 = (hidden if self.kind == "smart" else (hidden, 0))
        a.final_relu, a.clamp = int(self.policy_pop.final_relu), self.clamp
        self._lists(a.lists, B)
        a.x, a.gq = x.data_ptr(), gq.data_ptr()
        for mb, (ts, gs) in enumerate(zip(params, self.grads)):
            for i, (t, g) in enumerate(zip(ts, gs)):
                a.param[i][mb], a.grad[i][mb] = t.data_ptr(), g.data_ptr()
        a.workspace, a.workspace_bytes = self._grad_ws.data_ptr(), self._grad_ws.numel() * 4
        self._lcheck(self._backward(self.env._h, C.byref(a), self.env._stream()))
        return params

    def adam_step(self, params=None, grads=None, clamp=0.0, counts=None):
        """evg_adam_step_grouped over the members' parameters (or `params`) with self.grads (or `grads`), self.m, self.v and self.ctl; a member whose
        count (of the last policy_forward, or of `counts`, int32 [K]) is 0 is left alone"""
        params = self._member_params() if params is None else params
        grads = self.grads if grads is None else grads
        a = self._adam
        a.n, a.lr, a.beta1, a.beta2, a.eps, a.clamp, a.fresh_state = len(params[0]), self.lr, self.betas[0], self.betas[1], self.eps, clamp, int(self.fresh_state)
        a.num_members = self.K
        a.count = (self.counts if counts is None else counts).data_ptr()
        a.ctl = self.ctl.data_ptr()
        for mb in range(self.K):
            for i, (t, g, m, v) in enumerate(zip(params[mb], grads[mb], self.m[mb], self.v[mb])):
                if tuple(g.shape) != tuple(t.shape):
                    raise ValueError("the network's shapes changed: parameter %d of member %d is %s, its gradient buffer %s" % (
                        i, mb, tuple(t.shape), tuple(g.shape)))
                a.param[i][mb], a.grad[i][mb], a.m[i][mb], a.v[i][mb] = t.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                a.elements[i] = t.numel()
        self._lcheck(self.G.evg_adam_step_grouped(self.env._h, C.byref(a), self.env._stream()))

    # ------------------------------------------------------------------ a step
    def step_on(self, batch, member, weights=None):
        """One optimize_model per member on its rows of (swarm_obs [B, 59], action [B] i64, next_state_swarms [B, 12, 59], reward [B], not_done [B]
        bool) as SmartReplay.sample / gather return them; member uint8 [B]: who played each transition (>= K: nobody of this team).  -> loss, float32
        [K] (the learner's own buffer, overwritten by the next step); with `weights` (float32 [B]) -> (loss, priorities [B] = |td| + 1e-5; 0 for a
        row of nobody)."""
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
        u(member, (B,), torch.uint8, "member")
        if weights is not None:
            u(weights, (B,), torch.float32, "weights")
        b = self._buffers(B)
        ids12 = self.expand_ids(member, b["ids12"])
        self.next_forward("target", next_state, ids12, b["q_next"], b["q_one"])
        if self.mode == "double_mean":
            self.next_forward("select", next_state, ids12, b["q_select"], b["q_one"])
        self.policy_forward(swarm_obs, member, b["q_pred"])
        self.td_head(b["q_pred"], action, b["q_next"], b["q_select"], reward, not_done, weights, b["gq"], self.loss, b["priorities"], b["estimated"])
        params = self.backward(swarm_obs, b["gq"])
        self.adam_step(params)
        return self.loss if weights is None else (self.loss, b["priorities"])

    # ------------------------------------------------------------------ the rest of an optimizer
    def sync_target(self, members=None):
        """target.load_state_dict(policy.state_dict()) for every member (or those of `members`): the targets' tensors overwritten in place"""
        torch = _torch()
        with torch.no_grad():
            for mb in (range(self.K) if members is None else members):
                for t, p in zip(self._targets[mb]._params(0)[0], self.policy_pop.nets[0][mb]._params(0)[0]):
                    t.copy_(p)

    def state_dict(self):
        """Adam's state per member: copies of m, v and the control blocks, and the step counts (host integers: synchronises)"""
        return {"step": [int(s) for s in self.ctl[:, 0].tolist()], "ctl": self.ctl.clone(), "m": [[t.clone() for t in ts] for ts in self.m],
                "v": [[t.clone() for t in ts] for ts in self.v]}

    def load_state_dict(self, sd):
        torch = _torch()
        flat = lambda x: [t for ts in x for t in ts]
        if len(sd["m"]) != self.K or len(sd["v"]) != self.K or tuple(sd["ctl"].shape) != tuple(self.ctl.shape) or \
                any(tuple(a.shape) != tuple(b.shape) for a, b in zip(flat(sd["m"]) + flat(sd["v"]), flat(self.m) + flat(self.v))):
            raise ValueError("the state's shapes are not this learner's")
        with torch.no_grad():
            self.ctl.copy_(sd["ctl"])
            for dst, src in zip(flat(self.m) + flat(self.v), flat(sd["m"]) + flat(sd["v"])):
                dst.copy_(src)
