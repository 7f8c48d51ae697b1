"""The acting turn of the reference's base agent family, agents/DQN, on the device (include/evg_dqn.h, libevg_dqn.so).

    qnet = env.dqn_qnet(policy_net)                      # QNetwork(105, 132, seed) (fc1 / fc2, final ReLU), nn.Sequential(Linear(105, h), ReLU,
                                                         # Linear(h, 132)[, ReLU]), or a 4-tuple (w1, b1, w2, b2) with final_relu=...; h in 1..528
    q = qnet(obs_seat)                                   # the env's observation tensors: [N, 105], or [N, 2, 105] with seat=p -> [N, 132]
    q = qnet.rows(x)                                     # float32 [rows, 105] -> [rows, 132]: a target network's batch
    q = qnet.with_grad(x)                                # ... carrying autograd: loss(q.gather(1, a), y).backward() fills the parameters' .grad
    rows = env.dqn_get_action(q, eps, seat=0)            # epsilon_greedy: int32 [N, 7, 2] {unit, node 0..10}, what step_vs() takes as `actions`
    rows = env.dqn_actions(q)                            # filter_actions alone

DqnQNet is SmartQNet's contract for the 105-h-132 network: the fp32 parameters are read in place on every call (optimizer.step() and load_state_dict take
effect without rebinding), every pre-activation is the fmaf chain b[j], then k ascending (include/evg_dqn.h), the output is a plain tensor without
autograd, there is no host synchronisation, and nothing is allocated after the first call of a shape (or at all when `out` is given).  The observation
forms read the env's own dtype (float32, float64, int16) and convert on load as obs.float() does.  with_grad(x) is optimize_model's policy forward:
rows(x)'s values bit for bit, whose backward() is the device's backward pass (include/evg_dqn_grad.h, libevg_dqngrad.so).
"""
import ctypes as C

from . import _lib


def _torch():
    import torch
    return torch


def _linear_params(lin, name):
    torch = _torch()
    if not isinstance(lin, torch.nn.Linear) or lin.bias is None:
        raise ValueError("%s must be an nn.Linear with a bias" % name)
    return lin.weight, lin.bias


def _param_source(net, final_relu):
    """-> (a function returning the 4 tensors as they are now, final_relu)."""
    torch = _torch()
    if isinstance(net, (tuple, list)):
        if len(net) != 4 or not all(isinstance(t, torch.Tensor) for t in net):
            raise ValueError("a tuple of weights must be the 4 tensors (w1, b1, w2, b2), got %d item(s)" % len(net))
        if final_relu is None:
            raise ValueError("a tuple of weights needs final_relu=True or False")
        ts = tuple(net)
        return (lambda: ts), bool(final_relu)
    if isinstance(net, torch.nn.Sequential):
        mods = list(net)
        kinds = [type(m) for m in mods]
        lin, relu = torch.nn.Linear, torch.nn.ReLU
        if kinds[:3] != [lin, relu, lin] or not (len(mods) == 3 or (len(mods) == 4 and kinds[3] is relu)):
            raise ValueError("an nn.Sequential must be Linear, ReLU, Linear[, ReLU]")
        inferred = len(mods) == 4
        if final_relu is not None and bool(final_relu) != inferred:
            raise ValueError("final_relu=%s contradicts the Sequential (%s final ReLU)" % (final_relu, "with" if inferred else "without"))
        for i in (0, 2):
            _linear_params(mods[i], "layer %d" % i)
        return (lambda: (mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias)), inferred
    if all(hasattr(net, a) for a in ("fc1", "fc2")) and not hasattr(net, "fc3"):      # the reference's agents/DQN QNetwork: final ReLU on
        for a in ("fc1", "fc2"):
            _linear_params(getattr(net, a), a)
        return (lambda: (net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias)), True if final_relu is None else bool(final_relu)
    raise ValueError("net must be a QNetwork (fc1/fc2), an nn.Sequential of Linear/ReLU/Linear[/ReLU], or a 4-tuple of tensors")


def check_shapes(shapes):
    """The nn.Linear shapes of (w1, b1, w2, b2) -> h1; ValueError for anything that is no 105-h1-132 network with h1 in 1..528 (host only)."""
    w1, b1, w2, b2 = (tuple(s) for s in shapes)
    if len(w1) != 2 or w1[1] != _lib.DQN_IN or not 1 <= w1[0] <= _lib.DQN_MAX_HIDDEN:
        raise ValueError("w1 must be [h1, %d] with h1 in 1..%d, got %s" % (_lib.DQN_IN, _lib.DQN_MAX_HIDDEN, w1))
    h1 = w1[0]
    if w2 != (_lib.DQN_OUT, h1) or b1 != (h1,) or b2 != (_lib.DQN_OUT,):
        raise ValueError("w2 [%d, %d], b1 [%d], b2 [%d] expected, got %s %s %s" % (_lib.DQN_OUT, h1, h1, _lib.DQN_OUT, w2, b1, b2))
    return h1


class DqnQNet(object):
    """QNetwork(105 -> h1 -> 132) of agents/DQN on the device, one launch per call (evg_dqn_qnet)."""
    IN, OUT = _lib.DQN_IN, _lib.DQN_OUT

    def __init__(self, env, net, final_relu=None):
        self._src, self.final_relu = _param_source(net, final_relu)
        self.h1 = check_shapes([t.shape for t in self._src()])
        self.env = env
        self.D = _lib.load_dqn()
        self._d = _lib.EvgDqnNet()
        self._d.struct_size = C.sizeof(_lib.EvgDqnNet)
        self._outs = {}
        self._params()

    def _params(self):
        """The 4 tensors as they are now, checked: fp32, on the env's device, contiguous, 16-byte aligned, the shapes the evaluator was made for."""
        torch = _torch()
        ts = self._src()
        for t, n in zip(ts, ("w1", "b1", "w2", "b2")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.env.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float32 tensor on %s" % (n, self.env.device))
            if t.data_ptr() % 16:
                raise ValueError("%s must be 16-byte aligned" % n)
        h1 = check_shapes([t.shape for t in ts])
        if h1 != self.h1:
            raise ValueError("the network's hidden size changed from %d to %d" % (self.h1, h1))
        return ts

    def _out(self, rows, out):
        torch = _torch()
        if out is None:
            out = self._outs.get(rows)
            if out is None:
                out = self._outs[rows] = torch.empty((rows, self.OUT), dtype=torch.float32, device=self.env.device)
            return out
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.env.device or tuple(out.shape) != (rows, self.OUT) \
                or not out.is_contiguous() or out.data_ptr() % 16:
            raise ValueError("out must be a contiguous, 16-byte aligned float32 tensor of shape %s on %s" % ((rows, self.OUT), self.env.device))
        return out

    def _run(self, form, seat, rows, x, out):
        if not 1 <= rows <= _lib.QNET_MAX_ROWS:
            raise ValueError("rows must lie in 1..2^30 (got %d)" % rows)
        if x.data_ptr() % 16:
            raise ValueError("the input must be 16-byte aligned")
        out = self._out(rows, out)
        d = self._d
        d.w1, d.b1, d.w2, d.b2 = (t.data_ptr() for t in self._params())
        d.h1, d.final_relu, d.reserved = self.h1, int(self.final_relu), 0
        rc = self.D.evg_dqn_qnet(self.env._h, C.byref(d), form, seat, rows, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), self.env._stream())
        if rc:
            _lib.check(rc, self.D)
        return out

    def __call__(self, obs, seat=None, out=None):
        """Q from the env's observation tensors, in the env's obs_dtype: obs [N, 105] (what step_vs() returns; seat must be None), or obs [N, 2, 105]
        (env.obs) with seat = 0 or 1 -> float32 [N, 132].  Without `out` the result is the evaluator's own tensor for N rows, rewritten by the next call."""
        torch = _torch()
        env = self.env
        if not isinstance(obs, torch.Tensor) or obs.dim() not in (2, 3):
            raise ValueError("obs must be a tensor [N, 105] or [N, 2, 105]")
        N = obs.shape[0]
        if obs.dim() == 2:
            if seat is not None:
                raise ValueError("a one-seat observation [N, 105] takes no seat")
            env._user(obs, (N, self.IN), env.obs_dtype, "obs")
            return self._run(_lib.DQN_OBS_SEAT, 0, N, obs, out)
        if seat not in (0, 1):
            raise ValueError("a two-seat observation [N, 2, 105] needs seat=0 or 1")
        env._user(obs, (N, 2, self.IN), env.obs_dtype, "obs")
        return self._run(_lib.DQN_OBS, int(seat), N, obs, out)

    def rows(self, x, out=None):
        """Q of float32 rows x [rows, 105] -> [rows, 132]: a target network's batch of raw observations."""
        torch = _torch()
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError("x must be a float32 tensor [rows, 105]")
        self.env._user(x, (x.shape[0], self.IN), torch.float32, "x")
        return self._run(_lib.DQN_ROWS, 0, x.shape[0], x, out)


    # ---- the differentiable form (include/evg_dqn_grad.h, libevg_dqngrad.so)
    def with_grad(self, x, clamp=None):
        """rows(x) carrying autograd: x float32 [..., 105] -> a new tensor [..., 132], the same values bit for bit, whose backward() is the device's
        backward pass (evg_dqn_qnet_backward: the delta kernel, the weight-gradient kernel and, past 128 rows, the slices' reduction) and leaves the
        gradients of the network's parameters -- the tensors the module holds at this call -- in their .grad, as a torch forward would; x gets none.
        `clamp` (None, or c > 0) clamps every element of the gradients this call contributes to [-c, c].  At most 65 536 rows."""
        torch = _torch()
        if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != self.IN:
            raise ValueError("x must be a float32 tensor [..., %d]" % self.IN)
        if x.requires_grad:
            raise ValueError("with_grad() has no gradient with respect to x: x must not require grad")
        if isinstance(clamp, bool) or (clamp is not None and not (isinstance(clamp, (int, float)) and 0.0 < float(clamp) < float("inf"))):
            raise ValueError("clamp must be None or a finite number > 0 (got %r)" % (clamp,))
        self.env._user(x, tuple(x.shape), torch.float32, "x")
        rows = x.numel() // self.IN
        if not 1 <= rows <= _lib.DQN_GRAD_MAX_ROWS:
            raise ValueError("with_grad() takes 1..%d rows (got %d)" % (_lib.DQN_GRAD_MAX_ROWS, rows))
        if x.data_ptr() % 16:
            raise ValueError("the input must be 16-byte aligned")
        return _grad_function()(self, 0.0 if clamp is None else float(clamp), x, *self._params())

    def _backward(self, x, q, ts, gq, clamp):
        """the gradients of ts (the parameters saved by with_grad's forward) for the upstream gradient gq [..., 132]: new tensors of their shapes"""
        torch = _torch()
        G = _lib.load_dqn_grad()
        rows = x.numel() // self.IN
        gq = gq.to(torch.float32).contiguous()
        self.env._user(gq, tuple(x.shape[:-1]) + (self.OUT,), torch.float32, "the upstream gradient")
        if not hasattr(self, "_grad_ws"):
            self._grad_ws = {}
        ws = self._grad_ws.get(rows)
        if ws is None:                                                  # by rows, kept per row count
            ws = self._grad_ws[rows] = torch.empty(_lib.dqn_grad_workspace_bytes(rows, self.h1) // 4, dtype=torch.float32, device=self.env.device)
        d = _lib.EvgDqnNet()
        d.struct_size = C.sizeof(d)
        d.w1, d.b1, d.w2, d.b2 = (t.data_ptr() for t in ts)
        d.h1, d.final_relu, d.reserved = self.h1, int(self.final_relu), 0
        grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in ts]
        gs = _lib.EvgDqnGrads()
        gs.struct_size = C.sizeof(gs)
        gs.w1, gs.b1, gs.w2, gs.b2 = (g.data_ptr() for g in grads)
        rc = G.evg_dqn_qnet_backward(self.env._h, C.byref(d), rows, C.c_void_p(x.data_ptr()), C.c_void_p(q.data_ptr()), C.c_void_p(gq.data_ptr()),
                                     C.byref(gs), C.c_void_p(ws.data_ptr()), ws.numel() * 4, clamp, self.env._stream())
        if rc:
            _lib.check(rc, G)
        return grads


_GRAD_FN = []


def _grad_function():
    """the torch.autograd.Function behind with_grad (made on first use: importing this module does not import torch)"""
    if _GRAD_FN:
        return _GRAD_FN[0]
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class DqnQNetWithGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, net, clamp, x, *params):
            ctx.net, ctx.clamp = net, clamp
            rows = x.numel() // net.IN
            q = torch.empty((rows, net.OUT), dtype=torch.float32, device=x.device)      # the call's own tensor: the backward reads its signs
            net.rows(x.reshape(rows, net.IN), out=q)
            q = q.reshape(tuple(x.shape[:-1]) + (net.OUT,))
            ctx.save_for_backward(x, q, *params)
            return q

        @staticmethod
        @once_differentiable
        def backward(ctx, gq):
            x, q, params = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
            return (None, None, None) + tuple(ctx.net._backward(x, q, params, gq, ctx.clamp))

    _GRAD_FN.append(DqnQNetWithGrad.apply)
    return _GRAD_FN[0]


def _head_args(env, q, out, explored):
    torch = _torch()
    N = env.num_envs
    env._user(q, (N, _lib.DQN_OUT), torch.float32, "q")
    if out is None:
        env._seat_buffers()
        out = env._actions_seat
    env._user(out, (N, _lib.NUM_ACTIONS, 2), torch.int32, "out")
    if explored is not None:
        env._user(explored, (N,), torch.uint8, "explored")
    return out


def actions(env, q, out=None):
    """env.dqn_actions: DQNAgent.filter_actions for every env (evg_dqn_actions)."""
    D = _lib.load_dqn()
    out = _head_args(env, q, out, None)
    rc = D.evg_dqn_actions(env._h, C.c_void_p(q.data_ptr()), C.c_void_p(out.data_ptr()), env._stream())
    if rc:
        _lib.check(rc, D)
    return out


def get_action(env, q, epsilon, seat=0, out=None, explored=None):
    """env.dqn_get_action: DQNAgent.epsilon_greedy for every env (evg_dqn_get_action)."""
    torch = _torch()
    D = _lib.load_dqn()
    out = _head_args(env, q, out, explored)
    eps_env = None
    if isinstance(epsilon, torch.Tensor):
        eps_env = env._user(epsilon, (env.num_envs,), torch.float32, "epsilon")
        epsilon = 0.0
    rc = D.evg_dqn_get_action(env._h, C.c_void_p(q.data_ptr()), float(epsilon), env._ptr(eps_env), int(seat), C.c_void_p(out.data_ptr()),
                              env._ptr(explored), env._stream())
    if rc:
        _lib.check(rc, D)
    return out
