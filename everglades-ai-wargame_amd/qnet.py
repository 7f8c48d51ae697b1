"""SmartQNet -- the Smart_State Q network's forward pass on the device, one launch (include/evg.h, evg_smart_qnet).

An inference evaluator for the reference's QNetwork shape (agents/Smart_State/QNetwork.py: relu(fc3(relu(fc2(relu(fc1(x))))))), 59 -> h1 -> h2 -> 5 with
h1, h2 in 1..64.  The network stays the consumer's: the evaluator reads its fp32 parameters in place on every call, so optimizer.step() and
load_state_dict take effect without rebinding, and a module whose parameters were replaced (not updated in place) is followed too.  Training stays in
torch: the output of a call is a plain tensor without autograd, for the target network's forward and the acting turn's forward; optimize_model's
policy forward (whose gradient the loss needs) is a torch forward, or qnet.with_grad(x): the same values with the device's backward pass behind them
(include/evg_qnet_grad.h; the loss, the clamp of the summed gradients and the optimizer stay the consumer's).

    qnet = env.smart_qnet(policy_net)                     # QNetwork (final ReLU), nn.Sequential(Linear, ReLU, Linear, ReLU, Linear[, ReLU]),
                                                          # a 6-tuple (w1, b1, w2, b2, w3, b3) with final_relu=..., or a pair of these (two seats)
    q = qnet(shared, swarm)                               # [N, 34], [N, 12, 13] -> [N, 12, 5];  [N, 2, 34], [N, 2, 12, 13] -> [N, 2, 12, 5]
    q = qnet.expanded(x)                                  # [..., 59] -> [..., 5]
    q = qnet.with_grad(x)                                 # ... carrying autograd: loss(q.gather(1, a), y).backward() fills the parameters' .grad

Numerics: every pre-activation is the fmaf chain b[j], then k ascending (include/evg.h); the compact and the expanded forms of the same features give
equal Q.  No host synchronisation and no allocation when `out` is given: a call can sit inside a captured torch.cuda.graph.
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
    """-> (a function returning the 6 tensors as they are now, final_relu)."""
    torch = _torch()
    if isinstance(net, (tuple, list)) and len(net) == 6 and all(isinstance(t, torch.Tensor) for t in net):
        if final_relu is None:
            raise ValueError("a tuple of weights needs final_relu=True or False")
        ts = tuple(net)
        return (lambda: ts), bool(final_relu)
    if isinstance(net, torch.nn.Sequential):
        mods = list(net)
        kinds = [type(m) for m in mods]
        lin, relu = torch.nn.Linear, torch.nn.ReLU
        if kinds[:5] != [lin, relu, lin, relu, lin] or not (len(mods) == 5 or (len(mods) == 6 and kinds[5] is relu)):
            raise ValueError("an nn.Sequential must be Linear, ReLU, Linear, ReLU, Linear[, ReLU]")
        inferred = len(mods) == 6
        if final_relu is not None and bool(final_relu) != inferred:
            raise ValueError("final_relu=%s contradicts the Sequential (%s final ReLU)" % (final_relu, "with" if inferred else "without"))
        for i in (0, 2, 4):
            _linear_params(mods[i], "layer %d" % i)
        return (lambda: (mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, mods[4].weight, mods[4].bias)), inferred
    if all(hasattr(net, a) for a in ("fc1", "fc2", "fc3")):             # the reference's QNetwork: final ReLU on
        for a in ("fc1", "fc2", "fc3"):
            _linear_params(getattr(net, a), a)
        return (lambda: (net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias, net.fc3.weight, net.fc3.bias)), \
            True if final_relu is None else bool(final_relu)
    raise ValueError("net must be a QNetwork (fc1/fc2/fc3), an nn.Sequential of Linear/ReLU/Linear/ReLU/Linear[/ReLU], a 6-tuple of tensors, or a pair")


class SmartQNet(object):
    OUT = 5                                               # width of the head

    def __init__(self, env, net, final_relu=None):
        torch = _torch()
        self.env, self.L = env, env.L
        pair = isinstance(net, (tuple, list)) and len(net) == 2
        nets = list(net) if pair else [net]
        srcs = [_param_source(n, final_relu) for n in nets]
        if len({fr for _, fr in srcs}) != 1:
            raise ValueError("the two networks of a pair must agree on the final ReLU")
        self._srcs = [s for s, _ in srcs]
        self.pair = pair
        self.final_relu = srcs[0][1]
        shapes = [self._params(p)[1] for p in range(len(self._srcs))]
        if len(set(shapes)) != 1:
            raise ValueError("the two networks of a pair must have the same hidden sizes (got %s)" % (shapes,))
        self.h1, self.h2 = shapes[0]
        self._d = _lib.EvgQnet()
        self._d.struct_size = C.sizeof(_lib.EvgQnet)
        self._torch = torch

    def _params(self, p):
        """The 6 tensors of set p as they are now, checked: fp32, on the env's device, contiguous, 16-byte aligned, nn.Linear shapes."""
        torch = _torch()
        ts = self._srcs[p]()
        names = ("w1", "b1", "w2", "b2", "w3", "b3")
        for t, n in zip(ts, names):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.env.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float32 tensor on %s" % (n, self.env.device))
            if t.data_ptr() % 16:
                raise ValueError("%s must be 16-byte aligned" % n)
        w1, b1, w2, b2, w3, b3 = ts
        if w1.dim() != 2 or w1.shape[1] != 59 or not 1 <= w1.shape[0] <= _lib.QNET_MAX_HIDDEN:
            raise ValueError("w1 must be [h1, 59] with h1 in 1..64, got %s" % (tuple(w1.shape),))
        h1 = w1.shape[0]
        if w2.dim() != 2 or w2.shape[1] != h1 or not 1 <= w2.shape[0] <= _lib.QNET_MAX_HIDDEN:
            raise ValueError("w2 must be [h2, %d] with h2 in 1..64, got %s" % (h1, tuple(w2.shape)))
        h2 = w2.shape[0]
        if tuple(w3.shape) != (5, h2) or tuple(b1.shape) != (h1,) or tuple(b2.shape) != (h2,) or tuple(b3.shape) != (5,):
            raise ValueError("w3 [5, %d], b1 [%d], b2 [%d], b3 [5] expected, got %s %s %s %s" % (
                h2, h1, h2, tuple(w3.shape), tuple(b1.shape), tuple(b2.shape), tuple(b3.shape)))
        return ts, (h1, h2)

    def _descriptor(self, sets):
        d = self._d
        for p in range(2):
            ts, hh = self._params(p if self.pair else 0)
            if hh != (self.h1, self.h2):
                raise ValueError("the network's hidden sizes changed from %s to %s" % ((self.h1, self.h2), hh))
            d.w1[p], d.b1[p], d.w2[p], d.b2[p], d.w3[p], d.b3[p] = (t.data_ptr() for t in ts)
            if not self.pair:
                break
        if sets == 2 and not self.pair:               # the same set on both seats
            d.w1[1], d.b1[1], d.w2[1], d.b2[1], d.w3[1], d.b3[1] = d.w1[0], d.b1[0], d.w2[0], d.b2[0], d.w3[0], d.b3[0]
        d.h1, d.h2, d.final_relu, d.num_sets = self.h1, self.h2, int(self.final_relu), sets
        return d

    def _input(self, t, shape, name):
        torch = _torch()
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.env.device or tuple(t.shape) != tuple(shape) \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 tensor of shape %s on %s, got %s" % (
                name, tuple(shape), self.env.device, (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t)))
        if t.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned" % name)
        return t

    def _run(self, layout, sets, rows, in0, in1, out):
        if not 1 <= rows <= _lib.QNET_MAX_ROWS:
            raise ValueError("rows must lie in 1..2^30 (got %d)" % rows)
        d = self._descriptor(sets)
        self.env._check(self._launch(d, layout, rows, in0, in1, out))
        return out

    def _launch(self, d, layout, rows, in0, in1, out):
        return self.L.evg_smart_qnet(self.env._h, C.byref(d), layout, rows, C.c_void_p(in0.data_ptr()),
                                     None if in1 is None else C.c_void_p(in1.data_ptr()), C.c_void_p(out.data_ptr()), self.env._stream())

    def __call__(self, shared, swarm, out=None):
        """Q from the compact features: shared [N, 34] and swarm [N, 12, 13] -> [N, 12, 5] (one network), or shared [N, 2, 34] and swarm [N, 2, 12, 13]
        -> [N, 2, 12, 5] (seat p through network p of a pair, or through the one network)."""
        torch = _torch()
        if not isinstance(shared, torch.Tensor) or shared.dim() not in (2, 3):
            raise ValueError("shared must be a float32 tensor [N, 34] or [N, 2, 34]")
        seats = shared.dim() == 3
        if self.pair and not seats:
            raise ValueError("a pair of networks evaluates the two-seat layout: shared [N, 2, 34]")
        N = shared.shape[0]
        lead = (N, 2) if seats else (N,)
        self._input(shared, lead + (34,), "shared")
        self._input(swarm, lead + (12, 13), "swarm")
        if out is None:
            out = torch.empty(lead + (12, self.OUT), dtype=torch.float32, device=self.env.device)
        else:
            self._input(out, lead + (12, self.OUT), "out")
        layout = _lib.QNET_COMPACT_SEATS if seats else _lib.QNET_COMPACT
        return self._run(layout, 2 if seats else 1, N, shared, swarm, out)

    def expanded(self, x, out=None):
        """Q from expanded rows: x [..., 59] -> [..., 5] (smart_state() output [N, 12, 59], SmartReplay.sample's swarm_obs [B, 59] or
        next_state_swarms [B, 12, 59]).  One network only."""
        torch = _torch()
        if self.pair:
            raise ValueError("expanded() evaluates one network, not a pair")
        if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != 59:
            raise ValueError("x must be a float32 tensor [..., 59]")
        self._input(x, tuple(x.shape), "x")
        rows = x.numel() // 59
        shape = tuple(x.shape[:-1]) + (self.OUT,)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.env.device)
        else:
            self._input(out, shape, "out")
        return self._run(_lib.QNET_EXPANDED, 1, rows, x, None, out)

    # ---- the differentiable form (include/evg_qnet_grad.h, libevg_grad.so)
    _GRAD_ENTRY, _GRAD_STRUCT, _GRAD_PARTIAL = "evg_smart_qnet_backward", _lib.EvgQnetGrads, _lib.SMART_QNET_GRAD_PARTIAL

    def with_grad(self, x, clamp=None):
        """expanded(x) carrying autograd: x [..., 59] -> [..., OUT], the same values bit for bit, whose backward() is the device's backward pass
        (evg_smart_qnet_backward / evg_minimized_qnet_backward: two launches) and leaves the gradients of the network's parameters -- the tensors
        the module holds at this call -- in their .grad, as a torch forward would; x gets none.  `clamp` (None, or c > 0) clamps every element of
        the gradients this call contributes to [-c, c].  One network only; the fp32 classes only."""
        torch = _torch()
        if self.pair:
            raise ValueError("with_grad() differentiates one network, not a pair")
        if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != 59:
            raise ValueError("x must be a float32 tensor [..., 59]")
        if x.requires_grad:
            raise ValueError("with_grad() has no gradient with respect to x: x must not require grad")
        if clamp is not None and not (isinstance(clamp, (int, float)) and 0.0 < float(clamp) < float("inf")):
            raise ValueError("clamp must be None or a finite number > 0 (got %r)" % (clamp,))
        self._input(x, tuple(x.shape), "x")
        ts, _ = self._params(0)
        return _grad_function()(self, 0.0 if clamp is None else float(clamp), x, *ts)

    def _backward(self, x, ts, gq, clamp):
        """the gradients of ts (the parameters saved by with_grad's forward) for the upstream gradient gq [..., OUT]: new tensors of their shapes"""
        torch = _torch()
        G = _lib.load_grad()
        rows = x.numel() // 59
        gq = gq.to(torch.float32).contiguous()
        self._input(gq, tuple(x.shape[:-1]) + (self.OUT,), "the upstream gradient")
        if getattr(self, "_grad_ws", None) is None:                     # one partial per workgroup of the largest grid, allocated once
            self._grad_ws = torch.empty(_lib.QNET_GRAD_MAX_BLOCKS * self._GRAD_PARTIAL, dtype=torch.float32, device=self.env.device)
        d = type(self._d)()
        d.struct_size = C.sizeof(d)
        names = [n for n, _ in self._GRAD_STRUCT._fields_[2:]]
        grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in ts]
        gs = self._GRAD_STRUCT()
        gs.struct_size = C.sizeof(gs)
        for n, t, g in zip(names, ts, grads):
            getattr(d, n)[0] = t.data_ptr()
            setattr(gs, n, g.data_ptr())
        d.h1, d.final_relu, d.num_sets = ts[0].shape[0], int(self.final_relu), 1
        if hasattr(d, "h2"):
            d.h2 = ts[2].shape[0]
        rc = getattr(G, self._GRAD_ENTRY)(self.env._h, C.byref(d), rows, C.c_void_p(x.data_ptr()), C.c_void_p(gq.data_ptr()), C.byref(gs),
                                          C.c_void_p(self._grad_ws.data_ptr()), self._grad_ws.numel() * 4, clamp, self.env._stream())
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

    class QNetWithGrad(torch.autograd.Function):
        @staticmethod
        def forward(ctx, net, clamp, x, *params):
            ctx.net, ctx.clamp = net, clamp
            ctx.save_for_backward(x, *params)
            return net.expanded(x)

        @staticmethod
        @once_differentiable
        def backward(ctx, gq):
            x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
            return (None, None, None) + tuple(ctx.net._backward(x, params, gq, ctx.clamp))

    _GRAD_FN.append(QNetWithGrad.apply)
    return _GRAD_FN[0]


def _mini_param_source(net, final_relu):
    """-> (a function returning the 4 tensors as they are now, final_relu)."""
    torch = _torch()
    if isinstance(net, (tuple, list)) and len(net) == 4 and all(isinstance(t, torch.Tensor) for t in net):
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
    if all(hasattr(net, a) for a in ("fc1", "fc2")) and not hasattr(net, "fc3"):      # the reference's Minimized QNetwork: final ReLU on
        for a in ("fc1", "fc2"):
            _linear_params(getattr(net, a), a)
        return (lambda: (net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias)), True if final_relu is None else bool(final_relu)
    raise ValueError("net must be a Minimized QNetwork (fc1/fc2), an nn.Sequential of Linear/ReLU/Linear[/ReLU], a 4-tuple of tensors, or a pair")


class MinimizedQNet(SmartQNet):
    """The Minimized agents' Q network on the device, one launch (include/evg.h, evg_minimized_qnet): agents/Minimized/QNetwork.py,
    relu(fc2(relu(fc1(x)))), 59 -> h1 -> 11 with h1 in 1..128.  SmartQNet's contract -- parameters read in place on every call, the fmaf-chain numerics,
    no autograd, no host synchronisation -- and its calls: qnet(shared, swarm) -> [N, 12, 11] or [N, 2, 12, 11], qnet.expanded(x [..., 59]) -> [..., 11]."""
    OUT = _lib.MINI_QNET_OUT

    def __init__(self, env, net, final_relu=None):
        self.env, self.L = env, env.L
        pair = isinstance(net, (tuple, list)) and len(net) == 2
        nets = list(net) if pair else [net]
        srcs = [_mini_param_source(n, final_relu) for n in nets]
        if len({fr for _, fr in srcs}) != 1:
            raise ValueError("the two networks of a pair must agree on the final ReLU")
        self._srcs = [s for s, _ in srcs]
        self.pair = pair
        self.final_relu = srcs[0][1]
        shapes = [self._params(p)[1] for p in range(len(self._srcs))]
        if len(set(shapes)) != 1:
            raise ValueError("the two networks of a pair must have the same hidden size (got %s)" % (shapes,))
        self.h1 = shapes[0]
        self._d = _lib.EvgMiniQnet()
        self._d.struct_size = C.sizeof(_lib.EvgMiniQnet)

    def _params(self, p):
        """The 4 tensors of set p as they are now, checked: fp32, on the env's device, contiguous, 16-byte aligned, nn.Linear shapes."""
        torch = _torch()
        ts = self._srcs[p]()
        for t, n in zip(ts, ("w1", "b1", "w2", "b2")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.env.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float32 tensor on %s" % (n, self.env.device))
            if t.data_ptr() % 16:
                raise ValueError("%s must be 16-byte aligned" % n)
        w1, b1, w2, b2 = ts
        if w1.dim() != 2 or w1.shape[1] != 59 or not 1 <= w1.shape[0] <= _lib.MINI_QNET_MAX_HIDDEN:
            raise ValueError("w1 must be [h1, 59] with h1 in 1..%d, got %s" % (_lib.MINI_QNET_MAX_HIDDEN, tuple(w1.shape)))
        h1 = w1.shape[0]
        if tuple(w2.shape) != (self.OUT, h1) or tuple(b1.shape) != (h1,) or tuple(b2.shape) != (self.OUT,):
            raise ValueError("w2 [11, %d], b1 [%d], b2 [11] expected, got %s %s %s" % (h1, h1, tuple(w2.shape), tuple(b1.shape), tuple(b2.shape)))
        return ts, h1

    def _descriptor(self, sets):
        d = self._d
        for p in range(2):
            ts, h1 = self._params(p if self.pair else 0)
            if h1 != self.h1:
                raise ValueError("the network's hidden size changed from %d to %d" % (self.h1, h1))
            d.w1[p], d.b1[p], d.w2[p], d.b2[p] = (t.data_ptr() for t in ts)
            if not self.pair:
                break
        if sets == 2 and not self.pair:               # the same set on both seats
            d.w1[1], d.b1[1], d.w2[1], d.b2[1] = d.w1[0], d.b1[0], d.w2[0], d.b2[0]
        d.h1, d.final_relu, d.num_sets = self.h1, int(self.final_relu), sets
        return d

    _GRAD_ENTRY, _GRAD_STRUCT, _GRAD_PARTIAL = "evg_minimized_qnet_backward", _lib.EvgMiniQnetGrads, _lib.MINI_QNET_GRAD_PARTIAL

    def _launch(self, d, layout, rows, in0, in1, out):
        return self.L.evg_minimized_qnet(self.env._h, C.byref(d), layout, rows, C.c_void_p(in0.data_ptr()),
                                         None if in1 is None else C.c_void_p(in1.data_ptr()), C.c_void_p(out.data_ptr()), self.env._stream())


class _Bf16Launch(object):
    """The bf16 matrix-core forward (include/evg_qnet_bf16.h, libevg_bf16.so) in place of the fp32 launch: the one thing the two classes below change.
    A refused call's text is read from the library that refused it."""
    _ENTRY = None

    def with_grad(self, x, clamp=None):
        raise ValueError("with_grad() is defined on the fp32 chain: use the fp32 evaluator (precision=\"fp32\") for the policy forward")

    def _launch(self, d, layout, rows, in0, in1, out):
        B = _lib.load_bf16()
        rc = getattr(B, self._ENTRY)(self.env._h, C.byref(d), layout, rows, C.c_void_p(in0.data_ptr()),
                                     None if in1 is None else C.c_void_p(in1.data_ptr()), C.c_void_p(out.data_ptr()), self.env._stream())
        if rc:
            _lib.check(rc, B)
        return 0


class SmartQNetBf16(_Bf16Launch, SmartQNet):
    """SmartQNet with every layer on the bf16 matrix cores (evg_smart_qnet_bf16): inputs, weights and hidden activations rounded to bf16, fp32
    accumulation and fp32 Q -- the numeric contract of include/evg_qnet_bf16.h, for acting and for the target network.  The same calls, checks and
    parameter tracking; the fp32 parameters are read in place and converted on every call.  env.smart_qnet(net, precision="bf16") makes one."""
    _ENTRY = "evg_smart_qnet_bf16"


class MinimizedQNetBf16(_Bf16Launch, MinimizedQNet):
    """MinimizedQNet with both layers on the bf16 matrix cores (evg_minimized_qnet_bf16); see SmartQNetBf16.
    env.minimized_qnet(net, precision="bf16") makes one."""
    _ENTRY = "evg_minimized_qnet_bf16"


def make(env, net, final_relu, precision, fp32_cls, bf16_cls):
    """the evaluator of env.smart_qnet / env.minimized_qnet for a precision: "fp32" (the bit-exact chain, the default) or "bf16" """
    if precision == "fp32":
        return fp32_cls(env, net, final_relu=final_relu)
    if precision == "bf16":
        return bf16_cls(env, net, final_relu=final_relu)
    raise ValueError('precision must be "fp32" or "bf16" (got %r)' % (precision,))
