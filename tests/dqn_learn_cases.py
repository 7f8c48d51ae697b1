"""Cases of the agents/DQN family's learner step (include/evg_dqn_learn.h), shared by the CPU and the GPU tests.

td_case(B, seed) -> dict of the TD head's operands.  q_next is post-ReLU (about half of a row is exact 0.0, never -0.0); the first rows carry the
plants, row i the plant (i + seed) % 7, so that a batch of one row meets every plant over seeds 0..6:

  0  all 132 values equal                                  4  the maximum at index 0
  1  exactly three positive values, the rest 0.0           5  duplicate actions within the row (the same column three times, another twice)
  2  the seven largest all in the registers of lane 5      6  actions outside 0..131 (132, -1, 2^40), next to valid ones
     (elements 5, 21, ..., 101 of the 16-lane mapping)
  3  the maximum at index 131

adam_case(counts, seed) -> (params, grads) lists of fp32 arrays, gradients reaching past a clamp of 1.

check_td_refusals / check_adam_refusals(_lib, G, handle, address): every refusal of the two entry points through the ABI.  All of them are decided
before the handle or any pointer is used, so the CPU test runs them on a handle and an address that are merely non-NULL and aligned, the GPU test on
real ones."""
import ctypes as C

import numpy as np

OUT, K = 132, 7
PLANTS = 7
BATCHES = (1, 3, 16, 17, 64, 257)
NET_COUNTS = (55440, 528, 69696, 132)                       # the 105-528-132 network's own tensors


def past_cap_batch(max_blocks):
    return 16 * max_blocks + 19


def past_cap_count(max_blocks):
    return 4 * 256 * max_blocks + 1027


def td_case(B, seed):
    rng = np.random.RandomState(1000 * seed + B % 997)
    q_next = np.maximum(rng.standard_normal((B, OUT)) * 1.5, 0.0).astype(np.float32)
    q_pred = rng.standard_normal((B, OUT)).astype(np.float32)
    action = rng.randint(0, OUT, size=(B, K)).astype(np.int64)
    reward = (rng.standard_normal(B) * 0.5).astype(np.float32)
    for i in range(min(B, PLANTS)):
        plant = (i + seed) % PLANTS
        if plant == 0:
            q_next[i] = 0.75
        elif plant == 1:
            q_next[i] = 0.0
            q_next[i, [7, 40, 130]] = [0.5, 2.25, 1.125]
        elif plant == 2:
            q_next[i] = np.minimum(q_next[i], 1.0)
            q_next[i, 5:5 + 16 * 7:16] = [3.0, 9.0, 4.0, 8.0, 5.0, 7.0, 6.0]
        elif plant == 3:
            q_next[i, 131] = 11.0
        elif plant == 4:
            q_next[i, 0] = 12.0
        elif plant == 5:
            action[i] = [9, 131, 9, 0, 131, 9, 64]
        elif plant == 6:
            action[i] = [3, 132, -1, 1 << 40, 131, 3, -(1 << 40)]
    assert not np.signbit(q_next[q_next == 0]).any()
    return {"q_pred": q_pred, "action": action, "q_next": q_next, "reward": reward, "not_done": rng.rand(B) < 0.7,
            "weights": rng.uniform(0.1, 2.0, B).astype(np.float32)}


def adam_case(counts, seed):
    rng = np.random.RandomState(77 + seed)
    params = [rng.standard_normal(c).astype(np.float32) for c in counts]
    grads = [[(rng.standard_normal(c) * (0.01, 1.0, 30.0)[(s + i) % 3]).astype(np.float32) for i, c in enumerate(counts)] for s in range(5)]
    return params, grads


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _td_descriptor(_lib, address):
    d = _lib.EvgDqnTdHeadArgs()
    d.struct_size, d.mode, d.batch, d.gamma = C.sizeof(d), 0, 64, 0.99
    for f in ("q_pred", "action", "q_next", "reward", "not_done", "weights", "gq", "loss", "priorities", "estimated", "workspace"):
        setattr(d, f, address)
    d.workspace_bytes = _lib.DQN_TD_WORKSPACE_BYTES
    return d


def check_td_refusals(_lib, G, handle, address):
    bad = [("struct_size", 8, "struct_size"), ("batch", 0, "batch"), ("batch", -3, "batch"), ("batch", (1 << 20) + 1, "batch"), ("mode", 2, "mode"),
           ("mode", -1, "mode"), ("gamma", float("nan"), "gamma"), ("gamma", float("inf"), "gamma"), ("workspace_bytes", _lib.DQN_TD_WORKSPACE_BYTES - 1, "workspace")]
    bad += [(f, None, "NULL") for f in ("q_pred", "action", "q_next", "reward", "gq", "loss", "workspace")]
    bad += [(f, address + 8, "aligned") for f in ("q_pred", "action", "q_next", "reward", "not_done", "weights", "gq", "loss", "priorities", "estimated",
                                                  "workspace")]
    for field, value, text in bad:
        d = _td_descriptor(_lib, address)
        setattr(d, field, value)
        assert G.evg_dqn_td_head(handle, C.byref(d), None) == -1, (field, value)
        assert text in G.evg_last_error().decode(), (field, value, G.evg_last_error())
    d = _td_descriptor(_lib, address)
    assert G.evg_dqn_td_head(None, C.byref(d), None) == -1 and "null handle" in G.evg_last_error().decode()
    assert G.evg_dqn_td_head(handle, None, None) == -1 and "null handle" in G.evg_last_error().decode()


def _adam_descriptor(_lib, address, n=4):
    a = _lib.EvgAdamArgs()
    a.struct_size, a.n, a.lr, a.beta1, a.beta2, a.eps, a.clamp, a.fresh_state, a.ctl = C.sizeof(a), n, 1e-4, 0.9, 0.999, 1e-8, 1.0, 0, address
    for i in range(n):
        e = a.t[i]
        e.param, e.grad, e.m, e.v, e.count = address, address, address, address, 132
    return a


def check_adam_refusals(_lib, G, handle, address):
    nan, inf = float("nan"), float("inf")
    bad = [("struct_size", 8, "struct_size"), ("n", 0, "n must"), ("n", 7, "n must"), ("lr", nan, "lr"), ("lr", inf, "lr"), ("beta1", 1.0, "betas"),
           ("beta1", -0.1, "betas"), ("beta2", 1.0, "betas"), ("beta2", nan, "betas"), ("eps", 0.0, "eps"), ("eps", inf, "eps"), ("clamp", -1.0, "clamp"),
           ("clamp", inf, "clamp"), ("ctl", None, "ctl"), ("ctl", address + 8, "aligned")]
    for field, value, text in bad:
        a = _adam_descriptor(_lib, address)
        setattr(a, field, value)
        assert G.evg_adam_step_wide(handle, C.byref(a), None) == -1, (field, value)
        assert text in G.evg_last_error().decode(), (field, value, G.evg_last_error())
    for field, value, text in [("count", 0, "count"), ("count", (1 << 24) + 1, "count"), ("param", None, "NULL"), ("grad", None, "NULL"), ("m", None, "NULL"),
                               ("v", None, "NULL"), ("param", address + 4, "aligned"), ("grad", address + 8, "aligned"), ("m", address + 12, "aligned"),
                               ("v", address + 8, "aligned")]:
        a = _adam_descriptor(_lib, address)
        setattr(a.t[3], field, value)
        assert G.evg_adam_step_wide(handle, C.byref(a), None) == -1, (field, value)
        assert text in G.evg_last_error().decode() and "tensor 3" in G.evg_last_error().decode(), (field, value, G.evg_last_error())
    a = _adam_descriptor(_lib, address)
    assert G.evg_adam_step_wide(None, C.byref(a), None) == -1 and "null handle" in G.evg_last_error().decode()
    assert G.evg_adam_step_wide(handle, None, None) == -1 and "null handle" in G.evg_last_error().decode()
