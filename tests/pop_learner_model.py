"""Host model of the population learner's grouped stages (include/evg_pop_learn.h, everglades_amd.PopulationLearner).  It only composes the existing
models, with no arithmetic of its own: member m receives tests/learner_model.py's TD head, tests/qnet_grad_model.py's backward and learner_model's Adam
on the gathered rows R_m = {b : ids[b] == m}, ascending -- which divides by c_m = |R_m| by construction -- and the results go back to the rows'
positions.  The bounds are the existing counted ones with B := c_m.  A row whose id is >= K belongs to nobody: a zero gq row, priority 0,
estimated 0, in no sum.  A member with c_m = 0: loss 0, zero gradients (bound 0: they must be equal), and no Adam step at all.

  rows_of(ids, K)                               -> [R_0, ..., R_(K-1)]
  td_head(ops, ids, K, exact=False)             -> (values, bounds): gq [B, OUT], priorities [B], estimated [B], loss [K]
  td_head32(ops, ids, K)                        -> the same values in the header's fp32 order (the loss summed in evg_td_head's order for c_m rows)
  backward(x, params, final_relu, gq, ids, ...) -> ([grads of member m], [bounds of member m])
  adam(params, grads, m, v, ctls, counts, ...)  -> per member learner_model.adam, or the state unchanged with zero bounds where counts[m] == 0
"""
import numpy as np

import learner_model
import qnet_grad_model

F32 = np.float32
ROW_KEYS = ("q_pred", "action", "q_next", "q_select", "reward", "not_done", "weights")


def rows_of(ids, K):
    ids = np.asarray(ids)
    return [np.flatnonzero(ids == m) for m in range(K)]


def take(ops, rows):
    """the operands of learner_model.td_head restricted to `rows`"""
    return {k: (v[rows] if k in ROW_KEYS and v is not None else v) for k, v in ops.items()}


def _td(fn, ops, ids, K, **kw):
    B, OUT = np.asarray(ops["q_pred"]).shape
    both = fn is learner_model.td_head
    vals = {"gq": np.zeros((B, OUT)), "priorities": np.zeros(B), "estimated": np.zeros(B), "loss": np.zeros(K)}
    bounds = {k: np.zeros_like(v) for k, v in vals.items()}
    for m, R in enumerate(rows_of(ids, K)):
        if len(R) == 0:
            continue
        out = fn(**take(ops, R), **kw)
        got, E = out if both else (out, None)
        for k in ("gq", "priorities", "estimated"):
            vals[k][R] = got[k]
            if both:
                bounds[k][R] = E[k]
        vals["loss"][m] = got["loss"]
        if both:
            bounds["loss"][m] = E["loss"]
    return (vals, bounds) if both else vals


def td_head(ops, ids, K, exact=False):
    return _td(learner_model.td_head, ops, ids, K, exact=exact)


def td_head32(ops, ids, K):
    return _td(learner_model.td_head32, ops, ids, K)


def backward(x, params, final_relu, gq, ids, exact=False, clamp=0.0):
    """params: the members' parameter lists.  -> (grads[m], bounds[m]), each a list in the order of the member's parameters"""
    x, gq = np.asarray(x, F32).reshape(-1, 59), np.asarray(gq, F32)
    grads, bounds = [], []
    for m, R in enumerate(rows_of(ids, len(params))):
        if len(R) == 0:
            grads.append([np.zeros(np.shape(p)) for p in params[m]])
            bounds.append([np.zeros(np.shape(p)) for p in params[m]])
            continue
        g, E = qnet_grad_model.backward(x[R], params[m], final_relu, gq[R], exact=exact, clamp=clamp)
        grads.append([a.reshape(np.shape(p)) for a, p in zip(g, params[m])])
        bounds.append([a.reshape(np.shape(p)) for a, p in zip(E, params[m])])
    return grads, bounds


def roundings(kind_sizes, ids, K):
    """qnet_grad_model.roundings with B := c_m, per member (None for a member without rows)"""
    return [qnet_grad_model.roundings(kind_sizes, len(R)) if len(R) else None for R in rows_of(ids, K)]


def adam(params, grads, m, v, ctls, counts, **kw):
    """per member: ((params', m', v', ctl'), (E_param, E_m, E_v)); a member whose count is 0 keeps everything, with zero bounds"""
    out = []
    for mb in range(len(params)):
        if counts[mb] == 0:
            keep = lambda ts: [np.asarray(t, np.float64) for t in ts]
            zero = [np.zeros(np.shape(t)) for t in params[mb]]
            out.append(((keep(params[mb]), keep(m[mb]), keep(v[mb]), ctls[mb]), (zero, zero, zero)))
        else:
            out.append(learner_model.adam(params[mb], grads[mb], m[mb], v[mb], ctls[mb], **kw))
    return out
