"""GPU half of the planted combat positions (tests/combat_positions.py; CPU half: tests/test_combat_positions.py): every step-kernel mapping and form plays
the positions that playing never reaches -- a third and a twelfth round of the work list, the damage pool exactly at its cap and one word above, a damage
byte of 252, a lone survivor, a kill by the exact quotient, all eleven nodes contested -- and must equal the oracle after every turn: observations, scores,
done, status, winner, the whole state with float64 health bit for bit, rewards within REWARD_ATOL.  Before the first turn the census is asserted on the
DEVICE's state, so that a test cannot silently stop reaching its branch.

Both combat implementations are under test: csrc/step_combat.inc (product single-turn kernel, lanes = 64 / 32 / 256 / 2 of the diagnostic library, the
learner-seat and Q-decoding kernels) and csrc/evg_step4.inc (lanes = 4, and what the product launches for a persistent rollout of so few envs)."""
import numpy as np
import pytest

import combat_positions as cp
from test_gpu_parity import REWARD_ATOL, _custom_tables, check_state

pytestmark = pytest.mark.gpu

SEED = 20261020
HOLD, RANDOM = 3, 2                                       # turns: everyone holds (orders to node 0, which is no node), then random orders


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


def _expect_b32(groups):
    cp.expect_b(groups, 32)
    c = cp.census(groups, 16)                             # the same batch in the 16-env form: five wavefronts at its cap of 768, one above
    assert [w["words"] for w in c] == [768, 768, 768, 768, 768, 769, 336] and [w["npass"] for w in c] == [1, 1, 1, 1, 1, 2, 1]


FAMILIES = {
    "A": (lambda t: cp.family_a(), "default", cp.expect_a),
    "B two-lane": (lambda t: cp.family_b(32, 96), "default", _expect_b32),
    "B four-lane": (lambda t: cp.family_b(16, 80), "default", lambda g: cp.expect_b(g, 16, True)),
    "C": (lambda t: cp.family_c(), "saturating", cp.expect_c),
    "D": (lambda t: cp.family_d(t), "default", cp.expect_d),
    "D custom": (lambda t: cp.family_d(t), "custom", cp.expect_d),
    "E": (lambda t: cp.family_e(), "default", cp.expect_e),
}
MAPPINGS = {"product": dict(), "lanes32": dict(lanes=32), "lanes256": dict(lanes=256), "lanes4": dict(lanes=4), "lanes2": dict(lanes=2), "lanes64": dict(lanes=64)}
_REF = {}


def _tables(evg, oracle_mod, which):
    if which == "custom":
        return _custom_tables(evg, oracle_mod)
    if which == "saturating":
        return cp.saturating_tables(evg.default_tables, oracle_mod)
    return evg.default_tables(), oracle_mod.demo_tables()


def _orders(N, t, rng):
    """hold (node 0 is no node: no order is valid), then random groups to random nodes"""
    a = np.zeros((N, 2, 7, 2), np.int32)
    if t >= HOLD:
        a[..., 0] = rng.integers(0, 12, size=(N, 2, 7))
        a[..., 1] = rng.integers(1, 12, size=(N, 2, 7))
    return a


def _reference(evg, oracle_mod, name):
    """the oracle's game from the planted position, computed once per family and left unchanged: per turn the orders, the step's outputs and the state"""
    if name not in _REF:
        build, which, expect = FAMILIES[name]
        t, ot = _tables(evg, oracle_mod, which)
        st = build(ot)
        ora = oracle_mod.Oracle(len(st[0]), seed=SEED, tables=ot, auto_reset=False)
        ora.reset()
        ora.set_state(*st)
        rng = np.random.default_rng(7)
        turns = []
        for k in range(HOLD + RANDOM):
            a = _orders(len(st[0]), k, rng)
            obs, rew, done, info = ora.step(a)
            turns.append(dict(a=a, obs=obs, rew=rew, done=done, info=info, state=ora.get_state()))
        assert not turns[HOLD - 1]["done"].any()
        assert (turns[0]["state"]["health"] < st[2]).any(axis=2).any(axis=0).all()       # combat happened, on both sides
        _REF[name] = dict(st=st, tables=t, otables=ot, first=ora_first_obs(oracle_mod, st, ot), turns=turns, expect=expect)
    return _REF[name]


def ora_first_obs(oracle_mod, st, ot):
    ora = oracle_mod.Oracle(len(st[0]), seed=SEED, tables=ot, auto_reset=False)
    ora.reset()
    ora.set_state(*st)
    return ora.observe()


def _env(evg, ref, diag=None, auto_reset=False, **kw):
    extra = dict(library=evg._lib.DIAG_LIB_PATH, diag=diag) if diag else {}
    env = evg.EvergladesVecEnv(len(ref["st"][0]), seed=SEED, auto_reset=auto_reset, tables=ref["tables"], **extra, **kw)
    env.reset()
    env.set_state(*ref["st"])
    ref["expect"](env.get_state()["groups"])              # the census of the DEVICE's state: the position reaches the branch it is built for
    return env


def _same_turn(got, want, what, seat=None):
    obs, rew, done, info = got
    assert np.array_equal(_np(obs).astype(np.float64), want["obs"] if seat is None else want["obs"][:, seat]), (what, "obs")
    assert np.array_equal(_np(info["scores"]), want["info"]["scores"]) and np.array_equal(_np(info["status"]), want["info"]["status"]), (what, "scores / status")
    assert np.array_equal(_np(info["winner"]), want["info"]["winner"]) and np.array_equal(_np(done), want["done"]), (what, "winner / done")
    assert np.allclose(_np(rew), want["rew"], rtol=0, atol=REWARD_ATOL), (what, "reward")


def _play_single_turns(evg, oracle_mod, name, diag):
    ref = _reference(evg, oracle_mod, name)
    env = _env(evg, ref, diag)
    assert np.array_equal(_np(env.observe()).astype(np.float64), ref["first"]), (name, "observation of the planted position")
    for k, want in enumerate(ref["turns"]):
        _same_turn(env.step(want["a"]), want, (name, diag, k))
        check_state(env, want["state"], (name, diag, k))
    env.close()


# ---------------------------------------------------------------------------------------------- evg_step: the product kernel and the diagnostic mappings
@pytest.mark.parametrize("mapping", ["product", "lanes32", "lanes256", "lanes4", "lanes2"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_single_turn_forms_equal_the_oracle(evg, oracle_mod, name, mapping):
    """evg_step, one launch per turn: three turns holding, two of random orders, compared after every turn"""
    _play_single_turns(evg, oracle_mod, name, MAPPINGS[mapping] or None)


@pytest.mark.parametrize("lanes", [0, 4])
@pytest.mark.parametrize("name", ["C", "D", "D custom"])
def test_true_division_branch_equals_the_oracle(evg, oracle_mod, name, lanes):
    """force_ieee_div: the kernels' true-division branch (the table-reciprocal quotient is what the single-turn cases above run, where the table set passes
    evg_create's validation) on the saturated byte and on the exact kills, in both combat implementations"""
    _play_single_turns(evg, oracle_mod, name, dict(lanes=lanes, force_ieee_div=True))


# ---------------------------------------------------------------------------------------------- persistent launches
@pytest.mark.parametrize("mapping", ["product", "lanes64"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_persistent_launch_equals_the_oracle(evg, oracle_mod, name, mapping):
    """one launch of three turns with both seats played by the on-device "no_action" bot, so that the planted counts hold inside the launch: the product
    (the four-lane kernel at this batch size) and the two-lane persistent kernel"""
    ref = _reference(evg, oracle_mod, name)
    env = _env(evg, ref, MAPPINGS[mapping] or None, auto_reset=True)
    if mapping == "product":
        assert "four lanes" in env.launch_plan(HOLD)[1]
    want = ref["turns"][HOLD - 1]
    got = env.rollout_policies(HOLD, "no_action", "no_action", turns_per_launch=HOLD)
    _same_turn(got, want, (name, mapping, "last turn of the launch"))
    check_state(env, want["state"], (name, mapping))
    env.close()


# ---------------------------------------------------------------------------------------------- the other kernels that compile the combat fragment
@pytest.mark.parametrize("seat", [0, 1])
@pytest.mark.parametrize("name", ["A", "E"])
def test_learner_seat_turn_equals_the_oracle(evg, oracle_mod, name, seat):
    """evg_step_vs_policy: the caller holds, the "no_action" bot plays the other seat inside the step kernel"""
    ref = _reference(evg, oracle_mod, name)
    env = _env(evg, ref)
    want = ref["turns"][0]
    rows = np.zeros((len(ref["st"][0]), 7, 2), np.int32)
    _same_turn(env.step_vs("no_action", rows, seat=seat), want, (name, seat), seat=seat)
    check_state(env, want["state"], (name, seat))
    env.close()


@pytest.mark.parametrize("head", ["smart", "minimized"])
@pytest.mark.parametrize("name", ["A", "E"])
def test_q_decoding_turn_equals_the_oracle(evg, oracle_mod, name, head):
    """evg_step_vs_policy_smart_q / evg_step_vs_policy_minimized_q with zero Q values and epsilon 0: the rows the kernel decodes and plays come back in
    actions_out; the oracle plays the same rows.  An order only readies a group (server.py:251-270), and a ready group fights like an idle one (:525), so
    the census asserted on the planted state is that of the post-order state too."""
    import torch
    ref = _reference(evg, oracle_mod, name)
    N = len(ref["st"][0])
    env = _env(evg, ref)
    q = torch.zeros((N, 12, 5 if head == "smart" else 11), device=env.device)
    rows = torch.full((N, 7, 2), -9, dtype=torch.int32, device=env.device)
    got = env.step_vs_q("no_action", q, 0.0, seat=0, actions_out=rows)
    ora = oracle_mod.Oracle(N, seed=SEED, tables=ref["otables"], auto_reset=False)
    ora.reset()
    ora.set_state(*ref["st"])
    oa = np.zeros((N, 2, 7, 2), np.int32)
    oa[:, 0] = _np(rows)
    assert (oa[:, 0] != -9).all() and oa[:, 0].any()
    obs, rew, done, info = ora.step(oa)
    post = ora.get_state()
    _same_turn(got, dict(obs=obs, rew=rew, done=done, info=info), (name, head), seat=0)
    check_state(env, post, (name, head))
    env.close()


# ---------------------------------------------------------------------------------------------- F: stock entropy
@pytest.mark.parametrize("form", ["evg_step", "persistent"])
def test_stock_entropy_positions_equal_the_oracle(evg, oracle_mod, form):
    """rng_mode="mt19937": a lone survivor is drawn with randint(1), which consumes no generator output; a full melee draws randint(100) by masked rejection.
    The games AND the generators' final states (key words and position) must equal the oracle's."""
    st = cp.family_f()
    N = len(st[0])
    env = evg.EvergladesVecEnv(N, seed=SEED, auto_reset=(form == "persistent"), rng_mode="mt19937")
    ora = oracle_mod.Oracle(N, seed=SEED, auto_reset=(form == "persistent"))
    ora.use_stock_mt((SEED + np.arange(N)) & 0xFFFFFFFF)
    env.reset(); ora.reset()
    m0 = ora.get_stock_entropy()
    assert np.array_equal(env.get_stock_entropy(), m0)
    env.set_state(*st); ora.set_state(*st)
    # the oracle's set_state recomputes the scores with its game_end, which draws the reference's unobservable focus at a turn that is a multiple of 10
    # (oracle/evg_oracle.c:259): a draw no game makes, so the oracle's generators go back to where loading the position found them
    ora.set_stock_entropy(m0)
    c = cp.census(env.get_state()["groups"], 32)
    assert [w["items"] for w in c] == cp.F_ITEMS, [w["items"] for w in c]
    assert np.array_equal(env.get_stock_entropy(), m0)
    rng = np.random.default_rng(3)
    if form == "evg_step":
        for k in range(HOLD + RANDOM):
            a = _orders(N, k, rng)
            obs, rew, done, info = ora.step(a)
            _same_turn(env.step(a), dict(obs=obs, rew=rew, done=done, info=info), ("stock entropy", k))
            check_state(env, ora.get_state(), ("stock entropy", k))
            assert np.array_equal(env.get_stock_entropy(), ora.get_stock_entropy()), ("generator state", k)
    else:
        got = env.rollout_policies(HOLD, "no_action", "no_action", turns_per_launch=HOLD)
        for k in range(HOLD):
            obs, rew, done, info = ora.step(np.zeros((N, 2, 7, 2), np.int32))
        _same_turn(got, dict(obs=obs, rew=rew, done=done, info=info), "stock entropy, rollout")
        check_state(env, ora.get_state(), "stock entropy, rollout")
        assert np.array_equal(env.get_stock_entropy(), ora.get_stock_entropy())
    env.close()


# ---------------------------------------------------------------------------------------------- the refusal
def test_an_army_that_overflows_the_damage_byte_is_refused(evg, oracle_mod):
    """evg_create needs a device before it looks at the tables, so the refusal is tested here: 260 is refused with EVG_ERR_INVALID and its message, 252 --
    the largest total an army of this shape can have below 256 -- is accepted (and played by the cases "C" above)"""
    over = cp.oversaturated_tables(evg.default_tables)
    with pytest.raises(evg.EvgError) as ei:
        evg.EvergladesVecEnv(4, seed=1, tables=over)
    assert "libevg error %d:" % evg._lib.ERR_ARG in str(ei.value) and "total damage of an army must fit 8 bits" in str(ei.value)
    t, _ = cp.saturating_tables(evg.default_tables, oracle_mod)
    env = evg.EvergladesVecEnv(4, seed=1, tables=t)
    env.reset()
    env.close()
