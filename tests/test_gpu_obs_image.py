"""GPU tests of how the two-lane step kernels put a lane's observation row into the wave's image in LDS (csrc/step_outputs.inc): whole dwords on the
flat image's dword grid, one 16-bit store per lane at its row boundary, the board part read by slot.  What that can break: the parity of a row (an odd
row starts half a dword in), the two halfwords on either side of a row boundary, the runtime node of a slot, and partial waves.

  - batch sizes 1, 2, 31, 33, 69: a single row pair, and partial waves with an odd and an even number of valid envs;
  - the persistent form (launches planned for 150 turns per launch) and the single-turn form of the two-lane kernel over 160 turns with auto-reset (the
    time-expired reset falls on turn 150), every observation type, both players: the observation tensor after each of the first three turns, after turn
    150 and after the last turn equals the oracle's exactly (oracle/oracle.py, as tests/test_gpu_parity.py uses it);
  - the one-seat form on either seat (there the row of a lane is its env, not its lane), with the Smart_State features read from the image;
  - the non-default maps of tests/golden/custom_varA.npz and custom_varC.npz; the latter's player-1 node map is not DemoMap's, so that a slot shows
    another node than in every other case;
  - every observation output is a view with 64 sentinel elements in front and behind, which must stay untouched.

Batches this small are played by the four-lane kernel in the product library's persistent launches, so the two-lane kernel is forced through the
diagnostic library (diag=dict(lanes=64); lanes=32 is its 16-envs-per-wave variant, whose helper lanes never store); the single-turn and one-seat forms
are the product library's own at every size.  The oracle's games are played once per batch size and shared, read-only."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SEED = 20261019
GUARD = 64
OBS_FILL = -7                     # a sentinel no element around the view may lose
SIZES = [1, 2, 31, 33, 69]
DTYPES = ["float32", "float64", "int16"]
TURNS, EXTRA = 150, 10            # DemoMap's turn limit; turns played beyond the time-expired reset


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


def _checkpoints(limit):
    return (1, 2, 3, limit, limit + EXTRA)


_REFERENCE = {}


def _reference(oracle_mod, n, tables=None, key="demo", limit=TURNS):
    """{turn: the oracle's observations [n, 2, 105] after that turn} of random-vs-random play with auto-reset, for the compared turns; played once"""
    if (n, key) not in _REFERENCE:
        ora = oracle_mod.Oracle(n, seed=SEED, auto_reset=True, tables=tables)
        ora.reset()
        want = {}
        for t in range(1, limit + EXTRA + 1):
            a = ora.random_actions()
            if t in _checkpoints(limit):
                want[t] = ora.step(a)[0]
                want[t].setflags(write=False)
            else:
                ora.step_noobs(a)
        _REFERENCE[(n, key)] = want
    return _REFERENCE[(n, key)]


class _Guarded(object):
    """an output as a view into a larger allocation filled with a sentinel, GUARD elements in front of it and GUARD behind (GUARD elements of every
    type used here are a multiple of 16 bytes, so the view keeps the allocation's alignment)"""

    def __init__(self, torch, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.big = torch.full((2 * GUARD + self.n,), OBS_FILL, dtype=dtype, device=dev)
        self.view = self.big[GUARD:GUARD + self.n].view(shape)

    def intact(self):
        return bool((self.big[:GUARD] == OBS_FILL).all()) and bool((self.big[GUARD + self.n:] == OBS_FILL).all())


def _guarded_env(evg, n, dtype, **kw):
    """an env whose observation buffer is a guarded view"""
    import torch
    env = evg.EvergladesVecEnv(n, seed=SEED, obs_dtype=dtype, auto_reset=True, **kw)
    g = _Guarded(torch, (n, 2, 105), env.obs_dtype, env.device)
    env._adopt_buffers(g.view, env.reward, env.done, env.winner, env.scores, env.status, env._actions)
    return env, g


def _play(env, guard, want, calls, tpl, what):
    """rollout_random in pieces of `calls` turns; after every piece whose last turn is a compared one the observation tensor must be the oracle's"""
    env.reset()
    t = 0
    for k in calls:
        env.rollout_random(k, turns_per_launch=tpl)
        t += k
        if t in want:
            got = _np(env.obs).astype(np.float64)
            for p in (0, 1):
                assert np.array_equal(got[:, p], want[t][:, p]), (what, "turn", t, "player", p)
            assert guard.intact(), (what, "turn", t, "sentinels")
    assert env.check_fault() == 0
    env.close()


def _both_forms(evg, n, dtype, want, form, limit=TURNS, **kw):
    two_lanes = dict(library=evg._lib.DIAG_LIB_PATH, diag=dict(lanes=kw.pop("lanes", 64)))
    if form == "persistent":
        # A launch of one turn IS the single-turn form, so the persistent kernel's first compared turn is 2: one handle plays 2 + (limit - 2 + EXTRA)
        # turns -- whole launches of `limit` turns and the rest --, another 1 + 2 + ... for turn 3.
        env, g = _guarded_env(evg, n, dtype, **two_lanes, **kw)
        _play(env, g, want, [2, limit - 2 + EXTRA], limit, (form, n, dtype, "a"))
        env, g = _guarded_env(evg, n, dtype, **two_lanes, **kw)
        _play(env, g, want, [1, 2, limit - 3, EXTRA], limit, (form, n, dtype, "b"))
    elif form == "single_turn":
        env, g = _guarded_env(evg, n, dtype, **two_lanes, **kw)
        _play(env, g, want, [1, 1, 1, limit - 3, EXTRA], 1, (form, n, dtype))
    else:                           # the product library's single-turn kernel: the two-lane one at every size
        env, g = _guarded_env(evg, n, dtype, **kw)
        _play(env, g, want, [1, 1, 1, limit - 3, EXTRA], 1, (form, n, dtype))


@pytest.mark.parametrize("form", ["persistent", "single_turn", "single_turn_product"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", SIZES)
def test_two_seat_image_equals_the_oracle(evg, oracle_mod, N, dtype, form):
    _both_forms(evg, N, dtype, _reference(oracle_mod, N), form)


@pytest.mark.parametrize("form", ["persistent", "single_turn"])
def test_helper_lanes_never_store_into_the_image(evg, oracle_mod, form):
    """the 16-envs-per-wave variant: lanes 32..63 own no row; 33 envs are two full waves and one with a single row pair"""
    _both_forms(evg, 33, "float32", _reference(oracle_mod, 33), form, lanes=32)


@pytest.mark.parametrize("form", ["persistent", "single_turn"])
@pytest.mark.parametrize("fname", ["custom_varA.npz", "custom_varC.npz"])
def test_slots_of_a_map_with_another_player_1_view(evg, oracle_mod, fname, form, tmp_path):
    """The map and unit files of tests/golden/custom_var*.npz through tables_from_json, as test_gpu_parity.py's custom-map test builds them: slot s of player
    1's rows shows node p1_node_map[s], read at a runtime node.  custom_varA changes the board's tables but keeps DemoMap's flip; custom_varC's flip is
    another one, and not its own inverse, so there a slot shows a node that it shows in no other case of this file."""
    d = load_golden(fname)
    files = {}
    for key, arg in (("map_json", "map_file"), ("unit_json", "unit_file")):
        if str(d[key]):
            path = tmp_path / (fname + "_" + arg + ".json")
            path.write_text(str(d[key]))
            files[arg] = str(path)
    tables = evg.tables_from_json(p1_node_map=d["p1_node_map"].tolist(), **files)
    if fname == "custom_varC.npz":
        flip = list(tables.p1_node_map)
        assert flip != list(evg.default_tables().p1_node_map) and [flip[flip[s]] for s in range(12)] != list(range(12))
    ot = oracle_mod.Tables()
    assert C.sizeof(ot) == C.sizeof(tables)
    C.memmove(C.byref(ot), C.byref(tables), C.sizeof(tables))
    limit = int(tables.max_turns)
    want = _reference(oracle_mod, 33, tables=ot, key=fname, limit=limit)
    _both_forms(evg, 33, "float32", want, form, limit=limit, tables=tables)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seat", [0, 1])
def test_one_seat_image_and_its_features_equal_the_oracle(evg, oracle_mod, seat, dtype):
    """evg_step_vs_policy_smart at 33 envs: the image is [env][105], so row parity follows the env; the caller's row against the oracle's on the compared
    turns, and the Smart_State features the kernel reads from the image against evg_smart_state_compact of the row it wrote"""
    import torch
    N, limit = 33, TURNS
    env = evg.EvergladesVecEnv(N, seed=SEED, obs_dtype=dtype, auto_reset=True)
    ora = oracle_mod.Oracle(N, seed=SEED, auto_reset=True)
    g = _Guarded(torch, (N, 105), env.obs_dtype, env.device)
    shared = torch.zeros((N, 34), device=env.device)
    swarm = torch.zeros((N, 12, 13), device=env.device)
    env.reset()
    o_obs = ora.reset()
    oa = np.zeros((N, 2, 7, 2), np.int32)
    for t in range(1, limit + EXTRA + 1):
        rows = env.random_actions_seat(seat)
        ora.scripted_actions(3, 1 - seat, o_obs, oa)            # EVG_POLICY_SWARM, as __graft_entry__.smoke() plays it
        oa[:, seat] = _np(rows)
        sobs = env.step_vs("swarm", rows, seat=seat, out=g.view, features=(shared, swarm))[0]
        o_obs = ora.step(oa)[0]
        if t in _checkpoints(limit):
            assert np.array_equal(_np(sobs).astype(np.float64), o_obs[:, seat]), ("one-seat obs", seat, dtype, t)
            assert g.intact(), ("sentinels", seat, dtype, t)
            w_shared, w_swarm = env.smart_state_compact(-1, sobs)
            assert torch.equal(shared, w_shared) and torch.equal(swarm, w_swarm), ("features", seat, dtype, t)
    assert env.check_fault() == 0
    env.close()
