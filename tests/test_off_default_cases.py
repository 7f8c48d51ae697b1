"""CPU tests (no GPU needed) of the constants of tests/off_default_cases.py, on the oracle and the host models alone: what the GPU tests of
tests/test_gpu_off_defaults.py rely on to tell a kernel that drops the key's high word or the env id base from one that keeps them."""
import numpy as np
import pytest

import league_model as lm
import minimized_model as mm
import off_default_cases as cases
import rng_spec

LOW = cases.SEED & 0xFFFFFFFF


def test_the_seed_has_two_different_non_zero_words_and_the_ids_end_at_the_top():
    assert cases.SEED >> 32 and LOW and cases.SEED >> 32 != LOW
    for n in cases.SIZES + (1, 33, 64, 77):
        assert cases.base_for(n) + n == 2 ** 32 and cases.base_for(n) > 0


@pytest.mark.parametrize("N", cases.SIZES)
def test_the_oracle_keeps_the_high_word_and_the_id_base(oracle_mod, N):
    """the oracle's action rows are rng_spec's for the 64-bit seed and ids up to 0xFFFFFFFF; the low word alone, or ids from 0, draw other rows"""
    base = cases.base_for(N)
    rows = {}
    for name, seed, b in (("full", cases.SEED, base), ("low word", LOW, base), ("no base", cases.SEED, 0)):
        o = oracle_mod.Oracle(N, seed=seed, env_id_base=b)
        o.reset()
        rows[name] = o.random_actions()
    want = np.array([[rng_spec.random_action_rows(cases.SEED, base + e, 0, 0, p) for p in range(2)] for e in range(N)], np.int32)
    assert np.array_equal(rows["full"], want)
    for other in ("low word", "no base"):
        assert (rows["full"] != rows[other]).reshape(N, -1).any(1).all(), other         # in every env


def test_every_host_model_draws_differently_without_the_high_word(oracle_mod):
    N = cases.SIZES[0]
    ids = (cases.base_for(N) + np.arange(N)).astype(np.uint32)
    zero, ones = np.zeros(N, np.uint32), np.ones(N, np.float32)
    # the Smart_State agent's exploring decode (oracle.smart_get_action) and the Minimized agents' (minimized_model.get_action), epsilon 1
    obs = oracle_mod.Oracle(N, seed=cases.SEED, env_id_base=cases.base_for(N)).reset()
    q5, q11 = np.zeros((N, 12, 5), np.float32), np.zeros((N, 12, 11), np.float32)
    a = [oracle_mod.smart_get_action(q5, obs[:, 0], s, ids, zero, 0, ones)[0] for s in (cases.SEED, LOW)]
    assert (a[0] != a[1]).reshape(N, -1).any(1).all()
    b = [mm.get_action(q11, s, ids, zero, zero, 0, ones)[0] for s in (cases.SEED, LOW)]
    assert (b[0] != b[1]).reshape(N, -1).any(1).all()
    # the league's draw, the delay coin and the swarm shuffle
    for e in (int(ids[0]), int(ids[-1])):
        assert lm.league_word(cases.SEED, e, 1, 0) != lm.league_word(LOW, e, 1, 0)
        assert rng_spec.delay_uniform(cases.SEED, e, 0, 3, 1) != rng_spec.delay_uniform(LOW, e, 0, 3, 1)
    shuffles = [[rng_spec.swarm_shuffle(s, int(e), 0, 0, 1, range(8)) for e in ids] for s in (cases.SEED, LOW)]
    assert shuffles[0] != shuffles[1]
    for league in cases.LEAGUES:
        assert cases.model_histories(N, 0, league) != cases.model_histories(N, 0, league, seed=LOW)


@pytest.mark.parametrize("league", sorted(cases.LEAGUES))
@pytest.mark.parametrize("seat", [0, 1])
@pytest.mark.parametrize("N", cases.SIZES)
def test_the_leagues_play_every_member_and_return_to_one(N, seat, league):
    """within cases.EPISODES episodes: every member of non-zero weight is played, the member of weight zero never, some env changes its member and some env
    leaves a member and returns to it; ids from 0 would give other histories"""
    members, weights = cases.LEAGUES[league]
    h = cases.model_histories(N, seat, league)
    assert all(len(a) == cases.EPISODES for a in h)
    assert {x for a in h for x in a} == {m for m, w in enumerate(weights) if w > 0}
    assert any(a[i] != a[i + 1] for a in h for i in range(len(a) - 1))
    assert any(a[i] != a[i - 1] and a[i] in a[:i - 1] for a in h for i in range(2, len(a)))
    if league == "q":                                   # ... and it is the network member that some env leaves and returns to
        q = members.index("q")
        assert any(a[i] == q and a[i - 1] != q and q in a[:i - 1] for a in h for i in range(2, len(a)))
    m = lm.League(cases.SEED, 0, N, len(members), seat, True, weights)
    m.clear(np.zeros(N, np.int64))
    assert [a[0] for a in h] != [a[0] for a in m.history]


@pytest.mark.parametrize("N", cases.SIZES)
def test_random_games_at_these_ids_end_within_150_turns_with_both_winners(oracle_mod, N):
    o = oracle_mod.Oracle(N, seed=cases.SEED, env_id_base=cases.base_for(N))
    o.reset()
    for t in range(150):
        obs, reward, done, info = o.step(o.random_actions())
    assert done.all()
    assert {0, 1} <= set(info["winner"].tolist())
