"""CPU half of the planted combat positions (tests/combat_positions.py; the GPU half is tests/test_gpu_combat_positions.py): every family reaches the branch it
is built for -- the census numbers are asserted with their exact values --, the oracle accepts the position and plays it, and combat really happens.  These are
conditions on the INPUTS of the GPU tests; the expected values of a game always come from the oracle."""
import numpy as np
import pytest

import combat_positions as cp


def _oracle(oracle_mod, st, tables=None, seed=41):
    ora = oracle_mod.Oracle(len(st[0]), seed=seed, tables=tables, auto_reset=False)
    ora.reset()
    ora.set_state(*st)
    s = ora.get_state()
    for i, k in enumerate(("groups", "nodes", "health", "env")):
        assert np.array_equal(s[k], st[i]), ("the oracle hands the planted state back", k)
    return ora


def _hold(ora, turns=1):
    out = None
    for t in range(turns):
        out = ora.step(np.zeros((ora.n, 2, 7, 2), np.int32))
    return out


def _fought(census, before, after):
    """in every env that has fighting groups, units of BOTH sides lost health"""
    envs = sorted({r[0] for w in census for r in w["groups"]})
    assert envs
    lost = (after < before).any(axis=2)
    assert lost[envs].all(), [e for e in envs if not lost[e].all()]
    return envs


def test_builders_keep_the_rules_of_set_state(oracle_mod):
    t = oracle_mod.demo_tables()
    for st in (cp.family_a(), cp.family_b(32, 96), cp.family_b(16, 80), cp.family_c(), cp.family_d(t), cp.family_e(), cp.family_f()):
        cp.check_domain(st)
        stamps = st[0][..., 7]
        assert (np.diff(stamps, axis=2) < 0).any()               # list order differs from gid order


def test_family_a_reaches_every_round_count(oracle_mod):
    st = cp.family_a()
    c = cp.expect_a(st[0])
    assert len(st[0]) == 32 * 11 + 7
    ora = _oracle(oracle_mod, st)
    _hold(ora)
    envs = _fought(c, st[2], ora.get_state()["health"])
    idle = sorted(set(range(len(st[0]))) - set(envs))
    assert len(idle) == 44 and np.array_equal(ora.get_state()["health"][idle], st[2][idle])      # the 22 + 22 envs of "20+3" and "20" that do not fight
    # the other mappings see the same batch as other waves: nothing to assert but that the census describes them too
    assert sum(w["items"] for w in cp.census(st[0], 16)) == sum(w["items"] for w in c) == sum(w["items"] for w in cp.census(st[0], 16, True))


@pytest.mark.parametrize("envs_per_wave,alive,four_lane", [(32, 96, False), (16, 96, False), (16, 80, True)])
def test_family_b_sits_on_the_pool_cap(oracle_mod, envs_per_wave, alive, four_lane):
    st = cp.family_b(envs_per_wave, alive)
    c = cp.expect_b(st[0], envs_per_wave, four_lane)
    assert [w["words"] for w in c[:3]] == {(32, False): [1536, 1536, 1537], (16, False): [768, 768, 769], (16, True): [640, 640, 641]}[(envs_per_wave, four_lane)]
    per_side = (st[0][..., 6].sum(axis=2))
    assert (per_side == alive).sum() == per_side.size - 1 and per_side.max() == alive + 1
    ora = _oracle(oracle_mod, st)
    _hold(ora)
    _fought(c, st[2], ora.get_state()["health"])


def test_family_b_for_32_envs_is_at_the_cap_of_the_16_env_form_too():
    st = cp.family_b(32, 96)
    c = cp.census(st[0], 16)
    assert [w["words"] for w in c] == [768, 768, 768, 768, 768, 769, 336] and [w["npass"] for w in c] == [1, 1, 1, 1, 1, 2, 1]
    for w, g11 in ((0, 12), (1, 12), (2, 9), (3, 9)):
        env, side, gid, alive, base, sh0 = c[w]["groups"][-1]
        assert (env, side, gid, alive, base + alive, sh0) == (16 * w + 15, 1, 11, g11, 96, (96 - g11) & 3)


@pytest.mark.parametrize("which", ["saturating", "default"])
def test_family_c_fills_the_damage_byte(oracle_mod, which):
    t = cp.saturating_tables(oracle_mod.demo_tables) if which == "saturating" else oracle_mod.demo_tables()
    total = cp.army_damage(t, 0)
    assert total == (252 if which == "saturating" else 132)
    st = cp.family_c()
    c = cp.expect_c(st[0])
    ora = _oracle(oracle_mod, st, tables=t)
    _hold(ora)
    after = ora.get_state()["health"]
    _fought(c, st[2], after)
    # the damage the census predicts for player 1's survivors: every fighting unit of player 0 draws one of them
    for w in c:
        per_env = {}
        for env, side, gid, alive, base, sh0 in w["groups"]:
            if side == 0:
                per_env[env] = per_env.get(env, 0) + alive * t.unit_damage[t.group_type[0][gid]]
        assert set(per_env.values()) == {total}
    if which != "saturating":
        return
    armor = 255.0
    checked = 0
    for e in range(len(st[0])):
        if st[1][e, 5, 1] != -1:
            continue                                              # the node is held: the holder's units have the structure's defence as well
        slots = [8 * k + s for k, ss in cp.c_survivors(e % 4).items() for s in ss]
        h0, h1 = st[2][e, 1, slots], after[e, 1, slots]
        d = np.rint((h0 - h1) * armor / 10.0).astype(int)
        assert d.sum() == 252 and (d >= 0).all(), (e, d)
        for a, b, dd in zip(h0, h1, d):
            assert b == a - (10.0 * dd) / armor, (e, a, b, dd)   # server.py:601, :609
        if len(slots) == 1:
            assert h0[0] == 100.0 and h1[0] == 100.0 - (10.0 * 252) / 255.0
        checked += 1
    assert checked >= 16


def test_oversaturated_tables_exceed_the_byte(oracle_mod):
    assert cp.army_damage(cp.oversaturated_tables(oracle_mod.demo_tables)) == 260


@pytest.mark.parametrize("which", ["default", "custom"])
def test_family_d_kills_exactly(oracle_mod, which):
    if which == "custom":
        import everglades_amd
        from test_gpu_parity import _custom_tables
        _, t = _custom_tables(everglades_amd, oracle_mod)
    else:
        t = oracle_mod.demo_tables()
    a, tg = cp.d_pair(t)
    assert t.unit_damage[t.group_type[0][a]] == 1 and t.unit_health[t.group_type[0][tg]] == 3
    st = cp.family_d(t)
    c = cp.expect_d(st[0])
    cases = cp.d_cases()
    assert {(x[0], x[1], x[2]) for x in cases} == {(p, k, h) for p in range(2) for k in range(3) for h in range(3)}
    ora = _oracle(oracle_mod, st, tables=t)
    _hold(ora)
    s1 = ora.get_state()
    _fought(c, st[2], s1["health"])
    for e, (tp, ctl, hk, node) in enumerate(cases):
        slot = 8 * tg + (e * 3) % 8
        q = cp.d_quotient(t, node, ctl)
        if ctl == 1:
            assert q == 80.0 / (3.0 + t.node_defense[node]) and t.node_defense[node] > 0
        want_alive = hk == 1
        assert (s1["groups"][e, tp, tg, 6], s1["groups"][e, tp, tg, 5]) == ((1, 0) if want_alive else (0, 1)), (e, cases[e])
        assert s1["health"][e, tp, slot] == (np.nextafter(q, np.inf) - q if want_alive else 0.0), (e, cases[e])
    _hold(ora, 2)
    s3 = ora.get_state()
    for e, (tp, ctl, hk, node) in enumerate(cases):
        assert s3["groups"][e, tp, tg, 6] == 0                                                   # the float above the quotient dies on the second turn
        if ctl != 2:                                                                             # the attacker, alone now, takes the node over
            sign = 1 if tp == 1 else -1
            assert (s3["nodes"][e, node - 1, 0] - st[1][e, node - 1, 0]) * sign > 0, (e, cases[e])


def test_family_e_contests_all_eleven_nodes(oracle_mod):
    st = cp.family_e()
    c = cp.expect_e(st[0])
    alive = st[0][..., 6].sum(axis=2)
    assert 0.25 < 1.0 - alive.mean() / 100.0 < 0.35 and (st[0][..., 6] > 0).all()              # about 30 % dead, nobody wiped out
    assert (st[0][..., 4] != 0).sum() == 2 * (8 + 8 + 4) + 2 + 2                                # the groups in transit (waves 1, 2 and the ragged one)
    ora = _oracle(oracle_mod, st)
    _hold(ora)
    _fought(c, st[2], ora.get_state()["health"])
    four = cp.census(st[0], 16, True)
    assert four[0]["npass"] == 2 and four[0]["items"] + four[1]["items"] == 768                  # the four-lane kernel needs two passes for the same wave


def test_family_f_plays_in_stock_entropy_mode(oracle_mod):
    st = cp.family_f()
    N = len(st[0])
    assert N == 32 + cp.F_MELEE + 64 + 5
    c = cp.census(st[0], 32)
    assert [w["items"] for w in c] == cp.F_ITEMS == [424, 263, 34, 34]
    ora = oracle_mod.Oracle(N, seed=5, auto_reset=False)
    ora.use_stock_mt((5 + np.arange(N)) & 0xFFFFFFFF)
    ora.reset()
    ora.set_state(*st)
    m0 = ora.get_stock_entropy()
    _hold(ora)
    m1 = ora.get_stock_entropy()
    _fought(c, st[2], ora.get_state()["health"])
    # randint(1) consumes no output (oracle/evg_oracle.c mt_randint): with one survivor, player 0's 100 units draw nothing and the survivor draws one
    # randint(100) -- a few outputs with the masked rejection, nowhere near the 100 more that a consuming randint(1) would take
    used = (m1[:, 624].astype(int) - m0[:, 624].astype(int)) % 624
    for e in range(32):
        if e % 4 in (0, 1):
            assert 1 <= used[e] < 100, (e, used[e])
    assert (used[32:32 + cp.F_MELEE] >= 200).all()                 # the melee: 200 draws of randint(100), more where a draw is rejected
