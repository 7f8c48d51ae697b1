"""Planted combat positions and a host census of the step kernels' combat work list.  No GPU, no test: tests/test_combat_positions.py (CPU, oracle only)
and tests/test_gpu_combat_positions.py (every step-kernel mapping against the oracle) import it.

Builders return (groups, nodes, health, env) in the evg_set_state layout (include/evg.h; csrc/evg_abi.hip evg_set_state) and keep its rules: count and
destroyed agree with health > 0, health is 0 or in (0, 100], the turn is 10, arrival stamps are mixed so that list order differs from gid order.

census() restates, on the host, the arithmetic with which the two mappings lay out a turn of combat -- csrc/step_combat.inc (two lanes per env, 32 or 16
envs per wavefront) and csrc/evg_step4.inc (four lanes per env, 16 envs per wavefront); the source line stands beside each formula.  It says WHICH BRANCH a
position reaches and nothing else: every expected value of a game comes from the oracle."""
import ctypes as C

import numpy as np

from test_gpu_parity import _pool_words

NP, NG, NN, NU = 2, 12, 11, 100
SIZE = [8] * 11 + [12]
HOME = (1, 11)
TURN = 10
WG = 64                                 # a wavefront; a round of the work list is WG items (step_combat.inc:205, :255; evg_step4.inc:409, :437)
DP_CAP = {(32, False): 1536, (16, False): 768, (16, True): 640}      # step_common.inc:8 (LPW == 64 ? 1536 : 768); evg_step4.inc:36
NEIGHBOUR = {1: 2, 2: 3, 3: 6, 4: 3, 5: 3, 6: 9, 7: 9, 8: 9, 9: 6, 10: 9, 11: 10}    # a connected node, in DemoMap and in _custom_tables' map alike


# ---------------------------------------------------------------------------------------------------------------- state helpers
def blank(N, turn=TURN):
    """N envs in the game_init position (everyone at home, full health) at turn `turn`"""
    groups = np.zeros((N, NP, NG, 8), np.int32)
    nodes = np.zeros((N, NN, 2), np.int32)
    health = np.full((N, NP, NU), 100.0)
    env = np.zeros((N, 4), np.int32)
    for p in range(NP):
        for k in range(NG):
            groups[:, p, k] = [HOME[p], -1, 0, 0, 0, 0, SIZE[k], 0]
    nodes[:, :, 1] = -1
    nodes[:, 0] = [500, 0]
    nodes[:, 10] = [-500, 1]
    env[:, 0] = turn
    return groups, nodes, health, env


def alive_slots(size, n, rot):
    """n of `size` slots, spread so that the alive mask has holes: slot (3 s + rot) mod 8, (5 s + rot) mod 12 for s < n"""
    mul = 3 if size == 8 else 5
    return sorted(((mul * s + rot) % size) for s in range(n))


def put(st, e, p, k, node, alive=None, stamp=0, hp=None, moving_to=None, dist=2):
    """group k of player p in env e stands at `node` with the slots `alive` (default: all) alive; hp: their health (a number, or one per alive slot);
    moving_to: the group is in transit through `node` (it does not fight, server.py:525)"""
    groups, nodes, health, env = st
    alive = list(range(SIZE[k])) if alive is None else list(alive)
    row = np.zeros(SIZE[k])
    vals = np.broadcast_to(np.asarray(100.0 if hp is None else hp, np.float64), (len(alive),))
    for s, v in zip(alive, vals):
        assert 0.0 < v <= 100.0
        row[s] = v
    health[e, p, 8 * k:8 * k + SIZE[k]] = row
    cnt = len(alive)
    assert 0 <= stamp < TURN
    groups[e, p, k] = [node, -1 if moving_to is None else moving_to, 0 if moving_to is None else dist, 0, 0 if moving_to is None else 1, int(cnt == 0), cnt, stamp]


def stamp_of(e, p, k):
    """mixed arrival turns below TURN: (stamp, gid) order differs from gid order"""
    return (k * 5 + 3 * p + e) % 9


def hp_of(e, p, k, n):
    """healths in (0, 100] that are not all 100 (exact binary fractions and one that is not)"""
    vals = np.array([100.0, 62.5, 81.3, 100.0, 37.75, 93.0, 55.5, 100.0, 70.1, 48.0, 100.0, 66.6])
    return np.roll(vals, e + 3 * p + k)[:n]


def control(st, e, node, kind, side=0, cp=100):
    """kind 0: neutral, 1: held by `side`, 2: held by the other side, 3: partly captured by `side`, nobody holds it; cp: the node's control points.  The
    bases (nodes 1 and 11) keep their owners: a captured base would end the game."""
    nodes = st[1]
    assert node not in HOME and cp > 37
    sgn = (1 if side == 0 else -1)
    nodes[e, node - 1] = [[0, -1], [cp * sgn, side], [-cp * sgn, 1 - side], [37 * sgn, -1]][kind]


def concat(*states):
    return tuple(np.concatenate([s[i] for s in states], axis=0) for i in range(4))


def check_domain(st):
    """the rules of evg_set_state (csrc/evg_abi.hip evg_set_state) that a builder must keep"""
    groups, nodes, health, env = st
    for k in range(NG):
        h = health[:, :, 8 * k:8 * k + SIZE[k]]
        assert ((h == 0.0) | ((h > 0.0) & (h <= 100.0))).all()
        cnt = (h > 0).sum(axis=2)
        assert np.array_equal(cnt, groups[:, :, k, 6]) and np.array_equal(cnt == 0, groups[:, :, k, 5] != 0)
    g = groups
    assert ((g[..., 0] >= 1) & (g[..., 0] <= NN)).all() and (((g[..., 1] == -1) | ((g[..., 1] >= 1) & (g[..., 1] <= NN)))).all()
    assert ((g[..., 2] >= 0) & (g[..., 2] <= 7)).all() and not ((g[..., 3] != 0) & (g[..., 4] != 0)).any()
    assert ((g[..., 7] >= 0) & (g[..., 7] < TURN)).all() and (env[:, 0] == TURN).all() and (env[:, 1:] == 0).all()
    assert (np.abs(nodes[..., 0]) <= 511).all() and ((nodes[..., 1] >= -1) & (nodes[..., 1] <= 1)).all()
    assert (g[..., 6].sum(axis=2) > 0).all()                       # nobody is annihilated before the first turn


# ---------------------------------------------------------------------------------------------------------------- the census
def census(groups, envs_per_wave, four_lane=False):
    """Per wavefront of `envs_per_wave` envs (32: the two-lane kernel; 16: its 16-env form, or with four_lane the four-lane kernel), from evg_get_state group
    rows: a list of dicts
        items, nb, words, npass                                         of the whole wavefront
        passes: [dict(nitems, nb, words, rem_items, full_items, split_last, rounds, long_rounds)]
        groups: [(env, side, gid, alive, base, sh0)]                      of every fighting group"""
    groups = np.asarray(groups)
    N = groups.shape[0]
    cap = DP_CAP[(envs_per_wave, bool(four_lane))]
    loc, moving, cnt, stamp = groups[..., 0], groups[..., 4], groups[..., 6], groups[..., 7]
    elig = (cnt > 0) & (moving == 0)                                   # step_combat.inc:20 / evg_step4.inc:289: alive and not moving (server.py:525)
    words_ref = _pool_words(groups, envs_per_wave)
    out = []
    for w0 in range(0, N, envs_per_wave):
        lanes = []                                                     # one entry per (env, side) in lane order: step_combat.inc:76 packs its three counts
        rows = []
        for e in range(w0, min(w0 + envs_per_wave, N)):
            occ = [set(loc[e, p][elig[e, p]].tolist()) for p in range(NP)]
            contested = occ[0] & occ[1]                                # step_combat.inc:23 / evg_step4.inc:293 (server.py:539)
            for p in range(NP):
                order = sorted(range(NG), key=lambda k: (stamp[e, p, k], k))          # step_combat.inc:33: key = stamp << 21 | gid << 17 | ...
                tot = {}                                                              # alive fighting units of this side per node
                mine = []
                for k in order:
                    if elig[e, p, k] and loc[e, p, k] in contested:                   # step_combat.inc:47 (fightv)
                        n = int(loc[e, p, k])
                        mine.append((k, n, int(cnt[e, p, k]), tot.get(n, 0)))         # step_combat.inc:48: base = the returning add's old value
                        tot[n] = tot.get(n, 0) + int(cnt[e, p, k])
                ndw = sum((tot[n] + 3) >> 2 for n in tot)                             # step_combat.inc:66 / evg_step4.inc:352
                lanes.append(dict(env=e, side=p, fights=mine, tot=tot, ndw=ndw, nf_a=sum(k != 11 for k, _, _, _ in mine), nf_b=sum(k == 11 for k, _, _, _ in mine)))
        tot_d = sum(l["ndw"] for l in lanes)
        npass = 1 if tot_d <= cap else 2                                              # step_combat.inc:91 / evg_step4.inc:371
        half = envs_per_wave                                                          # lanes (env sides) of the first pass: step_combat.inc:95, :87 (mid)
        passes = []
        for ps in range(npass):
            mine = lanes if npass == 1 else [l for i, l in enumerate(lanes) if (i // half) == ps]
            na, nb = sum(l["nf_a"] for l in mine), sum(l["nf_b"] for l in mine)       # step_combat.inc:99-100
            nitems, ndwords = na + nb, sum(l["ndw"] for l in mine)
            rem_items = nitems & (WG - 1)                                             # step_combat.inc:148
            full_items = nitems - rem_items
            # step_combat.inc:147,149: only the 32-env form deals the sparse last round to two lanes per item; the four-lane kernel has no such round
            split_last = (envs_per_wave == 32 and not four_lane) and rem_items > 0 and rem_items <= WG // 2 and full_items >= nb
            rounds = -(-nitems // WG)
            # rounds whose items include a 12-unit group (second block of draws): listed FIRST by the two-lane kernel (step_combat.inc:102,109), LAST by the
            # four-lane kernel (evg_step4.inc:381,388)
            long_rounds = -(-nb // WG) if not four_lane else (rounds - na // WG if nb else 0)
            doff = 0
            for l in mine:                                                            # step_combat.inc:110-118: doff per lane and contested node, ascending
                for n in sorted(l["tot"]):
                    for k, node, c, base in l["fights"]:
                        if node == n:
                            rows.append((l["env"], l["side"], k, c, base, (doff * 4 + base) & 3))      # step_combat.inc:265 / evg_step4.inc:445
                    doff += (l["tot"][n] + 3) >> 2
            assert doff == ndwords
            passes.append(dict(nitems=nitems, nb=nb, words=ndwords, rem_items=rem_items, full_items=full_items, split_last=bool(split_last), rounds=rounds,
                               long_rounds=long_rounds))
        assert tot_d == words_ref[w0 // envs_per_wave]                                # the same count as tests/test_gpu_parity.py _pool_words
        out.append(dict(items=sum(l["nf_a"] + l["nf_b"] for l in lanes), nb=sum(l["nf_b"] for l in lanes), words=tot_d, npass=npass, passes=passes, groups=rows))
    return out


# ---------------------------------------------------------------------------------------------------------------- tables
def _copy_tables(evg_tables, oracle_mod):
    ot = oracle_mod.Tables()
    assert C.sizeof(ot) == C.sizeof(evg_tables)
    C.memmove(C.byref(ot), C.byref(evg_tables), C.sizeof(evg_tables))
    return ot


def _set_army(t, damage, type0_health, type0_groups):
    for u, d in enumerate(damage):
        t.unit_damage[u] = d
    t.unit_health[0] = type0_health
    for p in range(NP):
        for k in range(NG):
            t.group_type[p][k] = 0 if k in type0_groups else 1


def army_damage(t, p=0):
    return sum(SIZE[k] * t.unit_damage[t.group_type[p][k]] for k in range(NG))


def saturating_tables(make_tables, oracle_mod=None):
    """unit_damage (3, 2, 2), type 0 for groups 0-4 and 11, type 1 for the rest: an army deals 5*8*3 + 12*3 + 6*8*2 = 252, the largest total the
    damage byte admits (the total is a multiple of 4; evg_abi.hip build_dev_tables refuses more than 255).  Type 0 -- group 0 and group 11 -- has armor
    255, so a lone unit of it at a node nobody holds keeps 100 - 10 D / 255 after taking the summed damage D: the byte shows digit for digit."""
    t = make_tables()
    _set_army(t, (3, 2, 2), 255, (0, 1, 2, 3, 4, 11))
    assert army_damage(t, 0) == army_damage(t, 1) == 252
    return (t, _copy_tables(t, oracle_mod)) if oracle_mod is not None else t


def oversaturated_tables(make_tables):
    """one more group of type 0: 252 + 8 = 260, which evg_create must refuse"""
    t = make_tables()
    _set_army(t, (3, 2, 2), 255, (0, 1, 2, 3, 4, 5, 11))
    assert army_damage(t, 0) == 260
    return t


# ---------------------------------------------------------------------------------------------------------------- A: rounds of the work list
def _fight_at(st, e, gids0, gids1, node=6, kind=0, thin=False):
    """env e: the groups gids0 / gids1 of the two players stand at `node`; with `thin` a quarter of their units is dead"""
    for p, gids in enumerate((gids0, gids1)):
        for k in gids:
            n = SIZE[k] if not thin else SIZE[k] - 1 - (e + k + p) % 3
            put(st, e, p, k, node, alive=alive_slots(SIZE[k], n, e + k), stamp=stamp_of(e, p, k), hp=hp_of(e, p, k, n))
    control(st, e, node, kind, side=e & 1)


def _pick(e, p, n, with11):
    """n group ids; without group 11 they rotate through 0..10, with it group 11 is the first"""
    ids = [((e * 3 + p * 5 + j * 4) % 11) for j in range(11)]
    assert len(set(ids)) == 11
    return ([11] + ids[:n - 1]) if with11 else ids[:n]


A_WAVES = ["64", "65", "96", "97", "128", "129", "193", "768", "20+3", "20", "138"]
A_ITEMS = dict(zip(A_WAVES, [64, 65, 96, 97, 128, 129, 193, 768, 20, 20, 138]))
A_NB = dict(zip(A_WAVES, [0, 0, 0, 0, 0, 0, 16, 64, 3, 0, 64]))
A_RAGGED = 7


def family_a(waves=A_WAVES, ragged=A_RAGGED):
    """Waves of 32 envs whose two sides stand on node 6 with exactly the named number of fighting groups (= items of the work list) in all; in the first six
    group 11 is away (at home).  "193": 16 of the items are group 11's.  "768": every group of both sides, 4 units per side dead so that the pool stays
    below its cap (one pass).  "20+3": 10 envs fight with 2 items each, 3 of them group 11's (nb > 0 below one round: split_last off); "20": the same
    without group 11 (split_last on, nmain == 0).  "138": group 11 of both sides in every env (nb == 64) and 74 more.  Then a ragged wave of `ragged`
    envs, all fighting (3 + 3 groups)."""
    N = 32 * len(waves) + ragged
    st = blank(N)
    for w, name in enumerate(waves):
        for i in range(32):
            e = 32 * w + i
            if name in ("64", "65", "96", "97", "128", "129"):
                n = A_ITEMS[name] // 32 + (1 if i < A_ITEMS[name] % 32 else 0)
                _fight_at(st, e, _pick(e, 0, (n + 1) // 2, False), _pick(e, 1, n // 2, False), kind=i % 4, thin=(i % 3 == 1))
            elif name == "193":
                n = 6 + (1 if i == 0 else 0)
                _fight_at(st, e, _pick(e, 0, n - 3, False), _pick(e, 1, 3, i % 2 == 1), kind=i % 4, thin=(i % 3 == 1))
            elif name == "768":
                _fight_at(st, e, range(12), range(12), kind=i % 4)
                for p in range(NP):
                    for j in range(8):                                # 96 alive per side would be the pool's cap exactly; 8 dead keep this wave below it
                        k = (i + j + p) % 11
                        put(st, e, p, k, 6, alive=alive_slots(8, 7, e + j), stamp=stamp_of(e, p, k), hp=hp_of(e, p, k, 7))
            elif name in ("20+3", "20"):
                if i % 3 == 0 and i < 30:                             # envs 0, 3, .., 27 of the wave: 10 envs
                    with11 = name == "20+3" and i in (3, 12, 21)
                    _fight_at(st, e, _pick(e, 0, 1, with11 and i != 12), _pick(e, 1, 1, with11 and i == 12), kind=i % 4, thin=(i % 2 == 1))
            elif name == "138":
                n = 2 + (1 if i < 10 else 0)
                _fight_at(st, e, _pick(e, 0, 1 + (n + 1) // 2, True), _pick(e, 1, 1 + n // 2, True), kind=i % 4, thin=(i % 3 == 1))
            else:
                raise KeyError(name)
    for i in range(ragged):
        e = 32 * len(waves) + i
        _fight_at(st, e, _pick(e, 0, 3, i % 2 == 0), _pick(e, 1, 3, i % 3 == 0), kind=i % 4, thin=(i % 2 == 1))
    check_domain(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- B: the pool at its cap
def _thinned_army(st, e, p, alive, g11_alive, node, last_listed_11):
    """player p's whole army at `node` with `alive` units left, `g11_alive` of them in group 11; the dead are spread over groups 0..10 (each keeps a unit).
    last_listed_11: group 11 has the highest arrival stamp, so it is listed last (highest base) and its run ends the side's run of pool bytes"""
    dead = 88 - (alive - g11_alive)
    assert 0 <= dead <= 77
    lose = [dead // 11 + (1 if k < dead % 11 else 0) for k in range(11)]
    lose = lose[(e + p) % 11:] + lose[:(e + p) % 11]
    for k in range(11):
        n = 8 - lose[k]
        put(st, e, p, k, node, alive=alive_slots(8, n, e + k + p), stamp=min(stamp_of(e, p, k), 8 if last_listed_11 else 9), hp=hp_of(e, p, k, n))
    put(st, e, p, 11, node, alive=alive_slots(12, g11_alive, e + p), stamp=9 if last_listed_11 else stamp_of(e, p, 11), hp=hp_of(e, p, 11, g11_alive))


B_WAVES = ["cap, group 11 with 12 alive listed last", "cap, group 11 with 9 alive listed last", "cap + 1"]
B_RAGGED = 7


def family_b(envs_per_wave, alive_per_side, node=6, ragged=B_RAGGED):
    """Three wavefronts of `envs_per_wave` envs with `alive_per_side` units of each army on one node -- 96 for the two-lane kernels (24 words per side:
    32 x 48 = 1 536 = DP_CAP, 16 x 48 = 768 with 16 envs per wavefront), 80 for the four-lane kernel (16 x 40 = 640).  Waves 0 and 1 are AT the cap and in
    every env player 1's group 11 is listed last, with 12 and with 9 units alive: in the last env its run of damage bytes ends on the pool's last byte, and
    phase B's four-word read is clamped to DP_CAP - 1 (step_combat.inc:268 / evg_step4.inc:448).  In wave 2 one env of the second half has one unit more on
    one side: one word more, two passes.  Then a ragged wave, all fighting."""
    assert alive_per_side % 4 == 0
    N = 3 * envs_per_wave + ragged
    st = blank(N)
    for e in range(N):
        w, i = divmod(e, envs_per_wave)
        g11 = 9 if w == 1 else 12
        for p in range(NP):
            extra = 1 if (w == 2 and i == envs_per_wave // 2 + 4 and p == 0) else 0
            _thinned_army(st, e, p, alive_per_side + extra, g11, node, last_listed_11=True)
        control(st, e, node, e % 4, side=e & 1)
    check_domain(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- C: a saturated damage byte
C_CASES = ["group 0 slot 0", "group 11 slot 11", "two in one group", "two in two groups"]
C_PER_CASE = 8
C_RAGGED = 7


def c_survivors(case):
    """{gid: slots} of player 1's survivors"""
    return [{0: [0]}, {11: [11]}, {0: [2, 5]}, {0: [6], 11: [9]}][case]


def family_c(node=6, per_case=C_PER_CASE, ragged=C_RAGGED):
    """Player 0's whole army stands idle at `node` at full strength: 100 units that each draw one target among player 1's survivors there -- one or two
    units, so their damage bytes hold the whole army's damage between them (252 with saturating_tables(), 132 with the default army).  Env e is case
    e mod 4 of C_CASES; envs with e // 4 even have the node neutral (no structure defence), the others alternate between the two holders."""
    N = len(C_CASES) * per_case + ragged
    st = blank(N)
    for e in range(N):
        case, var = e % 4, e // 4
        for k in range(NG):
            put(st, e, 0, k, node, stamp=stamp_of(e, 0, k))
        for k in range(NG):
            slots = c_survivors(case).get(k, [])
            put(st, e, 1, k, node, alive=slots, stamp=stamp_of(e, 1, k), hp=100.0 if var % 3 else [100.0, 47.25][:len(slots)])
        control(st, e, node, 0 if var % 2 == 0 else 1 + (var // 2) % 2, side=1)
    # set_state wants a destroyed group somewhere sensible: it stays at the node, destroyed, as combat leaves it
    check_domain(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- D: exact kills
D_HEALTH = ["exact", "above", "below"]
D_CONTROL = ["neutral", "target's", "attacker's"]


def d_cases():
    """(target player, control, health, node) of env e: 2 x 3 x 3 = 18 combinations, on nodes 2..10 in turn, twice over and three more (39 envs: a wave and
    a ragged one of 7)"""
    return [(i % 2, (i // 2) % 3, (i // 6) % 3, 2 + (i * 4 + i // 18) % 9) for i in range(39)]


def d_pair(tables):
    """(attacking group, target group): the first group of a type that deals 1, the first group of a type with armor 3 (it differs from the attacker)"""
    att = [k for k in range(11) if tables.unit_damage[tables.group_type[0][k]] == 1]
    tgt = [k for k in range(11) if tables.unit_health[tables.group_type[0][k]] == 3]
    a = att[0]
    return a, [k for k in tgt if k != a][0]


def d_quotient(tables, node, control):
    """fl(10 * 8 / den), den = armor 3 (+ the node's defence where the target's side holds it, server.py:592-601)"""
    den = 3.0 + (tables.node_defense[node] if control == 1 else 0.0)
    return (10.0 * 8.0) / den


def family_d(tables):
    """One full 8-unit group of a damage-1 type attacks a lone unit of armor 3: all eight draws map to it (tot_o == 1), it takes 10 * 8 / den.  Its health is
    that quotient exactly (it must die: health <= 0, server.py:615), one float above (it must survive) or one float below (it dies)."""
    cases = d_cases()
    N = len(cases)
    st = blank(N)
    a, t = d_pair(tables)
    for e, (tp, ctl, hk, node) in enumerate(cases):
        q = d_quotient(tables, node, ctl)
        h = [q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf)][hk]
        put(st, e, 1 - tp, a, node, stamp=stamp_of(e, 1 - tp, a))
        put(st, e, tp, t, node, alive=[(e * 3) % 8], stamp=stamp_of(e, tp, t), hp=h)
        control(st, e, node, ctl, side=tp, cp=tables.node_control_points[node])
    check_domain(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- E: eleven contested nodes
E_WAVES = 3
E_RAGGED = 7


def family_e(waves=E_WAVES, ragged=E_RAGGED):
    """Group k of both players at node k + 1, group 11 at node 6 beside group 5; about 30 % of the units are dead, nobody is wiped out.  Node 6 lists two
    groups per side: in half of the variants group 5 comes first with 4..7 alive (group 11's run starts at byte 0, 1, 2, 3 of a pool word -- with 9, 10, 11
    and 12 alive), in the other half group 11 comes first with 9..12 alive (group 5's run starts at byte 1, 2, 3, 0).  Wave 0: everybody fights (768 items,
    64 of group 11).  Later waves: in some envs a group is in transit through its contested node and does not fight."""
    cnts = [4, 6, 7, 5, 4, 6, 8, 5, 4, 6]
    N = 32 * waves + ragged
    st = blank(N)
    for e in range(N):
        w, i = divmod(e, 32)
        for p in range(NP):
            v = (i + 13 * p) % 32
            if v < 16:
                a5, a11, first = 4 + v % 4, 9 + v // 4, 5
            else:
                a5, a11, first = 4 + (v // 4) % 4 + (1 if v % 4 == 3 else 0), 9 + v % 4, 11
            for k in range(11):
                n = a5 if k == 5 else cnts[(k + e + 3 * p) % 10]
                s = stamp_of(e, p, k)
                if k == 5:
                    s = 2 if first == 5 else 7
                put(st, e, p, k, k + 1, alive=alive_slots(8, n, e + k + p), stamp=s, hp=hp_of(e, p, k, n))
            put(st, e, p, 11, 6, alive=alive_slots(12, a11, e + p), stamp=7 if first == 5 else 2, hp=hp_of(e, p, 11, a11))
        for node in range(2, 11):
            control(st, e, node, (e + node) % 4, side=(e + node // 2) & 1)
        if w >= 1:
            groups = st[0]
            if i % 4 == 1:                    # group 5 of player 0 passes through node 6: group 11 still fights there
                groups[e, 0, 5, [1, 2, 4]] = [NEIGHBOUR[6], 2, 1]
            if i % 4 == 2:                    # group 2 of player 1 passes through node 3: nobody of player 1 fights there, the node is not contested
                groups[e, 1, 2, [1, 2, 4]] = [NEIGHBOUR[3], 1, 1]
            if i % 8 == 7:                    # group 11 of player 1 passes through node 6
                groups[e, 1, 11, [1, 2, 4]] = [NEIGHBOUR[6], 3, 1]
    check_domain(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- F: stock entropy
def melee(N, node=6):
    """all 24 groups at `node` at full health (the position of tests/test_gpu_parity.py _melee_state): every draw is randint(100), masked rejection"""
    st = blank(N)
    for e in range(N):
        for p in range(NP):
            for k in range(NG):
                put(st, e, p, k, node, stamp=stamp_of(e, p, k))
        control(st, e, node, e % 4, side=e & 1)
    check_domain(st)
    return st


F_MELEE = 9
# items per 32-env wavefront: C's 32 envs; 9 melee envs (24 each) + 23 envs of "65" (47); its other 9 envs (18) + 23 envs of "20+3" (16); its other 9
# envs (4) + the 5 ragged envs (6 each)
F_ITEMS = [424, 216 + 47, 18 + 16, 4 + 30]


def family_f():
    """for rng_mode="mt19937" (default tables): the one- and two-survivor positions of C (randint(1) consumes NO draw, oracle/evg_oracle.c mt_randint), a
    full melee, and two small waves of family A"""
    st = concat(family_c(ragged=0), melee(F_MELEE), family_a(waves=["65", "20+3"], ragged=5))
    check_domain(st)
    return st


# ---------------------------------------------------------------------------------------------------------------- what each family is built to reach
def _pass(nitems, nb, words=None):
    rem = nitems % WG
    d = dict(nitems=nitems, nb=nb, rem_items=rem, full_items=nitems - rem, rounds=-(-nitems // WG))
    if words is not None:
        d["words"] = words
    return d


# two-lane kernel, 32 envs per wavefront: (items, nb, split_last) written out, not derived
A_EXPECT = {"64": (64, 0, False), "65": (65, 0, True), "96": (96, 0, True), "97": (97, 0, False), "128": (128, 0, False), "129": (129, 0, True),
            "193": (193, 16, True), "768": (768, 64, False), "20+3": (20, 3, False), "20": (20, 0, True), "138": (138, 64, True)}
A_ROUNDS = {"64": 1, "65": 2, "96": 2, "97": 2, "128": 2, "129": 3, "193": 4, "768": 12, "20+3": 1, "20": 1, "138": 3}
A_RAGGED_EXPECT = (42, 7, False)


def _has(got, want):
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)


def expect_a(groups, waves=A_WAVES, ragged_expect=A_RAGGED_EXPECT):
    c = census(groups, 32)
    assert len(c) == len(waves) + 1
    for w, name in enumerate(waves):
        items, nb, split = A_EXPECT[name]
        assert (c[w]["items"], c[w]["nb"], c[w]["npass"]) == (items, nb, 1), (name, c[w]["items"], c[w]["nb"], c[w]["npass"])
        _has(c[w]["passes"][0], dict(_pass(items, nb), split_last=split, rounds=A_ROUNDS[name], long_rounds=-(-nb // 64)))
        assert c[w]["words"] <= 1536
    assert c[waves.index("768")]["words"] == 32 * 2 * 23 if "768" in waves else True
    if "20" in waves:
        p = c[waves.index("20")]["passes"][0]
        assert p["split_last"] and p["full_items"] == 0                        # nmain == 0: every item goes to a pair of lanes
    items, nb, split = ragged_expect
    assert (c[-1]["items"], c[-1]["nb"], c[-1]["npass"], c[-1]["passes"][0]["split_last"]) == (items, nb, 1, split)
    return c


def expect_b(groups, envs_per_wave, four_lane=False):
    cap = DP_CAP[(envs_per_wave, four_lane)]
    per_side = cap // envs_per_wave // 2                                       # words per side: 24, 24, 20
    c = census(groups, envs_per_wave, four_lane)
    assert [w["words"] for w in c] == [cap, cap, cap + 1, B_RAGGED * 2 * per_side] and [w["npass"] for w in c] == [1, 1, 2, 1]
    for w, g11 in ((0, 12), (1, 9)):                                           # the group listed last: last env, side 1, group 11, its run ends the pool
        env, side, gid, alive, base, sh0 = c[w]["groups"][-1]
        assert (env, side, gid, alive) == (envs_per_wave * (w + 1) - 1, 1, 11, g11) and base + alive == 4 * per_side and sh0 == (4 * per_side - g11) & 3
        assert max(r[4] for r in c[w]["groups"] if r[0] == env and r[1] == 1) == base
    first, second = c[2]["passes"]
    assert (first["words"], second["words"]) == (cap // 2, cap // 2 + 1)
    return c


def expect_c(groups):
    c = census(groups, 32)
    assert [(w["items"], w["nb"], w["words"], w["npass"]) for w in c] == [(424, 48, 832, 1), (92, 10, 7 * 26, 1)]
    for w in c:
        for env, side, gid, alive, base, sh0 in w["groups"]:
            if side == 1:
                assert alive == len(c_survivors(env % 4)[gid])
    return c


def expect_d(groups):
    c = census(groups, 32)
    assert [(w["items"], w["nb"], w["words"], w["npass"]) for w in c] == [(64, 0, 96, 1), (14, 0, 21, 1)]
    assert c[0]["passes"][0]["split_last"] is False and c[1]["passes"][0]["split_last"] is True
    return c


def expect_e(groups, waves=E_WAVES):
    c = census(groups, 32)
    assert (c[0]["items"], c[0]["nb"], c[0]["npass"]) == (768, 64, 1) and c[0]["passes"][0]["rounds"] == 12
    for w in range(1, waves):
        assert (c[w]["items"], c[w]["nb"], c[w]["npass"]) == (740, 60, 1)
    assert (c[-1]["items"], c[-1]["nb"], c[-1]["npass"]) == (162, 14, 1)
    rows = [r for w in c for r in w["groups"]]
    assert {r[5] for r in rows if r[2] != 11} == {0, 1, 2, 3}                                     # 8-unit groups: runs from every byte of a word
    assert {(r[3], r[5]) for r in rows if r[2] == 11} >= {(a, s) for a in (9, 10, 11, 12) for s in range(4)}
    for w in c[:1]:
        nodes_of = {}
        for env, side, gid, alive, base, sh0 in w["groups"]:
            nodes_of.setdefault(env, set()).add(6 if gid == 11 else gid + 1)
        assert all(v == set(range(1, 12)) for v in nodes_of.values()) and len(nodes_of) == 32     # all eleven nodes contested in every env
    return c
