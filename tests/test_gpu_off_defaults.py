"""GPU tests of every step form off the defaults the rest of the suite sets (tests/off_default_cases.py; the CPU half is tests/test_off_default_cases.py):

  A. wide keys: every handle has a seed whose high word is in use and env ids that end at 0xFFFFFFFF -- the plain turn, the persistent rollouts of the
     three kernels, the bots that draw, the exploring decodes, the leagues, a checkpoint -- against the oracle, the host models and the pinned compositions;
  B. every one-turn form in every observation type: three handles, one per type, on the same games and inputs, equal on every turn;
  C. in B's runs every caller-supplied output is a view into a larger sentinel-filled allocation: the elements around it stay untouched;
  D. the replay memory's sample(): the drawn handles equal the host model's (tests/replay_model.py ReplayModel.draw), draw for draw.

All comparisons are exact equality, except rewards against the oracle's float64 (REWARD_ATOL of tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import minimized_model as mm
import off_default_cases as cases
from test_gpu_league import _Composition, _same_end_state, _same_outputs
from test_gpu_minimized_self_play import _Buffers, _LeagueComposition, _same_handles, _same_league, _same_turn
from test_gpu_parity import REWARD_ATOL, check_state
from test_gpu_replay import run_loop

pytestmark = pytest.mark.gpu

SEED = cases.SEED
GUARD = 64
OBS_FILL, ROW_FILL, FLAG_FILL = -7, -5, 9           # no feature, order row or flag has these values; an observation has -7 in one column only, see _Guarded


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


def _env(evg, n, **kw):
    return evg.EvergladesVecEnv(n, seed=SEED, env_id_base=cases.base_for(n), **kw)


def _oracle(oracle_mod, n, **kw):
    return oracle_mod.Oracle(n, seed=SEED, env_id_base=cases.base_for(n), **kw)


def _ids(n):
    return (cases.base_for(n) + np.arange(n)).astype(np.uint32)


def _same_step(got, want, seat, what):
    """a device turn against the oracle's: observation (of one seat, or of both with seat=None), scores, status, winner, done, rewards"""
    (obs, rew, done, info), (o_obs, o_rew, o_done, o_info) = got, want
    assert np.array_equal(_np(obs).astype(np.float64), o_obs if seat is None else o_obs[:, seat]), (what, "obs")
    assert np.array_equal(_np(info["scores"]), o_info["scores"]) and np.array_equal(_np(info["status"]), o_info["status"]), (what, "scores / status")
    assert np.array_equal(_np(info["winner"]), o_info["winner"]) and np.array_equal(_np(done), o_done), (what, "winner / done")
    assert np.allclose(_np(rew), o_rew, rtol=0, atol=REWARD_ATOL), (what, "reward")


def _same_stats(env, ora):
    st, ost = env.episode_stats(), ora.episode_stats()
    assert np.array_equal(st["totals"], ost["totals"]) and np.array_equal(st["winner"], ost["winner"])
    assert np.array_equal(st["length"], ost["length"]) and np.allclose(st["returns"], ost["returns"], rtol=1e-6, atol=1e-5)


# ---------------------------------------------------------------------------------------------- A1: the plain turn
@pytest.mark.parametrize("N", cases.SIZES)
def test_plain_turn_equals_the_oracle(evg, oracle_mod, N):
    """the body of test_gpu_parity.py's test_random_rollout_vs_oracle: full random-vs-random episodes and two frozen turns"""
    env, ora = _env(evg, N, auto_reset=False), _oracle(oracle_mod, N)
    assert np.array_equal(_np(env.reset()).astype(np.float64), ora.reset())
    for t in range(152):
        a = env.random_actions()
        assert np.array_equal(_np(a), ora.random_actions()), ("action generator", t)
        _same_step(env.step(a), ora.step(_np(a)), None, t)
        if t % 25 == 0 or t >= 149:
            check_state(env, ora.get_state(), t)
            assert np.array_equal(_np(env.fog_of_war()), ora.fog_of_war()) and np.array_equal(_np(env.knowledge()), ora.knowledge()), t
            assert np.array_equal(_np(env.sightings()), ora.sightings()), t
    _same_stats(env, ora)
    assert bool(env.done.all())
    env.close()


def test_a_handle_whose_ids_end_at_the_top_of_the_range_is_created_and_plays(evg, oracle_mod):
    """env_id_base + num_envs == 2^32 is accepted (one env more is refused: tests/test_abi_and_host.py asserts that half), down to a single env with the
    id 0xFFFFFFFF"""
    for n in (1, 37):
        env, ora = _env(evg, n, auto_reset=False), _oracle(oracle_mod, n)
        assert env.env_id_base + env.num_envs == 2 ** 32
        assert np.array_equal(_np(env.reset()).astype(np.float64), ora.reset())
        for t in range(3):
            a = env.random_actions()
            assert np.array_equal(_np(a), ora.random_actions()), (n, t)
            _same_step(env.step(a), ora.step(_np(a)), None, (n, t))
        env.close()


# ---------------------------------------------------------------------------------------------- A2: persistent rollouts, three kernels
def _persistent_rollout_vs_oracle(evg, oracle_mod, N, **env_kw):
    """One launch of 146 turns, then 8 launches of 5 turns compared with the oracle after every launch (its last turn: observations, reward, done, scores,
    recorded orders): the random games end at turn 150, inside the second compared launch, so the later ones draw with episode counters above 0."""
    tpl, launches, lead = 5, 8, 146
    env = _env(evg, N, auto_reset=True, **env_kw)
    ora = _oracle(oracle_mod, N, auto_reset=True)
    assert np.array_equal(_np(env.reset()).astype(np.float64), ora.reset())
    env.rollout_random(lead, turns_per_launch=lead)
    for t in range(lead):
        ora.step_noobs(ora.random_actions())
    for k in range(launches):
        out = env.rollout_random(tpl, turns_per_launch=tpl)
        for t in range(tpl):
            acts = ora.random_actions()
            o_obs, o_rew, o_done, o_info = ora.step(acts)
        assert np.array_equal(_np(out[0]).astype(np.float64), o_obs), ("obs", k)
        assert np.allclose(_np(out[1]), o_rew, rtol=0, atol=REWARD_ATOL), ("reward", k)
        assert np.array_equal(_np(out[2]), o_done), ("done", k)
        assert np.array_equal(_np(out[3]["scores"]), o_info["scores"]), ("scores", k)
        assert np.array_equal(_np(env._actions), acts), ("recorded orders", k)
    check_state(env, ora.get_state(), "persistent")
    assert (ora.get_state()["env"][:, 2] > 0).all()                        # every env is in a later episode by now
    _same_stats(env, ora)
    assert env.check_fault() == 0
    env.close()


def test_persistent_rollout_of_the_four_lane_kernel_equals_the_oracle(evg, oracle_mod):
    """the product library plays so few envs with four lanes per env: the kernel that takes the key's high word as an argument of its own"""
    env = _env(evg, 77)
    assert "four lanes" in env.launch_plan(5)[1]
    env.close()
    _persistent_rollout_vs_oracle(evg, oracle_mod, 77)


@pytest.mark.parametrize("N,lanes", [(77, 64), (64, 32)])
def test_persistent_rollout_of_the_two_lane_kernels_equals_the_oracle(evg, oracle_mod, N, lanes):
    """the diagnostic library's forced two-lanes-per-env kernel (the flagship's; its keys come from the key table) and its 16-envs-per-wavefront form"""
    _persistent_rollout_vs_oracle(evg, oracle_mod, N, library=evg._lib.DIAG_LIB_PATH, diag=dict(lanes=lanes))


# ---------------------------------------------------------------------------------------------- A3: bots that draw
DRAWING_BOTS = ["random_actions_delay", "random_actions", "swarm_agent"]       # the delay coin, the action rows, the swarm shuffle


@pytest.mark.parametrize("bot", DRAWING_BOTS)
def test_learner_seat_turn_against_a_drawing_bot_equals_the_oracle(evg, oracle_mod, bot):
    """step_vs with the bot inside the step kernel, the caller's rows from random_actions_seat: 160 turns with auto-reset on both seats (37 envs with the
    caller on seat 0, 70 with the caller on seat 1) against the oracle's scripted_actions + step"""
    pid = evg.EvergladesVecEnv.POLICIES[bot]
    for seat, N in enumerate(cases.SIZES):
        env, ora = _env(evg, N, auto_reset=True), _oracle(oracle_mod, N, auto_reset=True)
        env.reset()
        o_obs = ora.reset()
        oa = np.zeros((N, 2, 7, 2), np.int32)
        for t in range(160):
            rows = env.random_actions_seat(seat)
            want_rows = ora.random_actions()[:, seat]
            assert np.array_equal(_np(rows), want_rows), (bot, seat, t, "caller's rows")
            ora.scripted_actions(pid, 1 - seat, o_obs, oa)
            oa[:, seat] = want_rows
            got = env.step_vs(bot, rows, seat=seat)
            want = ora.step(oa)
            _same_step(got, want, seat, (bot, seat, t))
            o_obs = want[0]
        check_state(env, ora.get_state(), (bot, seat))
        _same_stats(env, ora)
        assert int(env.episode_stats()["totals"][0]) >= N
        env.close()


@pytest.mark.parametrize("seats", [("random_actions_delay", "swarm_agent"), ("swarm_agent", "random_actions")])
def test_persistent_rollout_of_drawing_bots_equals_the_oracle(evg, oracle_mod, seats):
    """rollout_policies, bots fused into the persistent kernel, 4 launches of 40 turns: the last turn's observations and orders, the state, the episodes"""
    N = 77
    pid = [evg.EvergladesVecEnv.POLICIES[s] for s in seats]
    env, ora = _env(evg, N, auto_reset=True), _oracle(oracle_mod, N, auto_reset=True)
    env.reset()
    o_obs = ora.reset()
    env.rollout_policies(160, seats[0], seats[1], fused=True, turns_per_launch=40)
    for t in range(160):
        oa = np.zeros((N, 2, 7, 2), np.int32)
        ora.scripted_actions(pid[0], 0, o_obs, oa)
        ora.scripted_actions(pid[1], 1, o_obs, oa)
        o_obs, o_rew, o_done, o_info = ora.step(oa)
    assert np.array_equal(_np(env.obs).astype(np.float64), o_obs) and np.array_equal(_np(env._actions), oa)
    assert np.array_equal(_np(env.scores), o_info["scores"]) and np.array_equal(_np(env.done), o_done)
    check_state(env, ora.get_state(), seats)
    _same_stats(env, ora)
    assert int(env.episode_stats()["totals"][0]) >= N
    env.close()


# ---------------------------------------------------------------------------------------------- A4: exploring decodes
def _q_grid(torch, shape, gen):
    """values on a grid of halves: exact ties within a swarm and between swarms are common"""
    return (torch.randn(shape, generator=gen) * 2.0).round().div(2.0)


def _midgame(evg, oracle_mod, N, turns=146):
    """a handle and an oracle `turns` random turns into their games (the games end at turn 150: a few turns later every env is in episode 1)"""
    env, ora = _env(evg, N, auto_reset=True), _oracle(oracle_mod, N, auto_reset=True)
    env.reset(), ora.reset()
    env.rollout_random(turns, turns_per_launch=turns)
    for t in range(turns - 1):
        ora.step_noobs(ora.random_actions())
    o_obs = ora.step(ora.random_actions())[0]
    assert np.array_equal(_np(env.obs).astype(np.float64), o_obs)
    return env, ora, o_obs


def _decode(oracle_mod, head, q, obs_rows, ids, state_env, seat, eps):
    """(rows, directions or None, explored) of one seat's get_action: the oracle's for the 5-way head, the host model's for the 11-way head"""
    episodes = state_env[:, 2].astype(np.uint32)
    if head == 5:
        return oracle_mod.smart_get_action(np.ascontiguousarray(q), np.ascontiguousarray(obs_rows), SEED, ids, episodes, seat, eps)
    rows, ex = mm.get_action(q, SEED, ids, episodes, state_env[:, 0], seat, eps)
    return rows, None, ex


@pytest.mark.parametrize("head", [5, 11])
@pytest.mark.parametrize("N", cases.SIZES)
def test_exploring_decodes_equal_the_oracle_and_the_host_model(evg, oracle_mod, N, head):
    """smart_get_action / minimized_get_action, step_vs_q and step_q with epsilon per env from 0 to 1, over the end of episode 0 and the start of episode
    1: rows, directions (5-way) and explored flags against oracle.smart_get_action / minimized_model.get_action, the game against the oracle stepped with
    those rows (the other seat of step_vs_q: the swarm bot, which draws too).  Both values of `explored` occur on each seat."""
    import torch
    ids = _ids(N)
    gen = torch.Generator(device="cpu").manual_seed(N + head)
    eps_np = np.stack([np.linspace(0.0, 1.0, N), np.linspace(1.0, 0.0, N)], 1).astype(np.float32)
    seen = np.zeros((3, 2, 2), bool)                                      # [entry point][seat][explored]
    bot = "swarm_agent"
    pid = evg.EvergladesVecEnv.POLICIES[bot]
    # the decode alone, and the learner-seat turn
    for seat in (0, 1):
        env, ora, o_obs = _midgame(evg, oracle_mod, N)
        dev = env.device
        eps = torch.as_tensor(eps_np[:, seat].copy(), device=dev)
        rows = torch.full((N, 7, 2), ROW_FILL, dtype=torch.int32, device=dev)
        dirs = torch.full((N, 7, 2), ROW_FILL, dtype=torch.int32, device=dev)
        ex = torch.full((N,), FLAG_FILL, dtype=torch.uint8, device=dev)
        oa = np.zeros((N, 2, 7, 2), np.int32)
        sobs = env.observe_seat(seat)
        for t in range(12):
            q = _q_grid(torch, (N, 12, head), gen)
            want = _decode(oracle_mod, head, q.numpy(), o_obs[:, seat], ids, ora.get_state()["env"], seat, eps_np[:, seat])
            if t == 0 or t == 6:                                           # (turn 146, and turn 2 of the next episode)
                if head == 5:
                    env.smart_get_action(q.to(dev), eps, seat=seat, obs=sobs, out=rows, directions=dirs, explored=ex)
                    assert np.array_equal(_np(dirs), want[1]), (seat, t, "directions, decode alone")
                else:
                    env.minimized_get_action(q.to(dev), eps, seat=seat, out=rows, explored=ex)
                assert np.array_equal(_np(rows), want[0]) and np.array_equal(_np(ex), want[2]), (seat, t, "decode alone")
                seen[0, seat, 0] |= bool((want[2] == 0).any())
                seen[0, seat, 1] |= bool((want[2] == 1).any())
                rows.fill_(ROW_FILL), dirs.fill_(ROW_FILL), ex.fill_(FLAG_FILL)
            got = env.step_vs_q(bot, q.to(dev), eps, seat=seat, directions=dirs if head == 5 else None, explored=ex, actions_out=rows)
            assert np.array_equal(_np(rows), want[0]) and np.array_equal(_np(ex), want[2]), (seat, t, "step_vs_q")
            if head == 5:
                assert np.array_equal(_np(dirs), want[1]), (seat, t, "step_vs_q directions")
            seen[1, seat, 0] |= bool((want[2] == 0).any())
            seen[1, seat, 1] |= bool((want[2] == 1).any())
            ora.scripted_actions(pid, 1 - seat, o_obs, oa)
            oa[:, seat] = want[0]
            o_step = ora.step(oa)
            _same_step(got, o_step, seat, (seat, t, "step_vs_q"))
            o_obs, sobs = o_step[0], got[0]
        assert (ora.get_state()["env"][:, 2] > 0).all()
        check_state(env, ora.get_state(), ("step_vs_q", seat))
        env.close()
    # the self-play turn
    env, ora, o_obs = _midgame(evg, oracle_mod, N)
    dev = env.device
    eps = torch.as_tensor(eps_np, device=dev)
    rows = torch.full((N, 2, 7, 2), ROW_FILL, dtype=torch.int32, device=dev)
    dirs = torch.full((N, 2, 7, 2), ROW_FILL, dtype=torch.int32, device=dev)
    ex = torch.full((N, 2), FLAG_FILL, dtype=torch.uint8, device=dev)
    for t in range(12):
        q = _q_grid(torch, (N, 2, 12, head), gen)
        st = ora.get_state()["env"]
        want = [_decode(oracle_mod, head, q[:, p].numpy(), o_obs[:, p], ids, st, p, np.ascontiguousarray(eps_np[:, p])) for p in range(2)]
        got = env.step_q(q.to(dev), eps, directions=dirs if head == 5 else None, explored=ex, actions_out=rows)
        for p in range(2):
            assert np.array_equal(_np(rows[:, p]), want[p][0]) and np.array_equal(_np(ex[:, p]), want[p][2]), (p, t, "step_q")
            if head == 5:
                assert np.array_equal(_np(dirs[:, p]), want[p][1]), (p, t, "step_q directions")
            seen[2, p, 0] |= bool((want[p][2] == 0).any())
            seen[2, p, 1] |= bool((want[p][2] == 1).any())
        o_step = ora.step(np.stack([want[0][0], want[1][0]], axis=1))
        _same_step(got, o_step, None, (t, "step_q"))
        o_obs = o_step[0]
    assert (ora.get_state()["env"][:, 2] > 0).all()
    check_state(env, ora.get_state(), "step_q")
    env.close()
    assert seen.all()


# ---------------------------------------------------------------------------------------------- A5: the leagues
def _league_rows(torch, n, gen):
    g = torch.randint(0, 12, (n, 7, 1), generator=gen, dtype=torch.int32)
    d = torch.randint(1, 12, (n, 7, 1), generator=gen, dtype=torch.int32)
    return torch.cat([g, d], dim=2).contiguous()


@pytest.mark.parametrize("seat", [0, 1])
@pytest.mark.parametrize("form", ["step_vs", "step_vs_q 5-way", "step_vs_q 11-way"])
def test_one_seat_league_turns_equal_the_composition(evg, seat, form):
    """step_vs / step_vs_q with a league of bots against tests/test_gpu_league.py's composition (scripted_actions per member with its objects moved in and
    out, step, the host model lm.League(SEED, base, ...) deciding assignment, tally and swap); the Q forms' rows are decoded on the composition's handle by
    smart_get_action / minimized_get_action.  cases.TURNS turns at 37 envs: the episodes tests/test_off_default_cases.py looked at."""
    import torch
    N, base = 37, cases.base_for(37)
    members, weights = cases.LEAGUES["bots"]
    env = _env(evg, N, auto_reset=True)
    env.reset()
    league = env.opponent_league(members, weights=weights, seat=seat)
    comp = _Composition(evg, N, seat, "float32", members, weights, True, seed=SEED, env_id_base=base)
    dev = env.device
    gen = torch.Generator(device="cpu").manual_seed(3 + seat)
    feat = (torch.full((N, 34), float(OBS_FILL), device=dev), torch.full((N, 12, 13), float(OBS_FILL), device=dev))
    out_a = [torch.full((N, 7, 2), ROW_FILL, dtype=torch.int32, device=dev) for _ in range(2)] + [torch.full((N,), FLAG_FILL, dtype=torch.uint8, device=dev)]
    out_b = [torch.full((N, 7, 2), -3, dtype=torch.int32, device=dev) for _ in range(2)] + [torch.full((N,), 8, dtype=torch.uint8, device=dev)]
    eps_env = torch.linspace(0.0, 1.0, N).to(dev)
    prev = comp.env.observe_seat(seat).clone()
    assert np.array_equal(_np(league.assign), comp.model.assign)
    for t in range(cases.TURNS):
        features = feat if t % 2 else None
        eps = eps_env if t % 3 == 0 else 0.1
        if form == "step_vs":
            rows = _league_rows(torch, N, gen).to(dev)
            got = env.step_vs(league, rows, features=features)
        elif form == "step_vs_q 5-way":
            q = _q_grid(torch, (N, 12, 5), gen).to(dev)
            got = env.step_vs_q(league, q, eps, seat=seat, features=features, actions_out=out_a[0], directions=out_a[1], explored=out_a[2])
            rows = comp.env.smart_get_action(q, eps, seat=seat, obs=prev, out=out_b[0], directions=out_b[1], explored=out_b[2])
        else:
            q = _q_grid(torch, (N, 12, 11), gen).to(dev)
            got = env.step_vs_q(league, q, eps, seat=seat, features=features, actions_out=out_a[0], explored=out_a[2])
            rows = comp.env.minimized_get_action(q, eps, seat=seat, out=out_b[0], explored=out_b[2])
        want = comp.step(rows)
        _same_outputs(torch, got, want, t)
        if form != "step_vs":
            assert torch.equal(out_a[0], out_b[0]) and torch.equal(out_a[2], out_b[2]), (t, "rows / explored")
            if form == "step_vs_q 5-way":
                assert torch.equal(out_a[1], out_b[1]), (t, "directions")
        if features is not None:
            s2, w2 = env.smart_state_compact(-1, got[0])
            assert torch.equal(feat[0], s2) and torch.equal(feat[1], w2), (t, "features")
        if t % 10 == 9 or bool(got[2].any()):
            assert np.array_equal(_np(league.assign), comp.model.assign), t
        prev = want[0].contiguous()
    h = comp.model.history
    assert min(len(a) for a in h) >= cases.EPISODES
    assert [a[:cases.EPISODES] for a in h] == cases.model_histories(N, seat, "bots")
    _same_end_state(env, league, comp)
    assert int(league.counts[:, 0].sum()) == int(env.episode_stats()["totals"][0]) >= (cases.EPISODES - 1) * N
    env.close(), comp.env.close()


@pytest.mark.parametrize("seat", [0, 1])
def test_self_play_league_turn_with_a_network_member_equals_the_composition(evg, seat):
    """step_q(league=...) with a "q" member against tests/test_gpu_minimized_self_play.py's composition and lm.League(SEED, base, ...)"""
    import torch
    N, base = 37, cases.base_for(37)
    members, weights = cases.LEAGUES["q"]
    env = _env(evg, N, auto_reset=True)
    env.reset()
    league = env.opponent_league(members, weights=weights, seat=seat)
    assert league.q_member == members.index("q")
    comp = _LeagueComposition(evg, N, seat, "float32", members, weights, seed=SEED, env_id_base=base)
    dev = env.device
    ga, gb = _Buffers(torch, N, dev, OBS_FILL), _Buffers(torch, N, dev, ROW_FILL)
    eps_env = torch.stack([torch.linspace(0.0, 1.0, N), torch.linspace(1.0, 0.0, N)], dim=1).contiguous().to(dev)
    gen = torch.Generator(device="cpu").manual_seed(N + seat)
    assert np.array_equal(_np(league.assign), comp.model.assign)
    twos = 0
    for t in range(cases.TURNS):
        q = _q_grid(torch, (N, 2, 12, 11), gen).to(dev)
        eps = eps_env if t % 2 else (0.3, 0.1)
        features = t % 3 != 0
        got = env.step_q(q, eps, features=ga.feat if features else None, explored=ga.ex, actions_out=ga.rows, league=league)
        want = comp.step(q, eps, gb, features)
        _same_turn(torch, got, want, ga, gb, features, (seat, t))
        twos += int((ga.ex[:, 1 - seat] == 2).sum().item())
        if t % 10 == 9 or bool(got[2].any()):
            assert np.array_equal(_np(league.assign), comp.model.assign), t
    h = comp.model.history
    assert min(len(a) for a in h) >= cases.EPISODES
    assert [a[:cases.EPISODES] for a in h] == cases.model_histories(N, seat, "q")
    assert 0 < twos == comp.bot_played < N * cases.TURNS
    _same_handles(env, comp.env, comp.agents())
    _same_league(league, comp)
    assert int(league.counts[:, 0].sum()) == int(env.episode_stats()["totals"][0]) >= (cases.EPISODES - 1) * N
    env.close(), comp.env.close()


# ---------------------------------------------------------------------------------------------- A7: checkpoint
def test_checkpoint_of_a_wide_key_handle_resumes_bit_for_bit(evg):
    """one case of test_gpu_parity.py's test_checkpoint_resume_continues_bit_for_bit, learner-seat mode: saved at turn 140, the 40 turns that follow run
    over the end of the episode, against a bot that draws"""
    N = 37

    def play(env, turns):
        for _ in range(turns):
            sobs, rew, done, info = env.step_vs("random_actions_delay", env.random_actions_seat(1), seat=1)
        return _np(sobs).copy(), _np(rew).copy(), _np(env._actions_seat).copy()
    a = _env(evg, N, auto_reset=True)
    a.reset()
    play(a, 140)
    ck = a.checkpoint()
    want = play(a, 40)
    want_state, want_stats = a.get_state(), a.episode_stats()
    b = _env(evg, N, auto_reset=True)
    b.reset()
    play(b, 3)                                                             # a history of its own before the restore
    b.restore(ck)
    got = play(b, 40)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    check_state(b, want_state, "restored")
    st = b.episode_stats()
    for k in ("returns", "length", "winner", "totals"):
        assert np.array_equal(st[k], want_stats[k]), k
    assert int(st["totals"][0]) >= N
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------- B and C: every form, every observation type, guarded
class _Guarded(object):
    """a caller's output as a view into a larger allocation filled with a sentinel, GUARD elements in front of it and GUARD behind (the view stays 16-byte
    aligned: GUARD elements of every type used here are a multiple of 16 bytes)"""

    def __init__(self, torch, shape, dtype, fill, dev):
        self.n, self.fill = int(np.prod(shape)), fill
        self.big = torch.full((2 * GUARD + self.n,), fill, dtype=dtype, device=dev)
        self.view = self.big[GUARD:GUARD + self.n].view(shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()

    def refill(self):
        self.big.fill_(self.fill)

    def guards_untouched(self):
        return bool((self.big[:GUARD] == self.fill).all()) and bool((self.big[GUARD + self.n:] == self.fill).all())

    def left(self):
        """bool array: where the view still holds the sentinel"""
        return _np(self.view == self.fill)


# form -> (two seats, head, league): the nine one-turn forms the step-kernel dispatch builds, each once per observation type
FORMS = {"step_vs": (False, None, None), "step_vs_q 5-way": (False, 5, None), "step_q 5-way": (True, 5, None),
         "step_vs league": (False, None, "bots"), "step_vs_q 5-way league": (False, 5, "bots"),
         "step_vs_q 11-way": (False, 11, None), "step_vs_q 11-way league": (False, 11, "bots"),
         "step_q 11-way": (True, 11, None), "step_q 11-way league": (True, 11, "q")}
DTYPES = ("float32", "float64", "int16")
CONTROL_COLUMNS = list(range(3, 45, 4))            # a node's control state: the one signed field of an observation


class _Side(object):
    """one handle of a form's run: its league and its guarded outputs"""

    def __init__(self, evg, torch, form, N, seat, dtype):
        self.two, self.head, lg = FORMS[form]
        self.torch, self.N, self.seat = torch, N, seat
        self.env = env = _env(evg, N, obs_dtype=dtype, auto_reset=True)
        env.reset()
        self.league = env.opponent_league(cases.LEAGUES[lg][0], weights=cases.LEAGUES[lg][1], seat=seat) if lg else None
        dev, lead = env.device, ((N, 2) if self.two else (N,))
        self.obs = _Guarded(torch, lead + (105,), env.obs_dtype, OBS_FILL, dev)
        self.shared = _Guarded(torch, lead + (34,), torch.float32, float(OBS_FILL), dev)
        self.swarm = _Guarded(torch, lead + (12, 13), torch.float32, float(OBS_FILL), dev)
        self.rows = _Guarded(torch, lead + (7, 2), torch.int32, ROW_FILL, dev) if self.head else None
        self.dirs = _Guarded(torch, lead + (7, 2), torch.int32, ROW_FILL, dev) if self.head == 5 else None
        self.ex = _Guarded(torch, lead, torch.uint8, FLAG_FILL, dev) if self.head else None

    def outputs(self):
        return [(k, g) for k, g in (("obs", self.obs), ("shared", self.shared), ("swarm", self.swarm), ("rows", self.rows), ("directions", self.dirs),
                                    ("explored", self.ex)) if g is not None]

    def turn(self, x, eps, features):
        env = self.env
        feat = (self.shared.view, self.swarm.view) if features else None
        if self.two:
            return env.step_q(x, eps, features=feat, directions=self.dirs.view if self.dirs else None, explored=self.ex.view, actions_out=self.rows.view,
                              out=self.obs.view, league=self.league)
        policy = self.league if self.league is not None else "random_actions_delay"
        if self.head is None:
            return env.step_vs(policy, x, seat=self.seat, out=self.obs.view, features=feat)
        return env.step_vs_q(policy, x, eps, seat=self.seat, features=feat, directions=self.dirs.view if self.dirs else None, explored=self.ex.view,
                             actions_out=self.rows.view, out=self.obs.view)

    def check_guards(self, features, what):
        """both guards of every output untouched; no sentinel inside what the turn writes in full, the features only sentinels where they were not asked
        for.  An observation may show -7 as a node's control state (a signed count of control points): there, and only there, a -7 is accepted, if the
        handle's state has that value (a turn that ends a game shows the next episode's first observation, so the state is the observation's)."""
        for k, g in self.outputs():
            assert g.guards_untouched(), (what, k, "guard elements changed")
            left = g.left()
            if k in ("shared", "swarm") and not features:
                assert left.all(), (what, k, "written without being asked for")
            elif k == "obs":
                rest = np.delete(left, CONTROL_COLUMNS, axis=-1)
                assert not rest.any(), (what, k, "sentinel left inside")
                ctl = left[..., CONTROL_COLUMNS]
                if ctl.any():
                    state = self.env.get_state()["nodes"][:, :, 0] == OBS_FILL                 # [N, 11]
                    assert not (ctl & ~(state[:, None, :] if self.two else state)).any(), (what, k, "sentinel left inside (control state)")
            else:
                assert not left.any(), (what, k, "sentinel left inside")


def _run_form(evg, form, N, seat, turns):
    import torch
    two, head, lg = FORMS[form]
    sides = [_Side(evg, torch, form, N, seat, dt) for dt in DTYPES]
    dev = sides[0].env.device
    gen = torch.Generator(device="cpu").manual_seed(1000 + N)
    lead = (N, 2) if two else (N,)
    if two:
        eps_env = torch.stack([torch.linspace(0.0, 1.0, N), torch.linspace(1.0, 0.0, N)], dim=1).contiguous().to(dev)
    else:
        eps_env = torch.linspace(0.0, 1.0, N).to(dev)
    ends = 0
    for t in range(turns):
        x = (_league_rows(torch, N, gen) if head is None else _q_grid(torch, lead + (12, head), gen)).to(dev)
        eps = eps_env if t % 2 else ((0.3, 0.1) if two else 0.3)
        features = t % 3 != 0
        checked = t < 3 or t == turns - 1
        outs = []
        for s in sides:
            if checked:
                for _, g in s.outputs():
                    g.refill()
            outs.append(s.turn(x, eps, features))
            if checked:
                s.check_guards(features, (form, N, s.env.obs_dtype, t))
        ref, f64 = sides[1], outs[1]
        assert f64[0].dtype == torch.float64
        for s, o in zip(sides, outs):
            what = (form, N, s.env.obs_dtype, t)
            assert torch.equal(o[0].to(torch.float64), f64[0]), (what, "obs")
            assert torch.equal(o[1], f64[1]) and torch.equal(o[2], f64[2]), (what, "reward / done")
            for k in ("winner", "scores", "status"):
                assert torch.equal(o[3][k], f64[3][k]), (what, k)
            for k, g in s.outputs():
                if k == "obs" or (k in ("shared", "swarm") and not features):
                    continue
                assert torch.equal(g.view, dict(ref.outputs())[k].view), (what, k)
        ends += int(f64[2].sum().item())
    states = [(s.env.get_state(), s.env.get_run_state(), s.league.state() if s.league is not None else {}) for s in sides]
    for st, s in zip(states, sides):
        for a, b in zip(st, states[1]):
            assert sorted(a) == sorted(b)
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (form, N, s.env.obs_dtype, "end state", k)
    for s in sides:
        s.env.close()
    return ends


@pytest.mark.parametrize("N", cases.SIZES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_form_plays_the_same_games_in_every_observation_type(evg, form, N):
    """160 turns with auto-reset on three handles (float32, float64, int16; the same seed, id base and inputs), the caller on seat 0 at 37 envs and on seat
    1 at 70: observations equal as float64, everything else bit for bit on every turn, then the state, the run state and the league's state.  Every
    caller-supplied output is guarded (_Guarded) and checked on the first three turns and the last.  The float32 instantiation of each form is pinned to
    the oracle or to a pinned composition elsewhere; this ties the other eighteen to it."""
    ends = _run_form(evg, form, N, cases.SIZES.index(N), 160)
    assert ends >= N


@pytest.mark.parametrize("N", [1, 33])
@pytest.mark.parametrize("form", sorted(f for f in FORMS if not FORMS[f][0]))
def test_one_seat_forms_stay_inside_their_outputs_at_one_env_and_at_a_wave_plus_one(evg, form, N):
    """the one-seat image is [N][105]: at an odd N the last 16-byte vector of every observation type straddles the end of the buffer.  A lone partial wave
    (1 env) and a full wave plus one env (33), three turns, every output guarded"""
    _run_form(evg, form, N, int(N == 33), 3)


# ---------------------------------------------------------------------------------------------- D: replay draws, exactly
@pytest.mark.parametrize("form,H,n", [("step_vs_q", 29, 1), ("step_q", 15, 2), ("step_vs_q", 28, 1), ("step_q", 14, 2)])
def test_sample_draws_the_handles_of_the_host_model(evg, form, H, n):
    """sample(B, seed, return_handles=True) == ReplayModel.draw(seed, call, B) after 40 turns of a wrapped ring at 37 envs.  The memory keeps H + 1
    records per env and seat, R = (H + 1) x 37 x seats records in all: R = 1 110 and 1 184 for the first two shapes, 1 073 and 1 110 for the last two --
    all past one 1 024-record scan block, the last two also no multiple of four twice over (1 073 = 4 x 268 + 1, 1 110 = 4 x 277 + 2)."""
    env, mem, model = run_loop(evg, 37, form, turns=40, H=H, n=n, gather_at=(39,))
    assert mem.slots * 37 * mem.S > 1024 and model.size() > 0
    for B in (1, 257, 4099):
        for k in range(3):
            call = int(mem.sample_calls.item())
            got = _np(mem.sample(B, seed=SEED, return_handles=True)[5])
            assert np.array_equal(got, model.draw(SEED, call, B)), (B, k, call)
    mem.sample_calls.fill_(2 ** 32 + 3)                                     # the counter's high word enters the block
    got = _np(mem.sample(257, seed=SEED, return_handles=True)[5])
    assert np.array_equal(got, model.draw(SEED, 2 ** 32 + 3, 257))
    assert int(mem.sample_calls.item()) == 2 ** 32 + 4
    mem.check()
    env.close()
