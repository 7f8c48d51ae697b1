"""The Philox rounds built from one three-input xor (csrc/evg_rng.h) and the observation write-out addressed by constant offsets from one per-lane base
(csrc/step_outputs.inc), at the smallest shapes where either can go wrong: every comparison is exact equality with the CPU oracle.

Which kernel a case runs: the product library plays a persistent rollout of so few envs with the four-lanes-per-env kernel (16 envs per wavefront), which
shares the Philox function but has a write-out of its own; the diagnostic library (libevg_diag.so) is asked for the two-lanes-per-env kernel -- the
flagship's kernel, whose write-out template changed: 64 envs = two full wavefronts (the straight-line path), 77 = those plus a 13-env wavefront (the
bounds-checked path) -- and for its 16-envs-per-wavefront instantiation (lanes = 32), the same template with other constants."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OBS_ROW = 2 * 105            # values per env
SENTINEL, GUARD = -7, 64


@pytest.fixture(scope="module")
def evg():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import everglades_amd
    return everglades_amd


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("seed", [2026, 0x9E3779B97F4A7C15 & 0xFFFFFFFF])
@pytest.mark.parametrize("N", [1, 33, 77])
def test_random_actions_rows_equal_the_oracles(evg, oracle_mod, N, seed):
    """evg_random_actions against the oracle's random_actions(): all [N, 2, 7, 2] rows of three consecutive turns.  Every row is drawn from both halves
    of the words of two Philox blocks, so one wrong round shows."""
    env = evg.EvergladesVecEnv(N, seed=seed, auto_reset=False)
    ora = oracle_mod.Oracle(N, seed=seed)
    env.reset(); ora.reset()
    for t in range(3):
        a = env.random_actions()
        want = ora.random_actions()
        assert a.shape == (N, 2, 7, 2) and np.array_equal(_np(a), want), ("turn", t)
        env.step(a); ora.step(want)
    env.close()


def _persistent_rollout_vs_oracle(evg, oracle_mod, N, dtype, **env_kw):
    """8 launches of 5 turns.  Outputs are overwritten every turn, so what is compared after a launch is its LAST turn (observations, reward, done, scores,
    recorded orders); the final state covers the rest.  The guarded observation buffer goes in through the env's buffer-adoption hook (what PipelinedVecEnv
    uses), the recorded orders are read from the env's own order buffer: there is no public way to hand a rollout a caller's tensors."""
    import torch
    seed, tpl, launches = 77, 5, 8
    env = evg.EvergladesVecEnv(N, seed=seed, obs_dtype=dtype, auto_reset=True, **env_kw)
    ora = oracle_mod.Oracle(N, seed=seed, auto_reset=True)
    # the observation buffer with 64 guard elements behind it
    big = torch.full((N * OBS_ROW + GUARD,), SENTINEL, dtype=env.obs_dtype, device=env.device)
    obs = big[:N * OBS_ROW].view(N, 2, 105)
    env._adopt_buffers(obs, env.reward, env.done, env.winner, env.scores, env.status, env._actions)
    assert np.array_equal(_np(env.reset()).astype(np.float64), ora.reset())
    for k in range(launches):
        big.fill_(SENTINEL)
        out = env.rollout_random(tpl, turns_per_launch=tpl)
        for t in range(tpl):
            acts = ora.random_actions()
            o_obs, o_rew, o_done, o_info = ora.step(acts)
        assert not (o_obs == SENTINEL).any()                                   # (the sentinel is no value of an observation)
        got = _np(big)
        assert not (got[:N * OBS_ROW] == SENTINEL).any(), ("sentinel left inside", k)
        assert (got[N * OBS_ROW:] == SENTINEL).all(), ("guard elements changed", k)
        assert out[0].data_ptr() == big.data_ptr()
        assert np.array_equal(_np(out[0]).astype(np.float64), o_obs), ("obs", k)
        assert np.array_equal(_np(out[1]), o_rew.astype(np.float32)), ("reward", k)
        assert np.array_equal(_np(out[2]), o_done), ("done", k)
        assert np.array_equal(_np(out[3]["scores"]), o_info["scores"]), ("scores", k)
        assert np.array_equal(_np(env._actions), acts), ("recorded orders", k)
    s, want = env.get_state(), ora.get_state()
    for key in ("groups", "nodes", "health", "env"):
        assert np.array_equal(s[key], want[key]), key                        # health: float64, bit for bit
    env.close()


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
@pytest.mark.parametrize("N", [64, 77])
def test_persistent_rollout_equals_the_oracle_launch_by_launch(evg, oracle_mod, N, dtype):
    """rollout_random, 5 turns per launch, 8 launches, product library: observations (in a buffer pre-filled with a sentinel, 64 guard elements behind it),
    reward, done, scores and recorded orders after every launch, the state incl. float64 health at the end."""
    _persistent_rollout_vs_oracle(evg, oracle_mod, N, dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
@pytest.mark.parametrize("N", [64, 77])
def test_two_lane_persistent_write_out_equals_the_oracle(evg, oracle_mod, N, dtype):
    """The same through the diagnostic library's forced two-lanes-per-env kernel: the flagship's persistent kernel at two full wavefronts (every store of
    the straight-line write-out at its constant offset) and at two full wavefronts plus a partial one (the bounds-checked loop).  The only cases of this
    file that reach the changed template's straight-line path: a missing diagnostic library fails them."""
    _persistent_rollout_vs_oracle(evg, oracle_mod, N, dtype, library=evg._lib.DIAG_LIB_PATH, diag=dict(lanes=64))


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
def test_16_envs_per_wave_write_out_equals_the_oracle(evg, oracle_mod, dtype):
    """The same at 64 envs through the diagnostic library's 16-envs-per-wavefront variant: the write-out template with LPW = 32 (half the image, other
    store counts and another tail)."""
    if not os.path.exists(evg._lib.DIAG_LIB_PATH):
        pytest.skip("libevg_diag.so is not built (make -C csrc diag)")
    _persistent_rollout_vs_oracle(evg, oracle_mod, 64, dtype, library=evg._lib.DIAG_LIB_PATH, diag=dict(lanes=32))
