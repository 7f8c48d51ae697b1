"""CPU test (no GPU needed) of the Minimized Q network's host model (tests/minimized_model.py: the float32 fmaf chain evg_minimized_qnet promises)
against the reference's own QNetwork(59, 11, 80) forward recorded in tests/golden/minimized_qnet.npz (tools/gen_minimized_golden.py)."""
import numpy as np

from conftest import load_golden
import minimized_model as mm


def test_chain_equals_the_reference_forward_within_four_times_its_own_rounding_error():
    """Yardstick: the float64 evaluation of the same weights and inputs.  Tolerance: 4 x the largest |float32 chain - float64| on the fixture (torch sums
    in another order).  Measured on the fixture (480 rows x 11 outputs, |q| up to 15.7): chain against float64 3.68e-06, hence the bound 1.47e-05; chain
    against the reference's float32 forward 2.86e-06."""
    d = load_golden("minimized_qnet.npz")
    params = (d["w1"], d["b1"], d["w2"], d["b2"])
    assert d["w1"].shape == (80, 59) and d["w2"].shape == (11, 80) and d["x"].shape[0] * 12 <= 512
    x = d["x"].reshape(-1, 59)
    q32 = mm.forward(x, params, True)
    q64 = mm.forward_f64(x, params, True)
    own = np.abs(q32.astype(np.float64) - q64).max()
    got = np.abs(q32.astype(np.float64) - d["q"].reshape(-1, 11).astype(np.float64)).max()
    print("float32 chain against float64: %.3e; against the reference forward: %.3e; bound %.3e" % (own, got, 4 * own))
    assert 0 < own < 1e-4
    assert got <= 4 * own
    assert (d["q"] >= 0).all() and (d["q"] > 0).mean() > 0.3            # the reference applies the final ReLU, and it does not clip everything


def test_compact_and_expanded_forms_agree_bit_for_bit():
    d = load_golden("minimized_qnet.npz")
    params = (d["w1"], d["b1"], d["w2"], d["b2"])
    x = d["x"][:6]
    shared, swarm = x[:, 0, :34], x[:, :, 34:47]
    for fr in (True, False):
        assert np.array_equal(mm.forward_compact(shared, swarm, params, fr), mm.forward(x, params, fr))
