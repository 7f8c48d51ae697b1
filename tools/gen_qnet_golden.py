#!/usr/bin/env python3
"""Writes tests/golden/smart_qnet.npz: the reference's Q network (agents/Smart_State/QNetwork.py, imported from the reference tree, not restated) on
the Smart_State features already in tests/golden/smart_state.npz (`features` [102, 2, 12, 59], create_swarm_obs's values; rounded once to float32 as
the device holds them).  Three networks, each stored as its weights and the reference forward's float32 output on every feature row:

    a   QNetwork(59, 5, 60, 60) with the class's own seeded initialisation (torch.manual_seed(1) in its __init__)
    b   QNetwork(59, 5, 64, 17), weights from load_state_dict of a seeded normal x 0.3 (so that few outputs are clipped by the final ReLU)
    c   QNetwork(59, 5, 1, 64), the same way

Per network <v>: v_w1 [h1, 59], v_b1, v_w2 [h2, h1], v_b2, v_w3 [5, h2], v_b3 (float32), v_q [102, 2, 12, 5] float32 (reference forward, torch CPU).

    python tools/gen_qnet_golden.py        (needs the reference tree: EVG_REFERENCE, default /root/reference)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("EVG_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "smart_qnet.npz")
NETS = [("a", 60, 60, None), ("b", 64, 17, 101), ("c", 1, 64, 102)]      # name, fc1, fc2, seed of the loaded weights (None: the class's own)


def main():
    sys.path.insert(0, REF)
    import torch
    import agents.Smart_State.QNetwork as QN
    x = np.load(os.path.join(ROOT, "tests", "golden", "smart_state.npz"))["features"].astype(np.float32)
    out = {}
    for name, h1, h2, seed in NETS:
        net = QN.QNetwork(59, 5, h1, h2)
        if seed is not None:
            g = torch.Generator().manual_seed(seed)
            sd = {k: torch.randn(v.shape, generator=g) * 0.3 for k, v in net.state_dict().items()}
            net.load_state_dict(sd)
        with torch.no_grad():
            q = net(torch.from_numpy(x)).numpy().astype(np.float32)
        for key, t in (("w1", net.fc1.weight), ("b1", net.fc1.bias), ("w2", net.fc2.weight), ("b2", net.fc2.bias), ("w3", net.fc3.weight),
                       ("b3", net.fc3.bias)):
            out[name + "_" + key] = t.detach().numpy().astype(np.float32)
        out[name + "_q"] = q
        print("%s: QNetwork(59, 5, %d, %d), %.1f %% of the outputs > 0" % (name, h1, h2, 100.0 * (q > 0).mean()))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
