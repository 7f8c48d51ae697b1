#!/usr/bin/env python3
"""What the MI355X does with bf16 subnormals in the Q networks' bf16 forward (outside the pinned domain of include/evg_qnet_bf16.h; DESIGN.md records
the answer): a 59-1-11 Minimized network in both precisions with a subnormal input, weight, hidden activation and accumulator.

    python tools/qnet_bf16_subnormals.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import everglades_amd as evg
env = evg.EvergladesVecEnv(64, seed=1)
dev = env.device
def run(x0, w1v, b1v, w2v):
    w1 = torch.zeros((1, 59), device=dev); w1[0, 0] = w1v
    b1 = torch.full((1,), b1v, device=dev)
    w2 = torch.zeros((11, 1), device=dev); w2[:, 0] = w2v
    b2 = torch.zeros((11,), device=dev)
    x = torch.zeros((16, 59), device=dev); x[:, 0] = x0
    out = {}
    for prec in ("fp32", "bf16"):
        out[prec] = env.minimized_qnet((w1, b1, w2, b2), final_relu=False, precision=prec).expanded(x)[0, 0].item()
    return out
for name, args in [("A subnormal bf16 input 2^-130 x weight 2^100 (x w2 1)", (2.0 ** -130, 2.0 ** 100, 0.0, 1.0)),
                   ("B input 2^100 x subnormal bf16 weight 2^-130 (x w2 1)", (2.0 ** 100, 2.0 ** -130, 0.0, 1.0)),
                   ("C hidden activation = subnormal bias 2^-130, x w2 2^100", (0.0, 0.0, 2.0 ** -130, 2.0 ** 100)),
                   ("D product 2^-70 x 2^-70 = 2^-140 (fp32 subnormal accumulator), x w2 2^100", (2.0 ** -70, 2.0 ** -70, 0.0, 2.0 ** 100)),
                   ("E normal 2^-20 x 2^-10 (control; expect 2^-30)", (2.0 ** -20, 2.0 ** -10, 0.0, 1.0))]:
    r = run(*args)
    print("%s: fp32 %r, bf16 %r (2^-30 = %r)" % (name, r["fp32"], r["bf16"], 2.0 ** -30))
env.close()
