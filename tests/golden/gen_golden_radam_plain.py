#!/usr/bin/env python3
"""Golden-vector generator of g27_radam_plain.npz.

Runs ``torch.optim.RAdam`` itself on the CPU with ``foreach=False`` (the single-tensor path, ``_single_tensor_radam``) through the cases of
tests/radam_plain_operands.py (PLAIN_CASES; parameters and gradients regenerated from the seed there, nothing of them is stored): eight steps, one
parameter without a gradient on steps 3 and 4.  Per case it writes

    c{i}_steps  float32 [8, n]   the parameters after every step          c{i}_step  float64 [4]   the final step value of every parameter
    c{i}_m, c{i}_v  float32 [n]  the final exp_avg and exp_avg_sq

where n runs over radam_plain_operands.PICK: every element of the two small tensors and 256 seeded elements each of the (4096,) and (4097,) ones.

    python tests/golden/gen_golden_radam_plain.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import radam_plain_operands as P  # noqa: E402


def main():
    torch.set_num_threads(1)

    def make(params0, kwargs):
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in params0]
        opt = torch.optim.RAdam(ps, foreach=False, **kwargs)

        def set_grads(gs):
            for p, g in zip(ps, gs):
                p.grad = None if g is None else torch.from_numpy(g.copy())
        return opt, ps, set_grads, lambda p: opt.state[p]

    out = {}
    for ci in range(len(P.PLAIN_CASES)):
        res = P.run_case(ci, make, lambda t: t.detach().numpy().copy())
        for k, v in res.items():
            out[f"c{ci}_{k}"] = v
    np.savez_compressed(P.GOLD, **out)
    print("wrote", os.path.basename(P.GOLD), os.path.getsize(P.GOLD) // 1024, "KiB")


if __name__ == "__main__":
    main()
