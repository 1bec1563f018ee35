#!/usr/bin/env python3
"""Golden-vector generator of g22_radam_schedulefree.npz.  Runs ONLY in the build container (needs /root/reference).

Imports the reference's own ``models/radam_schedulefree.py`` and runs its ``RAdamScheduleFree`` on the CPU, ``foreach`` branch, through the six
cases of tests/radam_operands.py (RADAM_CASES; parameters and gradients regenerated from the seed there, nothing of them is stored): train(), nine
steps, eval(), train() again.  Per case it writes

    c{i}_steps  float32 [9, n]   the parameters after every step          c{i}_sched  float64 [9, 3]   (scheduled_lr, lr_max, weight_sum) per step
    c{i}_z, c{i}_v  float32 [n]  the final z and exp_avg_sq               c{i}_eval, c{i}_train  float32 [n]   after eval(), after train() again

where n runs over radam_operands.PICK: every element of the three small tensors and 256 seeded elements of the (4097,) one.  Nothing of the
reference's source travels: the fixture is data only.

    python tests/golden/gen_golden_radam.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import radam_operands as R  # noqa: E402


def reference_class():
    spec = importlib.util.spec_from_file_location("ref_radam_schedulefree", os.path.join(REF, "models", "radam_schedulefree.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # (reference code)
    return mod.RAdamScheduleFree


def main():
    RefOpt = reference_class()
    torch.set_num_threads(1)

    def make(params0, kwargs):
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in params0]
        opt = RefOpt(ps, foreach=True, **kwargs)

        def set_grads(gs):
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(g.copy())
        return opt, ps, set_grads, lambda p: opt.state[p]

    out = {}
    for ci in range(len(R.RADAM_CASES)):
        res = R.run_case(ci, make, lambda t: t.detach().numpy().copy())
        for k, v in res.items():
            out[f"c{ci}_{k}"] = v
    np.savez_compressed(R.GOLD, **out)
    print("wrote", os.path.basename(R.GOLD), os.path.getsize(R.GOLD) // 1024, "KiB")


if __name__ == "__main__":
    main()
