"""Writes tests/golden/g19_se_parent_bits.npz: what FTC_OP_SE computes on the seeded operands of tests/test_gpu_se_bits.py.

Run on an MI355X with this repository's library built from the commit whose bits are to be pinned (the fixture in the tree was recorded
at the commit before the one-round-trip rewrite of the SE kernels):

    python tests/golden/gen_golden_se_bits.py

Per case: the gates [B, C] in full (as uint32 bits), the SHA-256 of the folded weight bytes and of the operands.  Before anything runs
on the GPU the script checks on the CPU that the recorded partial products pin the order of their sum: the kernels' association (four
partial sums over j mod 4, remainder onto the first, (a0 + a1) + (a2 + a3)) must differ in fp32 bits from the sequential, the reversed
and the pairwise sum somewhere in every case with three or more partial products."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_se_bits as T  # noqa: E402


def kernel_order(hp):
    """[B, NS, S] -> [B, S], the association of se_load_hidden, every add rounded to fp32."""
    ns = hp.shape[1]
    a = [np.zeros_like(hp[:, 0]) for _ in range(4)]
    for j in range(ns - ns % 4):
        a[j % 4] = a[j % 4] + hp[:, j]
    for j in range(ns - ns % 4, ns):
        a[0] = a[0] + hp[:, j]
    return (a[0] + a[1]) + (a[2] + a[3])


def sequential(hp):
    s = np.zeros_like(hp[:, 0])
    for j in range(hp.shape[1]):
        s = s + hp[:, j]
    return s


def pairwise(hp):
    v = [hp[:, j] for j in range(hp.shape[1])]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0]


def order_is_pinned(c, hp):
    assert hp.dtype == np.float32
    k = kernel_order(hp).view(np.uint32)
    others = {"sequential": sequential(hp), "reversed": sequential(hp[:, ::-1]), "pairwise": pairwise(hp)}
    differing = [n for n, v in others.items() if np.any(v.view(np.uint32) != k)]
    assert differing, f"{c['id']}: every association of the partial products gives the same bits -- the case pins nothing"
    return differing


def main():
    for c in T.CASES:
        if c["hp"] and c["NS"] >= 3:
            order_is_pinned(c, T.operands(c)["aux"])
    out = {"ids": np.array([c["id"] for c in T.CASES]), "wb_sha": [], "in_sha": []}
    for c in T.CASES:
        ln = T.Launch(c)
        try:
            ln.run()
            scale, sha = ln.outputs()
        finally:
            ln.close()
        assert np.all(np.isfinite(scale.view(np.float32))) and scale.view(np.float32).std() > 0.01, f"{c['id']}: degenerate gates"
        out["scale_%03d" % c["idx"]] = scale
        out["wb_sha"].append(sha)
        out["in_sha"].append(T.operands_sha(T.operands(c)))
    out["wb_sha"], out["in_sha"] = np.array(out["wb_sha"]), np.array(out["in_sha"])
    dst = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(T.CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
