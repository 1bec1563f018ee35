"""Writes tests/golden/g20_mbhead_parent_bits.npz: what FTC_OP_MBHEAD computes on the seeded operands of tests/test_gpu_mbhead_bits.py.

Run on an MI355X with this repository's library built from the commit whose bits are to be pinned (the fixture in the tree was recorded
at the commit before the depthwise phase of csrc/mbconv_slice.hip was rewritten):

    python tests/golden/gen_golden_mbhead_bits.py

Per case: the SHA-256 of the `out` bytes, `sums` [B, bands, C] and `hpart` [B, bands, C / slice, S] in full (as uint32 bits) and the
SHA-256 of the operands.  Per case the script also evaluates the op in float64 on the CPU (16-bit operands, the expanded image narrowed
to the 16-bit type after its SiLU, as the kernel does) and asserts that
  - the recorded sums are that computation to within 1e-2 of the sum of magnitudes (a wiring check only: a transposed tap or a wrong
    layout is an error of order one; fp32 sums, the fast SiLU and a 16-bit value rounded the other way are orders below), and
  - the recorded sums differ in bits from the float64 channel sums rounded to fp32 in at least one channel, i.e. the data make the order
    of the sum visible: a kernel that added the same values in another order would not reproduce the fixture."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_mbhead_bits as T  # noqa: E402
from findtextcenternet_amd import _lib as L  # noqa: E402
from gpu_harness import round16  # noqa: E402


def float64_sums(c, o):
    """[B, bands, C] channel sums of the op's output before it is narrowed, and the sums of magnitudes, in float64."""
    B, H, W, Cc, R, nb = c["B"], c["H"], c["W"], c["C"], c["R"], c["nb"]
    t = torch.from_numpy
    x, we = round16(t(o["x"]), c["dt"]).double(), round16(t(o["we"]), c["dt"]).double()
    e = torch.nn.functional.silu(x @ we.t() + t(o["be"]).double())
    e = round16(e.float(), c["dt"]).double().reshape(B, H, W, Cc).permute(0, 3, 1, 2)
    wd = t(o["wd"]).double().t().reshape(Cc, 1, 3, 3)
    d = torch.nn.functional.silu(torch.nn.functional.conv2d(e, wd, t(o["bd"]).double(), padding=1, groups=Cc))       # [B, C, H, W]
    bands = [d[:, :, j * R:(j + 1) * R] if R else d for j in range(nb)]
    s = torch.stack([v.sum(dim=(2, 3)) for v in bands], dim=1)
    mag = torch.stack([v.abs().sum(dim=(2, 3)) for v in bands], dim=1)
    return s.numpy(), mag.numpy()


def main():
    out = {"ids": np.array([c["id"] for c in T.CASES]), "out_sha": [], "in_sha": []}
    for c in T.CASES:
        o = T.operands(c)
        sha, sums, hp = T.run_case(c, o)
        got = sums.view(np.float32)
        assert np.all(np.isfinite(got)) and got.std() > 0.01, f"{c['id']}: degenerate sums"
        want, mag = float64_sums(c, o)
        err = float((np.abs(got.astype(np.float64) - want) / mag).max())
        assert err < 1e-2, f"{c['id']}: the recorded sums are not the float64 evaluation of the op: {err:.2e} of the sum of magnitudes"
        differ = int((want.astype(np.float32).view(np.uint32) != sums).sum())
        assert differ > 0, f"{c['id']}: the sums equal the correctly rounded float64 sums in every channel -- the case does not pin the order"
        print(f"{c['id']}: sums within {err:.1e} of float64, {differ} of {sums.size} differ in bits from its rounding", flush=True)
        out["sums_%02d" % c["idx"]] = sums
        if c["hp"]:
            assert np.all(np.isfinite(hp.view(np.float32))) and hp.view(np.float32).std() > 1e-4, f"{c['id']}: degenerate hpart"
            out["hpart_%02d" % c["idx"]] = hp
        out["out_sha"].append(sha)
        out["in_sha"].append(T.operands_sha(o))
    out["out_sha"], out["in_sha"] = np.array(out["out_sha"]), np.array(out["in_sha"])
    dst = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(T.CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
