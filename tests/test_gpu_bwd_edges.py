"""-m gpu: FTC_OP_DILATE, FTC_OP_UPCATBWD (csrc/bwd_ops.hip) per element, and FTC_OP_LOSSES / FTC_OP_LOSS_BWD (csrc/train_ops.hip, csrc/bwd_ops.hip) at
their branch edges, as single-op plans.  Cases, references and bounds: tests/bwd_edge_cases.py; tests/test_bwd_edges_host.py proves on the CPU that an
fp32 evaluation of the same forms stays inside each bound and that the mutants it names fall outside or flip an exact output.

    DILATE      torch.equal with the scattered input (the zeros are written: the arena is filled with 0xCD)
    UPCATBWD    |out - out64| <= the per-element bound of bwd_edge_cases (weight errors 3 u Hi / 3 u Wi on the weighted |g| of the element's own taps + 18 u sum |w g|), out64 the
                float64 transpose of the upsample with exact rational weights
    LOSSES      each of the nine losses and their total within 2 e u + 2^-100, e from the running error analysis of the kernel's own expression;
                correct, total exact; the two normalisers within one fp32 rounding of the float64 sum of the reference's weights
    LOSS_BWD    every element of d maps and d decoder logits within its own such bound; pad columns, rows outside mask3 and the size gradient outside
                key > 0.85 exactly 0; no NaN anywhere; no element excluded
The reference of the loss ops is float64 autograd through oracle/loss_oracle.py with the reference's float32 divisors.  The last DILATE / UPCATBWD case has
just over 16384 x 256 channel quads: the grid-stride loop takes a second trip.  Real-valued data stay with test_gpu_bwd_ops / test_gpu_train_ops."""
import functools

import pytest
import torch

import bn_operands as N
import bwd_edge_cases as K
from findtextcenternet_amd import _lib as L
from gpu_harness import Arena, run_op

pytestmark = pytest.mark.gpu


def _guard_intact(ar):
    assert bool((ar.buf[ar.size:ar.size + 256] == 0xCD).all()), "bytes past the last operand were written"


@pytest.mark.parametrize("cid", [i for i, _ in K.DILATE_CASES])
def test_dilate_is_a_copy(cid):
    c = K.dilate_case(dict(K.DILATE_CASES)[cid])
    B, H, W, C = c.shape
    ar = Arena()
    o_in, o_out = ar.put(c.x), ar.reserve(B * 4 * H * W * C * 4)
    ar.materialize()
    run_op(dict(kind=L.OP_DILATE, B=B, H=H, W=W, Ho=2 * H, Wo=2 * W, Cin=C, in_=o_in, out=o_out), ar)
    assert torch.equal(ar.read(o_out, (B, 2 * H, 2 * W, C), torch.float32), c.want), cid
    _guard_intact(ar)


@pytest.mark.parametrize("cid", [i for i, _ in K.UPCAT_CASES])
def test_upcatbwd_per_element(cid):
    c = K.upcat_case(dict(K.UPCAT_CASES)[cid])
    B, Hi, Wi, Cy, Ct = c.shape
    ar = Arena()
    o_g, o_out = ar.put(c.g), ar.reserve(B * Hi * Wi * Cy * 4)
    ar.materialize()
    run_op(dict(kind=L.OP_UPCATBWD, B=B, H=Hi, W=Wi, Ho=2 * Hi, Wo=2 * Wi, Cin_total=Ct, aux0=Cy, in_=o_g, out=o_out), ar)
    N.assert_within(ar.read(o_out, (B, Hi, Wi, Cy), torch.float32), c.want, c.bound, f"upcatbwd {cid}")
    _guard_intact(ar)


@functools.lru_cache(maxsize=None)
def _loss_case(kind, rows):
    c = K.loss_grid(kind, rows)
    return c, K.oracle64(c), K.loss_bounds(c)


def _run_losses(c):
    lib = L.load()
    ar = Arena()
    o_maps, o_lab, o_id = ar.put(c.maps), ar.put(c.label), ar.put(c.idmap)
    o_sel = ar.put(c.sel) if c.R else None
    o_d = [ar.put(d) if c.R else None for d in c.dec]
    o_lossv, o_scr = ar.reserve(64), ar.reserve(int(lib.ftc_losses_scratch_bytes()))
    o_al, o_gm = ar.put(K.ALPHAS), ar.reserve(c.n * 9 * 4)
    o_gd = ar.reserve(3 * c.R * K.PAD * 4) if c.R else None
    ar.materialize()
    common = dict(B=c.B, H=c.h, W=c.w, aux0=c.R, in_=o_maps, in2=o_lab, w=o_id, w2=o_d[0], bias=o_d[1], bias2=o_d[2], scale=o_sel)
    run_op(dict(kind=L.OP_LOSSES, out=o_lossv, aux=o_scr, **common), ar)
    lossv = ar.read(o_lossv, (16,), torch.float32)
    run_op(dict(kind=L.OP_LOSS_BWD, aux1=K.PAD, Cout=N.fbits(K.LSCALE), shift=o_al, aux=o_lossv, out=o_gm, out2=o_gd, **common), ar)
    gm = ar.read(o_gm, (c.B, c.h, c.w, 9), torch.float32)
    gd = ar.read(o_gd, (3, c.R, K.PAD), torch.float32) if c.R else None
    _guard_intact(ar)
    return lossv, gm, gd


@pytest.mark.parametrize("kind,rows", K.LOSS_CASES, ids=[f"{k}{'' if r else '_no_rows_selected'}" for k, r in K.LOSS_CASES])
def test_losses_and_loss_bwd_at_the_branch_edges(kind, rows):
    """Five grids: both normalisers large; no pixel above 0.85; both sums strictly between 0 and 1; selected rows but none in mask3; aux0 = 0.  Keys on
    0, 0.5, 0.85, 0.99, 1 and their fp32 neighbours, ids 0 and above every modulus, logits 0, +-1, +-20, +-40, +-120, size targets inside, on and
    outside the Huber clip, a decoder row with two equal maxima and one with +-60 around the maximum."""
    c, ref, bnd = _loss_case(kind, rows)
    lossv, gm, gd = _run_losses(c)
    meta = f"{kind}, {c.R} rows"
    assert not bool(torch.isnan(gm).any()) and (gd is None or not bool(torch.isnan(gd).any())), meta
    K.check_losses(c, ref, bnd, lossv, meta)
    K.check_loss_bwd(c, ref, bnd, gm, gd, meta)
