"""include/ftc_text_compact.h on the MI355X: the attention kernel with a key / value row map against the plain kernel on gathered inputs
and against float64, and the compact mask-predict loop against ftc_text_predict.  Everything the two loops return is compared BIT FOR
BIT: a row of a batch is the row decoded alone whatever the batch is, so taking stopped rows out of later passes may not change a bit.

The loop tests assert a condition on their own inputs before anything else: the old loop's traces must show at least three distinct
per-row pass counts, among them 8 and a value <= 3 -- with rows that all stop together the comparison would pass with nothing compacted."""
import ctypes as C

import numpy as np
import pytest
import torch

from compact_harness import DEFAULT, DEV, SMALL, bench_rows, passes_per_row, recognizer
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.transformer import predict_device

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
GAIN = {128: 100.0, DEFAULT.embed_dim: 32.0}          # per size: the gain at which the eight rows stop after different numbers of passes


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def bits(t: torch.Tensor) -> bytes:
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- the attention kernel with a row map ------------------------------------------------------------------------------------------------
def _attention(q, kv, pad, heads, Sq, Sk, B, kv_row=None, Bkv=None, rows=False):
    E = 64 * heads
    ld = 3 * E
    out = torch.full((B * Sq, E + 4), 7.0, device=DEV)
    lib = L.load()
    if rows:
        rc = lib.ftc_text_attention_rows(q.data_ptr(), ld, kv.data_ptr() + 4 * E, ld, kv.data_ptr() + 8 * E, ld, pad.data_ptr() if pad is not None else None,
                                         kv_row.data_ptr() if kv_row is not None else None, Bkv, out.data_ptr(), E + 4, B, heads, Sq, Sk, stream())
    else:
        rc = lib.ftc_text_attention(q.data_ptr(), ld, kv.data_ptr() + 4 * E, ld, kv.data_ptr() + 8 * E, ld, pad.data_ptr() if pad is not None else None,
                                    out.data_ptr(), E + 4, B, heads, Sq, Sk, stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("heads,Sq,Sk", [(2, 400, 400), (3, 77, 211)])
def test_attention_rows_equals_the_plain_kernel_on_gathered_inputs(heads, Sq, Sk):
    gen = torch.Generator().manual_seed(31 * heads + Sq)
    E, Bkv = 64 * heads, 5
    q_all = torch.randn(6 * Sq, 3 * E, generator=gen).to(DEV)
    kv = torch.randn(Bkv * Sk, 3 * E, generator=gen).to(DEV)
    pad_b = torch.rand(Bkv, Sk, generator=gen) < 0.3
    pad_b[0] = False
    pad_b[4] = True
    pad_b[4, Sk // 2] = False                                            # a row with ONE valid key
    pad = pad_b.to(torch.uint8).to(DEV)
    m = [3, 0, 3, 4, 1, 0]                                               # repeats 3 and 0, reorders, omits 2
    kv_row = torch.tensor(m, dtype=torch.int32, device=DEV)
    got = _attention(q_all, kv, pad, heads, Sq, Sk, len(m), kv_row, Bkv, rows=True)
    idx = torch.tensor(m, device=DEV)
    kv_g = kv.view(Bkv, Sk, 3 * E)[idx].reshape(len(m) * Sk, 3 * E).contiguous()
    want = _attention(q_all, kv_g, pad[idx].contiguous(), heads, Sq, Sk, len(m))
    assert bits(got) == bits(want)
    assert bool((got[:, E:] == 7.0).all()) and not bool(torch.isnan(got).any())
    # NULL map: the plain kernel
    q5 = q_all[:Bkv * Sq].contiguous()
    assert bits(_attention(q5, kv, pad, heads, Sq, Sk, Bkv, None, Bkv, rows=True)) == bits(_attention(q5, kv, pad, heads, Sq, Sk, Bkv))
    assert bits(_attention(q5, kv, None, heads, Sq, Sk, Bkv, None, Bkv, rows=True)) == bits(_attention(q5, kv, None, heads, Sq, Sk, Bkv))
    # float64, with the bound tests/test_gpu_text.py uses for this kernel: 8 x sqrt(64 + Sk) x 2^-24 x max|v|
    q = q_all[:, :E].cpu().double().view(len(m), Sq, heads, 64).transpose(1, 2)
    k = kv_g[:, E:2 * E].cpu().double().view(len(m), Sk, heads, 64).transpose(1, 2)
    v = kv_g[:, 2 * E:].cpu().double().view(len(m), Sk, heads, 64).transpose(1, 2)
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(pad_b[m][:, None, None, :], float("-inf"))
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(len(m) * Sq, E)
    err = float((got[:, :E].cpu().double() - ref).abs().max())
    bound = 8 * (64 + Sk) ** 0.5 * EPS * float(v.abs().max())
    print(f"[compact] attention_rows h{heads} Sq{Sq} Sk{Sk}: max error {err:.2e} (bound {bound:.2e})")
    assert err <= bound


def test_attention_rows_entry_out_of_range_gives_nans_in_its_slot_only():
    """The guard is a comparison before the address is formed: the entries 5, -1 and 2^30 are never used as an index."""
    heads, Sq, Sk, Bkv = 2, 100, 90, 5
    gen = torch.Generator().manual_seed(9)
    E = 64 * heads
    q = torch.randn(5 * Sq, 3 * E, generator=gen).to(DEV)
    kv = torch.randn(Bkv * Sk, 3 * E, generator=gen).to(DEV)
    good = torch.tensor([1, 2, 0, 4, 3], dtype=torch.int32, device=DEV)
    bad = torch.tensor([1, Bkv, 0, -1, 1 << 30], dtype=torch.int32, device=DEV)
    want = _attention(q, kv, None, heads, Sq, Sk, 5, good, Bkv, rows=True).view(5, Sq, E + 4)
    got = _attention(q, kv, None, heads, Sq, Sk, 5, bad, Bkv, rows=True).view(5, Sq, E + 4)
    for slot in (1, 3, 4):
        assert bool(torch.isnan(got[slot, :, :E]).all()) and bool((got[slot, :, E:] == 7.0).all())
    for slot in (0, 2):
        assert bits(got[slot]) == bits(want[slot])


# ---- the compact loop against ftc_text_predict ------------------------------------------------------------------------------------------
def _both(model2, x):
    eng = model2._engine
    old = predict_device(eng, x, trace=True)
    ids, probs, tr = old[0].clone(), old[1].clone(), [t.clone() for t in old[2]]
    new = predict_device(eng, x, trace=True, compact=True)
    torch.cuda.synchronize()
    return (ids, probs, tr, old[3]), new


def _check(model2, x, what, need_spread=True):
    (ids, probs, tr, passes), (ids2, probs2, tr2, passes2, rows_run) = _both(model2, x)
    B = x.shape[0]
    ran = passes_per_row(tr[0])                                          # [8, B]
    counts = ran.sum(0)
    print(f"[compact] {what}: B {B}, passes per row {counts.tolist()[:16]}{' ...' if B > 16 else ''}, passes_run {passes}, rows_run {rows_run} "
          f"({sum(rows_run)} of {B * passes} row-passes)")
    if need_spread:
        # the condition on the inputs: without it the comparison below would pass with nothing compacted
        assert len(set(counts.tolist())) >= 3 and 8 in counts and counts.min() <= 3, f"{what}: the rows do not stop at different passes: {counts.tolist()}"
    assert passes2 == passes == int(counts.max())
    assert bits(ids2) == bits(ids) and bits(probs2) == bits(probs)
    for a, b, name in zip(tr, tr2, ("tokens", "codes", "probs")):
        assert bits(a) == bits(b), f"{what}: trace_{name} differs"
    assert len(rows_run) == 8 and rows_run == ran.sum(1).tolist()
    if need_spread:
        assert sum(rows_run) < B * passes
    else:
        assert sum(rows_run) <= B * passes
    return counts


CASES = [("fp32", SMALL), ("fp16x3", SMALL), ("bf16", SMALL), ("fp16", SMALL), ("fp32", DEFAULT), ("bf16", DEFAULT)]


@pytest.mark.parametrize("precision,dims", CASES, ids=[f"{p}-{d.embed_dim}" for p, d in CASES])
def test_compact_loop_is_bitwise_the_old_loop(precision, dims):
    model2 = recognizer(precision, dims, GAIN[dims.embed_dim])
    X = bench_rows(7)
    x8 = torch.from_numpy(X).to(DEV)
    what = f"{precision} E{dims.embed_dim}"
    counts = _check(model2, x8, what)
    rev = _check(model2, x8.flip(0).contiguous(), what + " reversed")
    assert rev.tolist() == counts.tolist()[::-1]                         # a row's pass count is its own, wherever it sits
    # B = 1: nothing can be dropped, so rows_run is 1 for every pass run (the strict inequality is a statement about batches)
    for r in (int(np.argmin(counts)), int(np.argmax(counts))):
        one = _check(model2, x8[r:r + 1].contiguous(), what + f" row {r} alone", need_spread=False)
        assert one.tolist() == [counts[r]]
    # B = 64: the eight rows eight times
    big = _check(model2, x8.repeat(8, 1, 1).contiguous(), what + " x8")
    assert big.tolist() == counts.tolist() * 8


def test_compact_loop_refuses_no_readback_and_reports_rows_of_unrun_passes_as_zero():
    model2 = recognizer("fp32", SMALL, GAIN[128])
    x = torch.from_numpy(bench_rows(7)[1:3].copy()).to(DEV)              # two rows that stop early
    with pytest.raises(L.FtcError, match="FTC_TEXT_NO_READBACK is refused"):
        predict_device(model2._engine, x, readback=False, compact=True)
    out = predict_device(model2._engine, x, compact=True)
    assert out[3] < 8 and out[4][out[3]:] == [0] * (8 - out[3]) and all(n > 0 for n in out[4][:out[3]])
