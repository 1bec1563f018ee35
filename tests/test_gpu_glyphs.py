"""Glyph code-point decode on the MI355X: the select kernel (ftc_glyph_select) against the reference's recorded decode (g14 case A),
the batched decoder + select (ftc_glyph_decode / decode_glyphs / CodeDecoder) against the reference (case B) and against the CPU
restatement on the GPU's own softmax, and batch independence."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import glyph_oracle
from findtextcenternet_amd import CenterNetDetector, CodeDecoder, TextDetectorModel, decode_glyphs, deterministic_state_dict
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.glyphs import glyph_decode_device

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MOD = (1091, 1093, 1097)
DEV = "cuda:0"


def log(msg):
    print("[glyphs] " + msg)          # measured agreement; shown by pytest -rP (or -s)


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(HERE, "golden", "g14_glyph_decode.npz"))


_MODELS = {}


def model_for(precision):
    if precision not in _MODELS:
        g = np.load(os.path.join(HERE, "golden", "g14_glyph_decode.npz"))
        size = str(g["model_size"])
        m = TextDetectorModel(pre_weights=False, model_size=size, precision=precision)
        m.load_state_dict(deterministic_state_dict(int(g["seed_w"]), size))
        m.eval()
        _MODELS[precision] = m
    return _MODELS[precision]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def select(logits, soft=True, lds=None):
    """ftc_glyph_select on three [n, ld_k] fp32 CUDA tensors (the first m_k columns are the logits)."""
    n = logits[0].shape[0]
    ids = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    probs = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    softs = [torch.full((n, m), -7.0, dtype=torch.float32, device=DEV) for m in MOD] if soft else None
    lds = lds or [t.stride(0) if n else MOD[k] for k, t in enumerate(logits)]
    sp = [s.data_ptr() for s in softs] if soft else [None] * 3
    L.check(L.load().ftc_glyph_select(logits[0].data_ptr(), logits[1].data_ptr(), logits[2].data_ptr(), lds[0], lds[1], lds[2], n,
                                      sp[0], sp[1], sp[2], ids.data_ptr(), probs.data_ptr(), stream()), "ftc_glyph_select")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), probs.cpu().numpy(), [s.cpu().numpy() for s in softs] if soft else None


def a_logits(g):
    return [torch.from_numpy(g[f"a_logits{k}"].astype(np.float32)).to(DEV) for k in range(3)]


def test_select_kernel_case_a_vs_reference(g14):
    lg = a_logits(g14)
    ids, probs, soft = select(lg)
    ok = ~g14["a_flag"]
    np.testing.assert_array_equal(ids[ok], g14["a_ids"][ok])
    rel = np.abs(probs - g14["a_probs"]) / g14["a_probs"]
    assert rel[ok].max() <= 2e-6, rel.max()
    for k in range(3):
        ref = torch.softmax(lg[k], dim=-1).cpu().numpy()
        assert np.abs(soft[k] - ref).max() <= 1e-6
        assert np.abs(soft[k].astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
    log(f"select kernel, case A: {int(ok.sum())}/{len(ok)} unflagged glyphs, ids equal; probs rel max {rel.max():.2e}")


def test_select_kernel_pitch_and_null_softmax(g14):
    lg = a_logits(g14)
    ids, probs, soft = select(lg)
    padded = []
    for k, t in enumerate(lg):
        p = torch.full((t.shape[0], MOD[k] + 37), 1e4, dtype=torch.float32, device=DEV)      # junk in the pad must never be read
        p[:, :MOD[k]] = t
        padded.append(p)
    ids2, probs2, soft2 = select(padded, lds=[MOD[k] + 37 for k in range(3)])
    ids3, probs3, _ = select(lg, soft=False)
    for i2, p2 in ((ids2, probs2), (ids3, probs3)):
        np.testing.assert_array_equal(i2, ids)
        np.testing.assert_array_equal(p2.view(np.int32), probs.view(np.int32))
    for k in range(3):
        np.testing.assert_array_equal(soft2[k].view(np.int32), soft[k].view(np.int32))


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257, 4097])
def test_select_kernel_rows_across_wave_and_workgroup_edges(g14, n):
    lg = a_logits(g14)
    base_ids, base_probs, base_soft = select(lg)
    na = lg[0].shape[0]
    pick = np.arange(n) % na
    ids, probs, soft = select([t[torch.from_numpy(pick).to(DEV)].contiguous() for t in lg])
    assert ids.shape == (n,)
    np.testing.assert_array_equal(ids, base_ids[pick])
    np.testing.assert_array_equal(probs.view(np.int32), base_probs[pick].view(np.int32))
    for k in range(3):
        np.testing.assert_array_equal(soft[k].view(np.int32), base_soft[k][pick].view(np.int32))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_select_kernel_vs_oracle_on_gpu_decoder_logits(g14, precision):
    model = model_for(precision)
    feats = torch.from_numpy(g14["b_features"]).to(DEV)
    with torch.no_grad():
        logits = model.decoder(feats)
    ids, probs, soft = select([t.contiguous() for t in logits])
    o_ids, o_probs = glyph_oracle.decode_rows(*soft)
    np.testing.assert_array_equal(ids, o_ids)
    assert (np.abs(probs - o_probs) / o_probs).max() <= 4e-6          # device logf / expf against NumPy's: measured 2.0e-6


def _clear(g, tol=2e-3):
    return (g["b_thr_dist"].min(axis=1) > tol) & (g["b_key_gap"] > tol)


@pytest.mark.parametrize("precision,gate", [("fp32", None), ("fp16x3", None), ("bf16", 0.98), ("fp16", 0.99)])
def test_decode_glyphs_vs_reference_case_b(g14, precision, gate):
    model = model_for(precision)
    ids, probs = decode_glyphs(model, g14["b_features"])
    assert ids.dtype == np.int64 and probs.dtype == np.float32 and ids.shape == (256,)
    clear = _clear(g14)
    agree = float((ids == g14["b_ids"]).mean())
    agree_clear = float((ids[clear] == g14["b_ids"][clear]).mean())
    rel = np.abs(probs - g14["b_probs"]) / g14["b_probs"]
    log(f"decode_glyphs {precision} vs reference, case B: clear fraction {clear.mean():.3f}; ids equal on {agree:.3f} of all, "
        f"{agree_clear:.3f} of clear glyphs; probs rel median {np.median(rel):.2e} max {rel.max():.2e}")
    if gate is None:
        assert clear.mean() >= 0.9
        np.testing.assert_array_equal(ids[clear], g14["b_ids"][clear])
        assert rel.max() <= 1e-3
    else:
        assert agree_clear >= gate          # measured on MI355X: bf16 0.996, fp16 1.000 of the clear glyphs


@pytest.mark.parametrize("precision", ["fp32", "fp16x3", "bf16", "fp16"])
def test_decode_glyphs_batch_independence(precision):
    model = model_for(precision)
    rng = np.random.default_rng(7)
    F = torch.from_numpy(rng.normal(0.0, 1.0, (1500, 100)).astype(np.float32)).to(DEV)
    for n in (1, 63, 64, 65, 1500):
        ids, probs = decode_glyphs(model, F[:n], return_tensors=True)
        ids, probs = ids.cpu().numpy(), probs.cpu().numpy()
        rows = sorted({0, n - 1, min(63, n - 1), min(64, n - 1)} | set(rng.integers(0, n, 6).tolist()))
        for i in rows:
            a_ids, a_probs = decode_glyphs(model, F[i:i + 1])
            assert a_ids[0] == ids[i] and a_probs.view(np.int32)[0] == probs.view(np.int32)[i], (precision, n, i)


def test_reference_call_sequence_matches_batched_softmax(g14):
    model = model_for("fp32")
    decoder = CodeDecoder(model.decoder)
    decoder.to(device=DEV)
    decoder.eval()
    feats = g14["b_features"][:40]
    with torch.no_grad():
        batched = decoder(torch.from_numpy(feats).to(DEV))
    assert isinstance(batched, tuple) and [t.shape for t in batched] == [(40, m) for m in MOD]
    for i in (0, 1, 17, 39):
        with torch.no_grad():
            one = decoder(torch.from_numpy(feats[i]).to(device=DEV).unsqueeze(0))       # test_image1_torch.py:273
        for k in range(3):
            assert torch.equal(one[k][0], batched[k][i])
    ids, probs = decode_glyphs(decoder, feats)
    o_ids, o_probs = glyph_oracle.decode_rows(*[t.cpu().numpy() for t in batched])
    np.testing.assert_array_equal(ids, o_ids)


def test_model_without_decoder_raises_cleanly():
    from findtextcenternet_amd.model import FtcModel
    m = FtcModel(deterministic_state_dict(0, "s", with_decoder=False), "fp32", "s")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    rows = torch.zeros((4, 128), dtype=torch.float32, device=DEV)
    out = torch.empty(16, dtype=torch.int64, device=DEV)
    rc = L.load().ftc_glyph_decode(m.handle, ws.data_ptr(), rows.data_ptr(), 4, out.data_ptr(), out.data_ptr(), None, None, None,
                                   ws.data_ptr(), stream())
    assert rc == -1 and b"decoder" in L.load().ftc_last_error()
    m.close()


def test_page_glyphs_vs_oracle_on_gpu_softmax():
    from PIL import Image
    from findtextcenternet_amd import page
    model = model_for("fp32")
    det = CenterNetDetector(model.detector)
    det.to(device=DEV)
    det.eval()
    img = np.asarray(Image.open(os.path.join(HERE, "golden", "test1_padded.png")).convert("RGB"))
    pd = page.PageDetector(det, cut_off=0.4, batch=1, variant="demo")
    loc, gf, _, _ = pd.detect_page(img)
    decoder = CodeDecoder(model.decoder).eval()
    ids, probs = decode_glyphs(decoder, gf)
    assert ids.shape == (len(gf),) and probs.shape == (len(gf),)
    if len(gf):
        _, _, soft = glyph_decode_device(model, torch.from_numpy(np.ascontiguousarray(gf, dtype=np.float32)).to(DEV), with_softmax=True)
        o_ids, o_probs = glyph_oracle.decode_rows(*[s.cpu().numpy() for s in soft])
        np.testing.assert_array_equal(ids, o_ids)
        assert np.abs(probs - o_probs).max() <= 1e-6 * o_probs.max()
    log(f"page test1_padded.png (demo variant, fp32, model 's'): {len(gf)} glyphs decoded in one call")
