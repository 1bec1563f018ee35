"""Glyph code-point decode, host side (no GPU): the CPU restatement against the reference's recorded decode (g14), the package's CRT
constants, the C ABI's argument checks and the public names the demo script imports."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import glyph_oracle
from findtextcenternet_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
G14 = os.path.join(HERE, "golden", "g14_glyph_decode.npz")
MOD = (1091, 1093, 1097)


@pytest.fixture(scope="module")
def g14():
    return np.load(G14)


def b_soft_rows(g, k):
    """Case B's stored softmax entries of head k as dense rows (zeros elsewhere: below 0.005, they never decide)."""
    ptr, idx, val = g[f"b_soft{k}_ptr"], g[f"b_soft{k}_idx"].astype(np.int64), g[f"b_soft{k}_val"]
    rows = np.zeros((len(ptr) - 1, MOD[k]), np.float32)
    for i in range(len(ptr) - 1):
        rows[i, idx[ptr[i]:ptr[i + 1]]] = val[ptr[i]:ptr[i + 1]]
    return rows


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_oracle_reproduces_reference_case_a(g14):
    soft = [torch.softmax(torch.from_numpy(g14[f"a_logits{k}"].astype(np.float32)), dim=-1).numpy() for k in range(3)]
    ids, probs = glyph_oracle.decode_rows(*soft)
    ok = ~g14["a_flag"]
    assert ok.sum() >= 80
    np.testing.assert_array_equal(ids[ok], g14["a_ids"][ok])
    assert ulps(probs[ok], g14["a_probs"][ok]).max() <= 4
    # the planted cases are all there: valid picks, all-invalid glyphs (returned with an out-of-range id)
    assert (g14["a_ids"] <= 0x10FFFF).sum() >= 40 and (g14["a_ids"] > 0x10FFFF).sum() >= 10


def test_oracle_reproduces_reference_case_b(g14):
    ids, probs = glyph_oracle.decode_rows(*[b_soft_rows(g14, k) for k in range(3)])
    np.testing.assert_array_equal(ids, g14["b_ids"])
    assert ulps(probs, g14["b_probs"]).max() <= 4


def test_crt_constants_match_calc_predid_table(g14):
    from findtextcenternet_amd import crt_codepoint
    from findtextcenternet_amd.glyphs import CRT_E, CRT_MODULUS
    r = g14["crt_residues"]
    np.testing.assert_array_equal(crt_codepoint(r[:, 0], r[:, 1], r[:, 2]), g14["crt_ids"])
    assert CRT_MODULUS == 1091 * 1093 * 1097
    for k, m in enumerate(MOD):
        assert all(CRT_E[k] % mm == (1 if mm == m else 0) for mm in MOD)
    assert [glyph_oracle.residues_to_codepoint(*map(int, t)) for t in r[:200]] == g14["crt_ids"][:200].tolist()


def test_library_exports_glyph_entry_points():
    lib = L.load()
    for name in ("ftc_glyph_select", "ftc_glyph_decode", "ftc_glyph_decode_workspace_bytes"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
    assert lib.ftc_abi_version() == L.FTC_ABI_VERSION == 13


def test_glyph_select_rejects_bad_arguments_without_a_device():
    lib = L.load()
    dummy = C.c_void_p(16)
    # n < 0
    assert lib.ftc_glyph_select(dummy, dummy, dummy, 1091, 1093, 1097, -1, None, None, None, dummy, dummy, None) == -1
    assert b"n < 0" in lib.ftc_last_error()
    # ld < m
    assert lib.ftc_glyph_select(dummy, dummy, dummy, 1090, 1093, 1097, 4, None, None, None, dummy, dummy, None) == -1
    assert b"ld" in lib.ftc_last_error()
    # null outputs / inputs
    assert lib.ftc_glyph_select(dummy, dummy, dummy, 1091, 1093, 1097, 4, None, None, None, None, dummy, None) == -1
    assert b"null" in lib.ftc_last_error()
    assert lib.ftc_glyph_select(None, dummy, dummy, 1091, 1093, 1097, 4, None, None, None, dummy, dummy, None) == -1
    # n == 0 is a no-op
    assert lib.ftc_glyph_select(None, None, None, 1091, 1093, 1097, 0, None, None, None, None, None, None) == 0


def test_glyph_decode_rejects_bad_arguments_and_models_without_decoder():
    from findtextcenternet_amd import deterministic_state_dict
    from findtextcenternet_amd.model import FtcModel
    lib = L.load()
    dummy = C.c_void_p(16)
    assert lib.ftc_glyph_decode(None, dummy, dummy, 4, dummy, dummy, None, None, None, dummy, None) == -1
    assert lib.ftc_glyph_decode_workspace_bytes(None, 4) == -1
    nodec = FtcModel(deterministic_state_dict(0, "s", with_decoder=False), "fp32", "s")
    assert lib.ftc_glyph_decode_workspace_bytes(nodec.handle, 4) == -1
    assert b"decoder" in lib.ftc_last_error()
    assert lib.ftc_glyph_decode(nodec.handle, dummy, dummy, 4, dummy, dummy, None, None, None, dummy, None) == -1
    assert b"decoder" in lib.ftc_last_error()
    withdec = FtcModel(deterministic_state_dict(0, "s"), "fp32", "s")
    assert lib.ftc_glyph_decode(withdec.handle, dummy, dummy, -3, dummy, dummy, None, None, None, dummy, None) == -1
    assert b"n_rows < 0" in lib.ftc_last_error()
    assert lib.ftc_glyph_decode(withdec.handle, dummy, dummy, 4, None, dummy, None, None, None, dummy, None) == -1
    assert b"null" in lib.ftc_last_error()
    assert lib.ftc_glyph_decode(withdec.handle, None, None, 0, None, None, None, None, None, None, None) == 0
    assert lib.ftc_glyph_decode_workspace_bytes(withdec.handle, 0) == 0
    # the padded buckets: one plan per bucket, workspace grows with the bucket only
    w1, w64, w65, w96 = (int(lib.ftc_glyph_decode_workspace_bytes(withdec.handle, n)) for n in (1, 64, 65, 96))
    assert w1 == w64 > 0 and w65 == w96 > w64
    nodec.close()
    withdec.close()


def test_demo_import_line_and_code_decoder_module():
    from findtextcenternet_amd import TextDetectorModel, CenterNetDetector, CodeDecoder  # noqa: F401  (test_image1_torch.py:21)
    import findtextcenternet_amd as ftc
    assert {"CodeDecoder", "decode_glyphs"} <= set(ftc.__all__)
    model = TextDetectorModel(pre_weights=False, model_size="s")
    decoder = CodeDecoder(model.decoder)
    keys = list(decoder.state_dict().keys())
    assert keys == ["decoder." + k for k in model.decoder.state_dict().keys()]
    assert keys[0] == "decoder.blocks.0.0.weight" and all(k.startswith("decoder.blocks.") for k in keys)
    before = [(p.data_ptr(), p.device) for p in model.parameters()]
    assert decoder.to(device="cuda") is decoder                     # the reference's decoder.to(device=device): the owner's weights stay put
    assert [(p.data_ptr(), p.device) for p in model.parameters()] == before
    decoder.eval()
    assert not decoder.training
    with pytest.raises(RuntimeError, match="MI355X"):
        decoder(torch.zeros(1, 100))
    with pytest.raises(TypeError):
        CodeDecoder(torch.nn.Linear(2, 2))


def test_decode_glyphs_zero_glyphs_returns_reference_empty_result():
    from findtextcenternet_amd import CodeDecoder, TextDetectorModel, decode_glyphs
    model = TextDetectorModel(pre_weights=False, model_size="s")
    for dec in (CodeDecoder(model.decoder), model):
        ids, probs = decode_glyphs(dec, np.zeros((0, 100), np.float32))
        ref = np.atleast_1d([])
        assert ids.shape == probs.shape == ref.shape and ids.dtype == probs.dtype == ref.dtype
    with pytest.raises(TypeError):
        decode_glyphs(object(), np.zeros((0, 100), np.float32))
    with pytest.raises(RuntimeError, match="MI355X"):
        decode_glyphs(model, torch.zeros(2, 100))
