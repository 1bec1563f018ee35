"""Text recognizer, host side (no GPU): the fixture g15 against the plain-torch restatement tests/text_oracle.py, the state_dict schema,
the selection step from stored logits, and the host-only parts of include/ftc_text.h (packing, refusals, exported symbols)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import text_fixture as TF
import text_oracle as O
from findtextcenternet_amd import ModelDimensions, Transformer, TransformerPredictor
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.schema import transformer_schema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g15():
    return TF.load()


def test_fixture_meets_its_own_design(g15):
    g = g15
    assert (g["passes"] == 8).any() and (g["stops"] == "early").any()
    assert g["lengths"].min() < 100 and g["lengths"].max() >= 398
    x = TF.padded_inputs(g, [1])[0]
    assert not x[200:212].any() and x[199].any() and x[212].any()             # the all-zero stretch inside the line
    assert 0.1 <= g["share_above_09_pass0"][1] <= 0.9
    assert len(g["invalid_best"]) > 0
    lim = g["margin_factor"] * g["d_p"][:, None]
    assert float(g["margin_factor"]) == 10.0
    assert (g["m_thr"] >= lim).all() and (g["m_stop"] >= lim).all() and (g["m_gap_over_need"] >= g["margin_factor"]).all()


def test_schema_equals_fixture_names_and_shapes(g15):
    sch = transformer_schema(ModelDimensions())
    assert list(sch.keys()) == list(g15["names"]) and len(sch) == 416
    assert [",".join(str(s) for s in shape) for shape, _ in sch.values()] == list(g15["shapes"])


def test_load_state_dict_round_trip(g15):
    sd = TF.state_dict_for(g15, 32.0)
    model = Transformer(**ModelDimensions().__dict__)
    assert list(model.state_dict().keys()) == list(g15["names"])
    model.load_state_dict(sd)
    back = model.state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    model2 = TransformerPredictor(model.encoder, model.decoder)
    model2.to("cpu"); model2.eval()
    assert model2.head_num == 12 and model2.max_len == 400
    with pytest.raises(RuntimeError, match="MI355X"):
        model2(torch.zeros(1, 5, 106))


def test_oracle_reproduces_fixture(g15):
    """The float32 restatement takes the fixture's path exactly (every pass: tokens in, codes out, stop) and its logits are within
    2 x d_logit of the stored float64 values."""
    g = g15
    for r in range(len(g["lengths"])):
        sd = TF.state_dict_for(g, float(g["gains"][r]))
        keep = tuple(int(k) for k in g["logit_passes"]) if r in g["logit_rows"] else ()
        with torch.no_grad():
            tr = O.predict_row(sd, torch.from_numpy(TF.row_input(g, r)), keep_logits=keep)
        n = int(g["passes"][r])
        assert len(tr["codes"]) == n and tr["stop"][1] == str(g["stops"][r])
        for k in range(n):
            np.testing.assert_array_equal(tr["tokens"][k].numpy(), g["tokens"][r, k])
            np.testing.assert_array_equal(tr["codes"][k].numpy(), g["codes"][r, k])
            assert np.abs(tr["scores"][k].numpy() - g["scores32"][r, k]).max() <= 2 * g["d_p"][r]
        for k in keep:
            _, l64 = TF.stored_logits(g, r, k)
            for h in range(3):
                err = np.abs(tr["logits"][k][h][g["logit_pos"]].numpy().astype(np.float64) - l64[h]).max()
                print(f"[text] oracle fp32 row {r} pass {k} head {h}: logit error {err:.2e} (d_logit {g['d_logit'][r]:.2e})")
                assert err <= 2 * g["d_logit"][r]
        if r == int(g["enc_row"]):
            e64 = g["enc32"].astype(np.float64) + g["enc64_minus32"]
            assert np.abs(tr["enc_out"][g["enc_pos"]].numpy() - e64).max() <= 2 * g["d_enc"]


def test_select_restatement_from_stored_logits(g15):
    """The selection step on the fixture's float32 logits gives the fixture's codes and scores bit for bit (torch form), and the NumPy
    form used against the GPU kernel gives the same codes from the same three largest entries."""
    g = g15
    for r in g["logit_rows"]:
        for k in g["logit_passes"]:
            l32, _ = TF.stored_logits(g, int(r), int(k))
            lg = [torch.from_numpy(a) for a in l32]
            code, score = O.select(lg)
            np.testing.assert_array_equal(code.numpy(), g["codes"][r, k][g["logit_pos"]])
            np.testing.assert_array_equal(score.numpy().view(np.int32), g["scores32"][r, k][g["logit_pos"]].view(np.int32))
            tp, ti = O.top3(lg)
            c2, s2 = O.select_host(tp.numpy(), ti.numpy())
            np.testing.assert_array_equal(c2, code.numpy())
            assert np.abs(s2 - score.numpy()).max() <= 4e-6 * max(score.numpy().max(), 1e-30)


def test_library_host_select_on_stored_logits(g15):
    """ftc_text_select_host (the select kernel's host restatement, same arithmetic as the kernel) on the fixture's float32 logits: the
    fixture's codes exactly, its scores within 10 x d_p, the three largest entries' indices those of torch.topk wherever the rank is
    not a tie (the tails of a peaked softmax are exact zeros; the fixture's m_top34 records it)."""
    g = g15
    lib = L.load()
    for r in (int(v) for v in g["logit_rows"]):
        for k in (int(v) for v in g["logit_passes"]):
            l32, _ = TF.stored_logits(g, r, k)
            lg = [np.ascontiguousarray(a, dtype=np.float32) for a in l32]
            n = lg[0].shape[0]
            codes, scores = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float32)
            tp, ti = np.empty((n, 3, 3), dtype=np.float32), np.empty((n, 3, 3), dtype=np.int32)
            assert lib.ftc_text_select_host(lg[0].ctypes.data, lg[1].ctypes.data, lg[2].ctypes.data, 1091, 1093, 1097, n, codes.ctypes.data,
                                            scores.ctypes.data, tp.ctypes.data, ti.ctypes.data) == 0
            np.testing.assert_array_equal(codes, g["codes"][r, k][g["logit_pos"]])
            assert np.abs(scores - g["scores32"][r, k][g["logit_pos"]]).max() <= 10 * g["d_p"][r]
            rtp, rti = O.top3([torch.from_numpy(a) for a in lg])
            clear = O.clear_top3([torch.from_numpy(a) for a in lg]).numpy()
            assert clear[:, :, 0].all()                       # the largest entry of every head is never a tie in the fixture
            np.testing.assert_array_equal(ti[clear], rti.numpy()[clear])
            assert np.abs(tp - rtp.numpy()).max() <= 1e-6
    assert lib.ftc_text_select_host(None, None, None, 1091, 1093, 1097, 1, None, None, None, None) == -1


def test_select_rules_on_synthetic_candidates():
    """First best choice on exact ties, score 0 and choice 0 when all 27 code points are invalid, the 0x3FFFF bound."""
    ti = np.zeros((3, 3, 3), dtype=np.int64)
    tp = np.zeros((3, 3, 3), dtype=np.float32)
    # position 0: residues of code points 65 / 66 / 67 in ranks 0 / 1 / 2, all nine probabilities equal -> choice (0,0,0) = 65 wins the tie
    for h, m in enumerate(O.MODULI):
        ti[0, h] = [65 % m, 66 % m, 67 % m]
    tp[0] = 1.0 / 3
    # position 1: every choice is an invalid code point (residues of numbers far above the limit)
    big = [0x40000 + 1000, 0x50000 + 77, 0x60000 + 5]
    for h, m in enumerate(O.MODULI):
        ti[1, h] = [b % m for b in big]
    tp[1] = [[0.8, 0.1, 0.05]] * 3
    # position 2: the best choice is invalid, the second-best (rank 1 everywhere) is the valid code point 0x3FFFF itself
    for h, m in enumerate(O.MODULI):
        ti[2, h] = [(0x40000) % m, 0x3FFFF % m, 5 % m]
    tp[2] = [[0.6, 0.3, 0.05]] * 3
    code, score = O.select_host(tp, ti)
    assert code[0] == 65 and np.isclose(score[0], 1 / 3, rtol=1e-6)
    assert code[1] == big[0] and score[1] == 0
    c_t, s_t, _ = O.select_from_top3(torch.from_numpy(tp), torch.from_numpy(ti))
    np.testing.assert_array_equal(c_t.numpy(), code)
    assert code[2] == 0x3FFFF and np.isclose(score[2], 0.3, rtol=1e-6)
    assert int(O.codepoint(0x3041 % 1091, 0x3041 % 1093, 0x3041 % 1097)) == 0x3041


def _tensor_array(sd):
    keep, arr = [], (L.Tensor * len(sd))()
    for i, (k, v) in enumerate(sd.items()):
        t = v.contiguous()
        kb = k.encode()
        keep.append((t, kb))
        arr[i].name, arr[i].data, arr[i].dtype, arr[i].ndim = kb, t.data_ptr(), L.F32, t.dim()
        for j, d in enumerate(t.shape):
            arr[i].shape[j] = d
    return arr, keep


def _dims(**kw):
    d = dict(enc_input_dim=106, embed_dim=128, head_num=2, enc_block_num=1, dec_block_num=1, max_enc_seq_len=400, max_dec_seq_len=400, reserved=0)
    d.update(kw)
    return L.TextDims(*[d[n] for n, _ in L.TextDims._fields_])


def test_text_create_packs_without_a_gpu_and_refuses_bad_input():
    from findtextcenternet_amd.weights import recognizer_state_dict
    lib = L.load()
    small = ModelDimensions(embed_dim=128, head_num=2, enc_block_num=1, dec_block_num=1)
    sd = recognizer_state_dict(3, small)
    arr, keep = _tensor_array(sd)
    for prec, per in ((L.F32, 4), (3, 4), (L.BF16, 2), (L.F16, 2)):
        h = C.c_void_p()
        assert lib.ftc_text_create(arr, len(sd), C.byref(_dims()), prec, C.byref(h)) == 0, lib.ftc_last_error()
        nbytes = lib.ftc_text_weights_bytes(h)
        gemm_params = sum(v.numel() for k, v in sd.items() if v.dim() == 2 and "encoding" not in k and "decoder.embed" not in k)
        assert nbytes > gemm_params * per
        assert lib.ftc_text_workspace_bytes(h, 1) > 0 and lib.ftc_text_workspace_bytes(h, 8) > 7 * lib.ftc_text_workspace_bytes(h, 1)
        assert lib.ftc_text_workspace_bytes(h, 0) == -1 and b"B must be" in lib.ftc_last_error()
        assert lib.ftc_text_launch_count(h, 0) == 2 + 9 + 1 and lib.ftc_text_launch_count(h, 2) == 1 + 13 + 3
        lib.ftc_text_destroy(h)
    h = C.c_void_p()
    assert lib.ftc_text_create(arr, len(sd), C.byref(_dims(head_num=4)), L.F32, C.byref(h)) == -1 and b"width 64" in lib.ftc_last_error()
    assert lib.ftc_text_create(arr, len(sd), C.byref(_dims(embed_dim=100)), L.F32, C.byref(h)) == -1 and b"width 64" in lib.ftc_last_error()
    assert lib.ftc_text_create(arr, len(sd), C.byref(_dims(max_dec_seq_len=512)), L.F32, C.byref(h)) == -1 and b"400" in lib.ftc_last_error()
    assert lib.ftc_text_create(arr, len(sd), C.byref(_dims()), 7, C.byref(h)) == -1 and b"precision" in lib.ftc_last_error()
    assert lib.ftc_text_create(arr, len(sd), C.byref(_dims(dec_block_num=2)), L.F32, C.byref(h)) == -1 and b"missing tensor decoder.blocks.1" in lib.ftc_last_error()
    bad = dict(sd)
    bad["encoder.norm.weight"] = torch.zeros(64)
    arr2, keep2 = _tensor_array(bad)
    assert lib.ftc_text_create(arr2, len(bad), C.byref(_dims()), L.F32, C.byref(h)) == -1 and b"encoder.norm.weight" in lib.ftc_last_error()


def test_python_seam_refuses_what_it_does_not_support():
    with pytest.raises(ValueError, match="multiple of head_num"):
        Transformer(106, 100, 12, max_enc_seq_len=400, max_dec_seq_len=400)
    with pytest.raises(NotImplementedError, match="width 64"):
        Transformer(106, 768, 6, max_enc_seq_len=400, max_dec_seq_len=400)
    with pytest.raises(NotImplementedError, match="400"):
        Transformer(106, 128, 2)                       # the reference's default tables are 5000 long
    with pytest.raises(ValueError, match="precision"):
        Transformer(106, 128, 2, max_enc_seq_len=400, max_dec_seq_len=400, precision="int8")
    m = Transformer(106, 128, 2, 1, 1, 400, 400, dropout=0.1)
    m.train()
    with pytest.raises(NotImplementedError, match="eval"):
        m(torch.zeros(1, 4, 106), torch.zeros(1, 400, dtype=torch.long))
    with pytest.raises(TypeError):
        TransformerPredictor(m.encoder, Transformer(106, 128, 2, 1, 1, 400, 400).decoder)


def test_every_text_symbol_of_the_header_is_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "ftc_text.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ftc_text_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(L.TEXT_EXPORTS)
    lib = L.load()
    for s in declared:
        assert getattr(lib, s) is not None
    assert lib.ftc_text_abi_version() == 1 == L.FTC_TEXT_ABI_VERSION
    assert lib.ftc_abi_version() == 13                 # include/ftc.h is not touched by the text surface
    assert not set(L.TEXT_EXPORTS) & set(L.EXPORTS)
