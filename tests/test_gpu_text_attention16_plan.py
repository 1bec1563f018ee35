"""-m gpu: the 16-bit attention inside the recognizer's plans (ftc_text_set_attention, ``Transformer(attention=)``; include/ftc_text_attention16.h).

* the default is today's: ``attention=None`` and ``"fp32"`` give the same bits in all four precisions, and no setting changes a launch count;
* the switch is wired: one handle switched with ftc_text_set_attention gives a fresh ``attention="bf16"`` model's bits, the two settings' teacher-forced
  logits differ, ``"match"`` resolves as documented, junk is refused;
* accuracy, by the gates the project takes from the reference (never from this code): with ``attention="match"`` in bf16 and fp16 the teacher-forced
  logits and the encoder output of the g15 rows stay within 2 x the deviation of the reference's own bfloat16-autocast run from its float64 run, and the
  share of pass-0 codes that differ from the fixture's is at most twice the reference's own and at most 10 % -- the bounds of
  tests/test_gpu_text.py::test_teacher_forced_logits_and_encoder_vs_float64 and ::test_sixteen_bit_first_pass_codes, whose reference side ran its
  attention under bf16 autocast itself;
* rows of a batch are bitwise the rows alone;
* ftc_text_predict_compact is bitwise ftc_text_predict with the setting on: the 16-bit kernel's kv_row path inside a plan.
"""
import numpy as np
import pytest
import torch

import text_fixture as TF
from compact_harness import DEV, SMALL, bench_rows, passes_per_row
from findtextcenternet_amd import ModelDimensions, OCR_hip_Processer, Transformer, TransformerPredictor, recognizer_state_dict
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.transformer import predict_device, teacher_forced

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "fp16x3", "bf16", "fp16")
MATCH = {"fp32": "fp32", "fp16x3": "fp32", "bf16": "bf16", "fp16": "fp16"}
GAIN = 100.0          # tests/test_gpu_text_compact.py: at this gain the eight rows of the small model stop after different numbers of passes
_SMALL = {}
_FULL = {}


def log(msg):
    print("[attention16 plan] " + msg)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def small(precision, attention, fresh=False):
    key = (precision, attention)
    if fresh or key not in _SMALL:
        m = Transformer(**SMALL.__dict__, precision=precision, attention=attention)
        m.load_state_dict(recognizer_state_dict(1, SMALL, gain=GAIN))
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(DEV)
        m2.eval()
        if fresh:
            return m, m2
        _SMALL[key] = (m, m2)
    return _SMALL[key]


def full(precision, gain):
    """One full-size Transformer(attention="match") per precision on the g15 weights; the output heads are rewritten in place for another gain."""
    g = TF.load()
    if precision not in _FULL:
        m = Transformer(**ModelDimensions().__dict__, precision=precision, attention="match")
        m.load_state_dict(TF.state_dict_for(g, gain))
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(DEV)
        m2.eval()
        _FULL[precision] = [m, m2, gain]
    ent = _FULL[precision]
    if ent[2] != gain:
        sd = TF.state_dict_for(g, gain)
        with torch.no_grad():
            for i in range(3):
                getattr(ent[0].decoder.out_layers, str(i)).weight.copy_(sd[f"decoder.out_layers.{i}.weight"])
        ent[2] = gain
    return ent[0], ent[1]


def _predict(m2, x, compact=False):
    out = predict_device(m2._engine, x, trace=True, compact=compact)
    torch.cuda.synchronize()
    return out


def _equal(a, b, what):
    assert bits(a[0]) == bits(b[0]), f"{what}: ids differ"
    assert bits(a[1]) == bits(b[1]), f"{what}: probs differ"
    for x, y, name in zip(a[2], b[2], ("tokens", "codes", "probs")):
        assert bits(x) == bits(y), f"{what}: trace_{name} differs"
    assert a[3] == b[3], f"{what}: passes_run differs"


# ---- the default is today's --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_default_and_fp32_are_the_same_bits(precision):
    x = torch.from_numpy(bench_rows(7)[:4].copy()).to(DEV)
    (m, a2), (n, b2) = small(precision, None), small(precision, "fp32")
    assert m.attention == n.attention == "fp32"
    _equal(_predict(a2, x), _predict(b2, x), precision)
    assert int(L.load().ftc_text_get_attention(a2._engine.handle)) == L.F32


def test_launch_counts_are_equal_in_every_setting():
    for precision in PRECISIONS:
        base = small(precision, None)[0]._engine.launch_counts()
        for attention in ("fp32", "fp16", "bf16", "match"):
            assert small(precision, attention)[0]._engine.launch_counts() == base, (precision, attention)
    assert base["decoder_pass"] > 0 and base["encoder"] > 0


# ---- the switch is wired -----------------------------------------------------------------------------------------------------------------

def test_match_resolves_by_precision_and_junk_is_refused():
    for precision in PRECISIONS:
        m = Transformer(**SMALL.__dict__, precision=precision, attention="match")
        assert m.attention == MATCH[precision]
        m._engine.create()
        assert int(L.load().ftc_text_get_attention(m._engine.handle)) == {"fp32": L.F32, "fp16": L.F16, "bf16": L.BF16}[m.attention]
    for junk in ("fp64", "bfloat16", "fp16x3", "FP16", 16):
        with pytest.raises(ValueError):
            Transformer(**SMALL.__dict__, attention=junk)
    lib = L.load()
    eng = small("fp32", None)[0]._engine
    eng.create()
    h = eng.handle
    for junk in (3, -1, 7):
        assert lib.ftc_text_set_attention(h, junk) < 0 and lib.ftc_last_error()
        assert int(lib.ftc_text_get_attention(h)) == L.F32
    assert lib.ftc_text_set_attention(None, L.BF16) < 0 and int(lib.ftc_text_get_attention(None)) == -1
    import inspect
    assert inspect.signature(OCR_hip_Processer.__init__).parameters["text_attention"].default is None


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_handle_switched_is_a_fresh_model_of_that_setting(precision):
    lib = L.load()
    x = torch.from_numpy(bench_rows(7)[:4].copy()).to(DEV)
    m, m2 = small(precision, None, fresh=True)
    _, want2 = small(precision, "bf16")
    before = _predict(m2, x)
    before = (before[0].clone(), before[1].clone(), [t.clone() for t in before[2]], before[3])
    tok = torch.full((4, 400), L.TEXT_MASK_TOKEN, dtype=torch.int64)
    _, lg32 = teacher_forced(m._engine, x, tok)
    h = m._engine.handle
    assert lib.ftc_text_set_attention(h, L.BF16) == 0 and int(lib.ftc_text_get_attention(h)) == L.BF16
    after = _predict(m2, x)
    _equal(after, _predict(want2, x), f"{precision}: the switched handle against a fresh attention='bf16' model")
    _, lg16 = teacher_forced(m._engine, x, tok)
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for a, b in zip(lg32, lg16)), "the setting changed no logit: the plans were not rebuilt"
    d = max(float((a - b).abs().max()) for a, b in zip(lg32, lg16))
    log(f"{precision}: largest logit difference between the fp32 and the bf16 attention {d:.3e}")
    assert lib.ftc_text_set_attention(h, L.F32) == 0
    _equal(_predict(m2, x), before, f"{precision}: switched back")


# ---- accuracy by the reference's own gates ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_teacher_forced_logits_and_encoder_within_the_reference_gates(precision):
    g = TF.load()
    worst = worst_enc = 0.0
    for r in (int(v) for v in g["logit_rows"]):
        model, _ = full(precision, float(g["gains"][r]))
        assert model.attention == precision
        x = torch.from_numpy(TF.row_input(g, r))[None].to(DEV)
        ks = [int(k) for k in g["logit_passes"]]
        with torch.no_grad():
            enc, outs = teacher_forced(model._engine, x, TF.tokens_of(g, r, ks[0])[None], [TF.tokens_of(g, r, k)[None] for k in ks[1:]])
        for k, lg in zip(ks, outs):
            _, l64 = TF.stored_logits(g, r, k)
            for h in range(3):
                got = lg[h][0].cpu().numpy()[g["logit_pos"]].astype(np.float64)
                err = float(np.abs(got - l64[h]).max())
                bound = 2 * g["bf16_logit_dev"][r]
                worst = max(worst, err / bound)
                log(f"{precision} + {precision} attention, row {r} pass {k} head {h}: logit error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
                assert err <= bound
        if r == int(g["enc_row"]):
            e64 = g["enc32"].astype(np.float64) + g["enc64_minus32"]
            err = float(np.abs(enc[0].cpu().numpy()[g["enc_pos"]] - e64).max())
            bound = 2 * g["bf16_enc_dev"][r]
            worst_enc = err / bound
            log(f"{precision} + {precision} attention, encoder output row {r}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
            assert err <= bound
    log(f"{precision} + {precision} attention: worst logit error / bound {worst:.3f}, encoder error / bound {worst_enc:.3f}")


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_first_pass_codes_within_the_reference_share(precision):
    g = TF.load()
    differ = total = 0
    for r in range(len(g["lengths"])):
        _, model2 = full(precision, float(g["gains"][r]))
        x = torch.from_numpy(TF.row_input(g, r))[None].to(DEV)
        _, _, tr, _ = predict_device(model2._engine, x, trace=True)
        differ += int((tr[1][0, 0].cpu().numpy() != g["codes"][r, 0]).sum())
        total += 400
    ref_share = float(g["bf16_code_share"].mean())
    bound = min(2 * ref_share, 0.10)
    log(f"{precision} + {precision} attention, pass 0: {differ} of {total} codes differ ({differ / total:.4f}); the reference's bf16 autocast: {ref_share:.4f}; "
        f"share / bound {differ / total / bound:.3f}")
    assert differ / total <= bound


# ---- batch independence and the compact loop --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_rows_of_a_batch_are_bitwise_the_rows_alone(precision):
    _, m2 = small(precision, "match")
    X = bench_rows(7)[:4]
    both = _predict(m2, torch.from_numpy(X.copy()).to(DEV))
    both = (both[0].clone(), both[1].clone())
    seen = set()
    for r in range(4):
        one = _predict(m2, torch.from_numpy(X[r:r + 1].copy()).to(DEV))
        assert bits(one[0][0]) == bits(both[0][r]) and bits(one[1][0]) == bits(both[1][r]), f"{precision}: row {r} of 4 differs from the row alone"
        seen.add(bits(one[0][0]))
    assert len(seen) > 1


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_compact_loop_is_bitwise_the_plain_loop_with_the_setting_on(precision):
    _, m2 = small(precision, "match")
    X = bench_rows(7)
    for name, x in (("in order", torch.from_numpy(X).to(DEV)), ("reversed", torch.from_numpy(X[::-1].copy()).to(DEV))):
        old = _predict(m2, x)
        old = (old[0].clone(), old[1].clone(), [t.clone() for t in old[2]], old[3])
        new = _predict(m2, x, compact=True)
        _equal(new[:4], old, f"{precision} {name}")
        rows_run = new[4]
        ran = passes_per_row(old[2][0])
        log(f"{precision} {name}: passes per row {ran.sum(0).tolist()}, rows_run {rows_run}")
        assert rows_run == ran.sum(1).tolist()
        # the condition on the inputs: without it nothing was compacted and the kv_row path did not run
        assert sum(rows_run) < 8 * old[3] and any(0 < n < 8 for n in rows_run), f"{precision} {name}: no pass ran on a compact batch: {rows_run}"
    assert int(L.load().ftc_text_get_attention(m2._engine.handle)) == {"bf16": L.BF16, "fp16": L.F16}[precision]
