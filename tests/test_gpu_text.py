"""Text recognizer on the MI355X: each new kernel against float64 torch on the CPU, the teacher-forced network against the fixture's
float64 values, the free-running mask-predict loop against the fixture's path, batch independence and the NumPy backend.

The free-running fixture (g15) does not reach the loop's no-remask exit (it needs all 400 positions above 0.9) nor is an all-invalid
position guaranteed at a given place: both are covered on synthetic logits in the select / row-update tests below.

Bounds.  Network outputs: fp32 at most 8 x d_logit (the reference's own float32-vs-float64 difference, stored per row, times a margin for
another summation order); fp16x3 at most 1e-3 of the tensor's range (the contract of that mode); bf16 at most 2 x the deviation of the
reference's own bfloat16-autocast run from its float64 run (stored per row); fp16 the bf16 bound.  Kernels: the error of an fp32 sum of
n independently rounded terms grows like sqrt(n) x 2^-24 x the terms' size; the bounds written at each test are 8 x that.  The select
kernel is compared BIT FOR BIT (codes, scores, the three largest entries and their indices) with its host restatement
``ftc_text_select_host``, which runs the same steps in the same order with the same plain-operation exp / log (csrc/text_math.h).

tests/test_gpu_text_exact.py holds the attention, row, padding and swiglu kernels and the recognizer's own GEMM ops to BIT EQUALITY on exact operands
(tests/text_operands.py); the Gaussian tests here stay for what those cannot see, the rounding behaviour on real-valued data."""
import ctypes as C

import numpy as np
import pytest
import torch

import text_fixture as TF
import text_oracle as O
from findtextcenternet_amd import HipTextBackend, ModelDimensions, Transformer, TransformerPredictor, recognize_chunks
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.transformer import predict_device, teacher_forced

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MOD = TF.MOD
EPS = 2.0 ** -24


def log(msg):
    print("[text] " + msg)


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@pytest.fixture(scope="module")
def g15():
    return TF.load()


_MODELS = {}


def model_for(precision, gain):
    """One Transformer per precision; the output heads are rewritten in place for another gain (the engine re-packs on the version change)."""
    g = TF.load()
    if precision not in _MODELS:
        m = Transformer(**ModelDimensions().__dict__, precision=precision)
        m.load_state_dict(TF.state_dict_for(g, gain))
        m2 = TransformerPredictor(m.encoder, m.decoder)
        m2.to(DEV); m2.eval()
        _MODELS[precision] = [m, m2, gain]
    ent = _MODELS[precision]
    if ent[2] != gain:
        sd = TF.state_dict_for(g, gain)
        with torch.no_grad():
            for i in range(3):
                getattr(ent[0].decoder.out_layers, str(i)).weight.copy_(sd[f"decoder.out_layers.{i}.weight"])
        ent[2] = gain
    return ent[0], ent[1]


# ---- 1. kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,heads,Sq,Sk,masked", [(2, 3, 400, 400, True), (1, 12, 400, 400, False), (3, 2, 77, 400, True), (2, 2, 400, 33, True),
                                                  (1, 1, 1, 1, False), (2, 4, 250, 211, True)])
def test_attention_kernel_vs_float64(B, heads, Sq, Sk, masked):
    """|error| <= 8 x sqrt(64 + Sk) x 2^-24 x max|v|: the score is a 64-term dot product of N(0,1) values scaled by 1/8 (size ~1, so the
    error of exp(s) is ~sqrt(64) eps relative), the output a convex combination of Sk values; 8 x the sqrt growth of independent roundings."""
    gen = torch.Generator().manual_seed(B * 1000 + Sq + Sk)
    E = 64 * heads
    ld = 3 * E
    qkv_q = torch.randn(B * Sq, ld, generator=gen)
    qkv_k = torch.randn(B * Sk, ld, generator=gen)
    pad = torch.zeros(B, Sk, dtype=torch.bool)
    if masked:
        pad = torch.rand(B, Sk, generator=gen) < 0.3
        pad[0, :] = False                                   # a fully valid row
        pad[-1, :] = True; pad[-1, Sk // 2] = False         # a row with ONE valid key
    dq, dk = qkv_q.to(DEV), qkv_k.to(DEV)
    out = torch.full((B * Sq, E + 4), 7.0, device=DEV)
    padd = pad.to(torch.uint8).to(DEV)
    rc = L.load().ftc_text_attention(dq.data_ptr(), ld, dk.data_ptr() + 4 * E, ld, dk.data_ptr() + 8 * E, ld, padd.data_ptr() if masked else None,
                                     out.data_ptr(), E + 4, B, heads, Sq, Sk, stream())
    assert rc == 0, L.load().ftc_last_error()
    got = out.cpu()
    assert (got[:, E:] == 7.0).all()                        # the pitch is honoured
    q = qkv_q[:, :E].double().view(B, Sq, heads, 64).transpose(1, 2)
    k = qkv_k[:, E:2 * E].double().view(B, Sk, heads, 64).transpose(1, 2)
    v = qkv_k[:, 2 * E:].double().view(B, Sk, heads, 64).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / 8.0
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * Sq, E)
    err = float((got[:, :E].double() - ref).abs().max())
    bound = 8 * (64 + Sk) ** 0.5 * EPS * float(v.abs().max())
    log(f"attention B{B} h{heads} Sq{Sq} Sk{Sk}: max error {err:.2e} (bound {bound:.2e})")
    assert err <= bound


def _rownorm(a, b, pos_in, gamma, beta, pos_out, tokens, tabs, rows, S, E, want_out=True, want_pos=False):
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    A, Bt, PI, G, Be, PO, T = d(a), d(b), d(pos_in), d(gamma), d(beta), d(pos_out), d(tokens)
    tb = [d(t) for t in tabs] if tabs else [None] * 3
    out = torch.empty(rows, E, device=DEV) if want_out else None
    outp = torch.empty(rows, E, device=DEV) if want_pos else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = L.load().ftc_text_rownorm(p(A), p(Bt), p(PI), p(G), p(Be), p(PO), p(T), p(tb[0]), p(tb[1]), p(tb[2]), p(out), p(outp), rows, S, E, stream())
    assert rc == 0, L.load().ftc_last_error()
    return (None if out is None else out.cpu()), (None if outp is None else outp.cpu())


@pytest.mark.parametrize("E", [768, 128, 1024])
def test_rownorm_forms_vs_float64(E):
    """|error| <= 8 x sqrt(E) x 2^-24 x (max|y| + 1): mean and variance are E-term fp32 sums (sqrt growth of independent roundings, times
    8), the result is (x - mean) * rstd * gamma + beta.  The last case has a row variance of ~1e-5, the size of eps: a wrong eps or an
    unbiased variance moves the result by far more than the bound there."""
    gen = torch.Generator().manual_seed(E)
    S, rows = 400, 400 * 2 + 0
    a, b = torch.randn(rows, E, generator=gen) * 3, torch.randn(rows, E, generator=gen)
    pin, pout = torch.randn(S, E, generator=gen), torch.randn(S, E, generator=gen)
    gamma, beta = torch.rand(E, generator=gen) + 0.5, torch.randn(E, generator=gen) * 0.1
    ln = lambda t: torch.nn.functional.layer_norm(t, (E,), gamma.double(), beta.double())
    rep = lambda t: t.double().repeat(rows // S, 1)
    # (b) encoder input: position table + LayerNorm, second output + next position table
    y, yp = _rownorm(a, None, pin, gamma, beta, pout, None, None, rows, S, E, True, True)
    ref = ln(a.double() + rep(pin))
    bound = 8 * E ** 0.5 * EPS * float(ref.abs().max() + 1)
    e1, e2 = float((y - ref).abs().max()), float((yp - (ref + rep(pout))).abs().max())
    assert e1 <= bound and e2 <= bound, (e1, e2, bound)
    # (c) residual + LayerNorm, two-skip form, single output
    y, _ = _rownorm(a, b, None, gamma, beta, None, None, None, rows, S, E)
    e3 = float((y - ln(a.double() + b.double())).abs().max())
    assert e3 <= bound
    # position table only (the cross-attention key input): exact
    _, yp = _rownorm(a, None, None, None, None, pout, None, None, rows, S, E, False, True)
    assert torch.equal(yp, a + pout.repeat(rows // S, 1))
    # (a) token embedding: three table rows + position + LayerNorm
    tabs = [torch.randn(m, E, generator=gen) for m in MOD]
    tok = torch.randint(0, 0x40000, (rows,), generator=gen)
    tok[:5] = torch.tensor([0, 1, 2, 3, 1091 * 1093])
    y, yp = _rownorm(None, None, pin, gamma, beta, pout, tok, tabs, rows, S, E, True, True)
    x = tabs[0][tok % MOD[0]].double() + tabs[1][tok % MOD[1]].double() + tabs[2][tok % MOD[2]].double() + rep(pin)
    e4 = float((y - ln(x)).abs().max())
    log(f"rownorm E{E}: errors {e1:.2e} {e2:.2e} {e3:.2e} {e4:.2e} (bound {bound:.2e})")
    assert e4 <= bound and float((yp - (ln(x) + rep(pout))).abs().max()) <= bound
    # small variance: eps = 1e-5 and the biased variance decide the result
    small = a * 1e-3 + 2.0
    y, _ = _rownorm(small, None, None, gamma, beta, None, None, None, rows, S, E)
    ref_s = ln(small.double())
    e5 = float((y - ref_s).abs().max())
    wrong_eps = torch.nn.functional.layer_norm(small.double(), (E,), gamma.double(), beta.double(), eps=1e-6)
    assert float((wrong_eps - ref_s).abs().max()) > 100 * bound          # the case does tell the two apart
    # the input's own rounding: x = 2 + 3e-3 z has an ulp of 2.4e-7 against a spread of 3e-3, i.e. 8e-5 relative per element after centring
    bound_s = bound + 2 * 2.0 ** -23 / 3e-3 * float(ref_s.abs().max())
    log(f"rownorm E{E} small variance: error {e5:.2e} (bound {bound_s:.2e})")
    assert e5 <= bound_s
    # rows past a multiple of the workgroup
    y, _ = _rownorm(a[:7], None, None, gamma, beta, None, None, None, 7, S, E)
    assert float((y - ln(a[:7].double())).abs().max()) <= bound


def test_swiglu_vs_float64():
    """|error| <= 8 x 2^-24 x |y| + 1e-7: one expf, one division, two products."""
    gen = torch.Generator().manual_seed(5)
    rows, H = 403, 1536
    x = torch.randn(rows, 2 * H, generator=gen) * 4
    d = x.to(DEV)
    out = torch.empty(rows, H, device=DEV)
    assert L.load().ftc_text_swiglu(d.data_ptr(), out.data_ptr(), rows, H, stream()) == 0
    ref = x[:, :H].double() * torch.nn.functional.silu(x[:, H:].double())
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= 8 * EPS * ref.abs() + 1e-7).all()), float(err.max())


def _select(lg, lds=None, top=True):
    n = lg[0].shape[0]
    codes = torch.empty(n, dtype=torch.int64, device=DEV)
    scores = torch.empty(n, dtype=torch.float32, device=DEV)
    tp = torch.empty(n, 3, 3, dtype=torch.float32, device=DEV) if top else None
    ti = torch.empty(n, 3, 3, dtype=torch.int32, device=DEV) if top else None
    lds = lds or [t.shape[1] for t in lg]
    rc = L.load().ftc_text_select(lg[0].data_ptr(), lg[1].data_ptr(), lg[2].data_ptr(), lds[0], lds[1], lds[2], n, codes.data_ptr(), scores.data_ptr(),
                                  tp.data_ptr() if top else None, ti.data_ptr() if top else None, stream())
    assert rc == 0, L.load().ftc_last_error()
    return codes.cpu().numpy(), scores.cpu().numpy(), (tp.cpu().numpy() if top else None), (ti.cpu().numpy() if top else None)


def _select_host(lg_cpu, lds=None):
    """ftc_text_select_host: the kernel's steps on the CPU with the same plain-operation exp / log (csrc/text_math.h)."""
    lg = [t.contiguous() for t in lg_cpu]
    n = lg[0].shape[0]
    codes, scores = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float32)
    tp, ti = np.empty((n, 3, 3), dtype=np.float32), np.empty((n, 3, 3), dtype=np.int32)
    lds = lds or [t.shape[1] for t in lg]
    rc = L.load().ftc_text_select_host(lg[0].data_ptr(), lg[1].data_ptr(), lg[2].data_ptr(), lds[0], lds[1], lds[2], n, codes.ctypes.data, scores.ctypes.data,
                                       tp.ctypes.data, ti.ctypes.data)
    assert rc == 0, L.load().ftc_last_error()
    return codes, scores, tp, ti


def _check_select_against_host(lg_cpu, what, tie_rows=()):
    """Kernel == host restatement BIT FOR BIT in all four outputs (codes, scores, the three largest entries and their indices).  Besides:
    the independent NumPy restatement gives the same codes from those entries (scores to 4e-6 relative: NumPy's log / exp are another
    arithmetic), and the indices equal torch.topk's wherever a rank is not a tie (O.clear_top3; ``tie_rows`` must hold some)."""
    lg = [t.to(DEV).contiguous() for t in lg_cpu]
    codes, scores, tp, ti = _select(lg)
    h_codes, h_scores, h_tp, h_ti = _select_host(lg_cpu)
    np.testing.assert_array_equal(codes, h_codes, err_msg=str(what))
    np.testing.assert_array_equal(scores.view(np.int32), h_scores.view(np.int32), err_msg=str(what))
    np.testing.assert_array_equal(tp.view(np.int32), h_tp.view(np.int32), err_msg=str(what))
    np.testing.assert_array_equal(ti, h_ti, err_msg=str(what))
    n_codes, n_scores = O.select_host(tp, ti)
    np.testing.assert_array_equal(codes, n_codes)
    assert (np.abs(scores - n_scores) <= 4e-6 * np.maximum(n_scores, 1e-30)).all(), (what, np.abs(scores - n_scores).max())
    rtp, rti = O.top3(lg_cpu)
    assert np.abs(tp - rtp.numpy()).max() <= 1e-6
    clear = O.clear_top3(lg_cpu).numpy()
    for i in tie_rows:
        assert not clear[i].all()
    np.testing.assert_array_equal(ti[clear], rti.numpy()[clear], err_msg=str(what))
    return codes, scores, tp, ti, rti.numpy()


def test_select_kernel_on_fixture_logits(g15):
    g = g15
    for r in g["logit_rows"]:
        for k in g["logit_passes"]:
            l32, _ = TF.stored_logits(g, int(r), int(k))
            codes, scores, tp, ti, rti = _check_select_against_host([torch.from_numpy(a) for a in l32], (int(r), int(k)))
            np.testing.assert_array_equal(codes, g["codes"][r, k][g["logit_pos"]])
            assert np.abs(scores - g["scores32"][r, k][g["logit_pos"]]).max() <= 10 * g["d_p"][r]
            c2, s2, _, _ = _select([torch.from_numpy(a).to(DEV) for a in l32], top=False)
            np.testing.assert_array_equal(c2, codes)
            np.testing.assert_array_equal(s2.view(np.int32), scores.view(np.int32))


def test_select_kernel_synthetic_ties_invalid_and_pitch():
    """Exact ties (first-index rule in the three largest entries and among the 27 choices), positions whose 27 code points are all
    invalid (choice 0, score 0), rows across wave and workgroup edges, padded rows whose pad must never be read."""
    n = 11
    lg = [torch.full((n, m), -30.0) for m in MOD]
    for h, m in enumerate(MOD):
        lg[h][0, [65 % m, 66 % m, 67 % m]] = 5.0                        # three equal maxima per head: ranks by index, choice (0,0,0) on the tie
        for j, big in enumerate((0x40000 + 1000, 0x50000 + 77, 0x60000 + 5)):
            lg[h][1, big % m] = 6.0 - j                                  # all 27 invalid
        lg[h][2, :] = 0.0                                                # uniform row: indices 0, 1, 2; code point 0 wins
        lg[h][3, 0x3FFFF % m] = 9.0; lg[h][3, 0x40000 % m] = 9.5        # best choice invalid, the valid limit itself second
        lg[h][4, m - 1] = 4.0; lg[h][4, m - 2] = 4.0                    # the row's last indices (lane 2 / 4 / 8 of the last chunk)
    gen = torch.Generator().manual_seed(11)
    for i in range(5, n):
        for h, m in enumerate(MOD):
            lg[h][i] = torch.randn(m, generator=gen) * 3
            lg[h][i, (0x3041 + 7 * i) % m] = 14.0
    # rows 0, 2 and 4 hold equal values among a head's largest entries: the kernel's rule there is the lowest index (checked below and, bit for
    # bit, against the host restatement); torch.topk's order among equals is not defined, so its indices are compared on the other rows
    codes, scores, tp, ti, rti = _check_select_against_host(lg, "synthetic", tie_rows=(0, 2, 4))
    for h, m in enumerate(MOD):
        assert list(ti[0, h]) == [65, 66, 67] and list(ti[2, h]) == [0, 1, 2] and list(ti[4, h]) == [m - 2, m - 1, 0]
        assert sorted(ti[0, h]) == sorted(rti[0, h]) and sorted(ti[4, h][:2]) == sorted(rti[4, h][:2])
    assert codes[0] == 65 and scores[0] > 0.3
    assert codes[1] == 0x40000 + 1000 and scores[1] == 0.0
    assert codes[2] == 0 and codes[3] == 0x3FFFF
    for i in range(5, n):
        assert codes[i] == 0x3041 + 7 * i and scores[i] > 0.9
    padded = []
    for h, m in enumerate(MOD):
        p = torch.full((n, m + 37), 1e4)
        p[:, :m] = lg[h]
        padded.append(p.to(DEV))
    c2, s2, _, _ = _select(padded, lds=[m + 37 for m in MOD])
    np.testing.assert_array_equal(c2, codes)
    np.testing.assert_array_equal(s2.view(np.int32), scores.view(np.int32))


def test_row_update_rules_including_the_no_remask_exit():
    """The loop's per-row decisions against the restatement: early stop, the no-remask stop (all 400 positions above 0.9 -- not reached by
    the free-running fixture), a running row, the last pass, a row that is already done."""
    Bn = 5
    gen = torch.Generator().manual_seed(3)
    tokens = torch.full((Bn, 400), 3, dtype=torch.int64)
    tokens[:, ::3] = 0x3042
    codes = torch.randint(1, 0x3FFFF, (Bn, 400), generator=gen)
    scores = torch.rand(Bn, 400, generator=gen) * 0.5 + 0.4
    scores[0] = 0.995                                                    # early stop
    scores[1] = 0.95; scores[1, 0] = 0.9005; tokens[1, 0] = 3            # masked positions not above 0.99, nothing to re-mask: no-remask stop
    codes[2, 7] = 0x40000 + 3; scores[2, 7] = 0.0                       # running row with an invalid code
    scores[3] = 0.995; codes[3, 5] = 0; scores[3, 5] = 0.1; tokens[3, 5] = 3     # code 0 is not tested by the early stop
    done0 = torch.tensor([0, 0, 0, 0, 1], dtype=torch.int32)
    for k in (0, 7):
        dt, dc, ds = tokens.to(DEV), codes.to(DEV), scores.to(DEV)
        done, active = done0.to(DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
        ids = torch.full((Bn, 400), -5, dtype=torch.int64, device=DEV)
        probs = torch.full((Bn, 400), -5.0, device=DEV)
        tr = [torch.full((8, Bn, 400), -1, dtype=torch.int64, device=DEV), torch.full((8, Bn, 400), -1, dtype=torch.int64, device=DEV),
              torch.full((8, Bn, 400), -1.0, device=DEV)]
        rc = L.load().ftc_text_row_update(dt.data_ptr(), dc.data_ptr(), ds.data_ptr(), Bn, k, done.data_ptr(), active.data_ptr(), ids.data_ptr(),
                                          probs.data_ptr(), tr[0].data_ptr(), tr[1].data_ptr(), tr[2].data_ptr(), stream())
        assert rc == 0, L.load().ftc_last_error()
        stopped, nxt = O.rows_update_host(k, tokens.numpy(), codes.numpy(), scores.numpy())
        stopped[4] = True
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), stopped)
        if k == 0:
            assert list(stopped) == [True, True, False, True, True]
        assert int(active[k]) == int((~stopped).sum())
        for b in range(Bn):
            if b == 4:
                assert (ids[b] == -5).all() and (tr[0][k, b] == -1).all() and torch.equal(dt[b].cpu(), tokens[b])
                continue
            assert torch.equal(tr[0][k, b].cpu(), tokens[b]) and torch.equal(tr[1][k, b].cpu(), codes[b]) and torch.equal(tr[2][k, b].cpu(), scores[b])
            if stopped[b]:
                assert torch.equal(ids[b].cpu(), codes[b]) and torch.equal(probs[b].cpu(), scores[b]) and torch.equal(dt[b].cpu(), tokens[b])
            else:
                np.testing.assert_array_equal(dt[b].cpu().numpy(), nxt[b])
                assert (ids[b] == -5).all()


# ---- 2. teacher-forced ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16x3", "bf16", "fp16"])
def test_teacher_forced_logits_and_encoder_vs_float64(g15, precision):
    g = g15
    for r in (int(v) for v in g["logit_rows"]):
        model, _ = model_for(precision, float(g["gains"][r]))
        x = torch.from_numpy(TF.row_input(g, r))[None].to(DEV)
        ks = [int(k) for k in g["logit_passes"]]
        with torch.no_grad():
            enc, outs = teacher_forced(model._engine, x, TF.tokens_of(g, r, ks[0])[None], [TF.tokens_of(g, r, k)[None] for k in ks[1:]])
            first = model(x, TF.tokens_of(g, r, ks[0])[None].to(DEV))                      # Transformer.forward: the same pass
        for h in range(3):
            assert torch.equal(first[h], outs[0][h])
        worst = 0.0
        for k, lg in zip(ks, outs):
            _, l64 = TF.stored_logits(g, r, k)
            for h in range(3):
                got = lg[h][0].cpu().numpy()[g["logit_pos"]].astype(np.float64)
                err = float(np.abs(got - l64[h]).max())
                rng = float(l64[h].max() - l64[h].min())
                bound = {"fp32": 8 * g["d_logit"][r], "fp16x3": 1e-3 * rng, "bf16": 2 * g["bf16_logit_dev"][r], "fp16": 2 * g["bf16_logit_dev"][r]}[precision]
                worst = max(worst, err / bound)
                log(f"{precision} row {r} pass {k} head {h}: logit error {err:.3e}, bound {bound:.3e} (d_logit {g['d_logit'][r]:.2e}, range {rng:.1f})")
                assert err <= bound
        if r == int(g["enc_row"]):
            e64 = g["enc32"].astype(np.float64) + g["enc64_minus32"]
            err = float(np.abs(enc[0].cpu().numpy()[g["enc_pos"]] - e64).max())
            rng = float(e64.max() - e64.min())
            bound = {"fp32": 8 * g["d_enc"], "fp16x3": 1e-3 * rng, "bf16": 2 * g["bf16_enc_dev"][r], "fp16": 2 * g["bf16_enc_dev"][r]}[precision]
            log(f"{precision} encoder output row {r}: error {err:.3e}, bound {bound:.3e} (d_enc {g['d_enc']:.2e})")
            assert err <= bound


# ---- 3. free-running --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_predict_follows_the_fixture_path(g15, precision):
    """Every pass's tokens and codes and the final codes equal the fixture's at all positions; scores within 10 x d_p."""
    g = g15
    for r in range(len(g["lengths"])):
        _, model2 = model_for(precision, float(g["gains"][r]))
        x = torch.from_numpy(TF.row_input(g, r))[None].to(DEV)
        ids, probs, tr, passes = predict_device(model2._engine, x, trace=True)
        n = int(g["passes"][r])
        tok, cod, sc = (t.cpu().numpy()[:, 0] for t in tr)
        for k in range(8):
            if k < n:
                bad = np.flatnonzero(tok[k] != g["tokens"][r, k])
                assert bad.size == 0, f"{precision} row {r} pass {k}: tokens differ at {bad[:8]} (margins m_thr {g['m_thr'][r, max(k - 1, 0)]:.2e})"
                bad = np.flatnonzero(cod[k] != g["codes"][r, k])
                assert bad.size == 0, f"{precision} row {r} pass {k}: codes differ at {bad[:8]} (m_gap {g['m_gap'][r, k]:.2e})"
                err = float(np.abs(sc[k] - g["scores32"][r, k]).max())
                log(f"{precision} row {r} pass {k}: score error {err:.2e} (10 x d_p = {10 * g['d_p'][r]:.2e})")
                assert err <= 10 * g["d_p"][r]
            else:
                assert (tok[k] == -1).all()                 # the row had stopped: nothing more is recorded for it
        assert passes == n
        np.testing.assert_array_equal(ids[0].cpu().numpy(), g["codes"][r, n - 1])
        assert np.abs(probs[0].cpu().numpy() - g["scores32"][r, n - 1]).max() <= 10 * g["d_p"][r]
        with torch.no_grad():
            pred = model2(x).squeeze(0).cpu().numpy()       # the reference's call
        assert pred.dtype == np.int64 and pred.shape == (400,)
        np.testing.assert_array_equal(pred, g["codes"][r, n - 1])
        ids2, probs2, _, passes2 = predict_device(model2._engine, x, readback=False)       # all eight passes, stopped rows frozen on the device
        assert passes2 == 8 and torch.equal(ids2, ids) and torch.equal(probs2, probs)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_sixteen_bit_first_pass_codes(g15, precision):
    """A 16-bit run cannot follow the path: pass 0 only (all tokens masked).  The share of positions whose code differs from the fixture's
    is at most twice the share by which the reference's own bfloat16-autocast run differs from its float64 run, and at most 10 %."""
    g = g15
    differ = total = 0
    for r in range(len(g["lengths"])):
        _, model2 = model_for(precision, float(g["gains"][r]))
        x = torch.from_numpy(TF.row_input(g, r))[None].to(DEV)
        _, _, tr, _ = predict_device(model2._engine, x, trace=True)
        differ += int((tr[1][0, 0].cpu().numpy() != g["codes"][r, 0]).sum())
        total += 400
    ref_share = float(g["bf16_code_share"].mean())
    log(f"{precision} pass 0: {differ} of {total} codes differ ({differ / total:.4f}); the reference's bf16 autocast: {ref_share:.4f}")
    assert differ / total <= min(2 * ref_share, 0.10)


# ---- 4. batch independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16x3", "bf16", "fp16"])
def test_rows_of_a_batch_are_bitwise_the_rows_alone(g15, precision):
    g = g15
    gain = float(g["gains"][0])
    _, model2 = model_for(precision, gain)
    X = TF.padded_inputs(g)
    alone = {}
    for r in range(4):
        ids, probs, _, _ = predict_device(model2._engine, torch.from_numpy(X[r:r + 1]).to(DEV))
        alone[r] = (ids[0].cpu().numpy(), probs[0].cpu().numpy().view(np.int32))
    assert len({int(a[0].sum()) for a in alone.values()}) > 1
    for order in ([0], [1, 0], [3, 2], [0, 1, 2, 3, 3, 2, 1, 0], [2, 2, 0, 1, 3, 0, 1, 3]):
        ids, probs, _, _ = predict_device(model2._engine, torch.from_numpy(X[order]).to(DEV))
        for i, r in enumerate(order):
            np.testing.assert_array_equal(ids[i].cpu().numpy(), alone[r][0], err_msg=f"{precision} order {order} slot {i}")
            np.testing.assert_array_equal(probs[i].cpu().numpy().view(np.int32), alone[r][1], err_msg=f"{precision} order {order} slot {i}")
    short = torch.from_numpy(X[0:1, :37]).to(DEV)          # L < 400: the padding inside the library is the caller's zero padding
    ids, _, _, _ = predict_device(model2._engine, short)
    np.testing.assert_array_equal(ids[0].cpu().numpy(), alone[0][0])


# ---- 5. backend -------------------------------------------------------------------------------------------------------------------------
def test_backend_call_transformer_and_chunks(g15):
    g = g15
    r = 0
    _, model2 = model_for("fp32", float(g["gains"][r]))
    backend = HipTextBackend(model2)
    x = TF.row_input(g, r)
    n = len(x)
    encoder_input = np.zeros(shape=(1, max(100, n), 106), dtype=np.float32)        # process_ocr_base.py:230-233 pads a chunk to at least 100 rows
    encoder_input[0, :n] = x
    pred = backend.call_transformer(encoder_input)
    assert pred.dtype == np.int64 and pred.shape == (400,)
    np.testing.assert_array_equal(pred, g["codes"][r, g["passes"][r] - 1])
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    pred2 = backend.call_transformer(encoder_input)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before, "the second call allocated device memory"
    np.testing.assert_array_equal(pred2, pred)
    outs = recognize_chunks(model2, [x, x[:20], encoder_input])
    np.testing.assert_array_equal(outs[0], pred)
    np.testing.assert_array_equal(outs[2], pred)
    np.testing.assert_array_equal(outs[1], backend.call_transformer(x[None, :20]))
    with pytest.raises(ValueError, match="all zeros"):
        backend.call_transformer(np.zeros((1, 100, 106), dtype=np.float32))
    with pytest.raises(ValueError, match="all zeros"):
        model2(torch.zeros(2, 10, 106, device=DEV))
