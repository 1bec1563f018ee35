"""-m gpu: TextGrad(model, linear="hip_fp16", attention="hip_fp16") -- every linear layer AND all three attention sites of the recognizer's training
forward and backward on fp16 operands (include/ftc_text_linear_f16.h, include/ftc_text_attention_f16.h), run as the reference's AMP step runs:
forward_backward(..., grad_scale=65536.0), gradients divided by 65536 -- against tests/golden/g25_text_grad_f16_attn.npz (the reference's float64 step
with exactly those roundings, tests/golden/gen_golden_text_grad_f16_attn.py).

The gates are the fixture's (gate_loss, gate_logit, gate_grad), set by the generator from its own construction run in float32 on the CPU, never from the
kernel: g21's gate where that construction lies at most half of it from the fixture, twice its distance otherwise
(tests/test_attention_f16_operands_host.py asserts the rule).  Over every logit position and every gradient entry the float32 construction lies
    loss      4.8e-6 relative                      -> gate 2e-4, g21's
    logits    5.25e-4 of range                     -> gate 1.049e-3 of the largest reference logit + 1e-7 (g21's: 1e-3)
    entries   1.341e-3 of the largest entry, at decoder.blocks.0.cross_attn.pos_emb_q.encoding
                                                   -> gate 2.681e-3 of the largest reference entry (for a ``.bias`` also that of its sibling ``.weight``)
                                                      + 1e-7 (g21's: 1e-3)
from the fixture; every parameter's L2 norm stays within g21's 1e-3 relative + 1e-7 sqrt(numel) (float32 construction: 2.1e-4).  Why the entries' gate
is wider than g21's: a flipped rounding of P or dS moves one attention row by an fp16 ulp, and an entry of a ``pos_emb_q.encoding`` gradient is the sum
over the TWO batch rows of one position's gradient -- nothing dilutes the flip.  On the 16 stored entries per parameter alone the float32 construction
shows 2.0e-4 (it happens to miss the affected entries); measured on an MI355X, the kernels show 1.19e-3 on them, at that same parameter, logits 3.0e-4
of range, norms 2.5e-4.

Also: two calls leave the same bits in every ``.grad``; a batch row's logits are the bits of that row run alone; ``attention(..., operands="fp16")``
under autograd equals the C ABI call; grad_scale = 2^30 leaves non-finite gradients, ``torch.amp.GradScaler`` then skips ``RAdamScheduleFree``'s step and
a step at 65536 is taken; and with the defaults ``attention(q, k, v)`` and ``TextGrad(model)`` return the bits of ``ftc_text_attention`` /
``ftc_text_attention_bwd``: the new arguments changed nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_operands as S
import text_grad_fixture as TG
from findtextcenternet_amd import RAdamScheduleFree, Transformer
from findtextcenternet_amd import _lib as L
from findtextcenternet_amd import text_grad as G
from findtextcenternet_amd.text_grad import TextGrad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 65536.0
G25 = TG.PATH.replace("g21_text_grad.npz", "g25_text_grad_f16_attn.npz")


@pytest.fixture(scope="module")
def g25():
    g = np.load(G25)
    assert float(g["grad_scale"]) == SCALE
    return g


@pytest.fixture(scope="module")
def model():
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    return m


@pytest.fixture(scope="module")
def inputs():
    return tuple(torch.from_numpy(x).to(DEV) for x in TG.make_inputs())


@pytest.fixture(scope="module")
def run(model, inputs):
    tg = TextGrad(model, device=DEV, linear="hip_fp16", attention="hip_fp16")
    res = tg.forward_backward(*inputs, grad_scale=SCALE)
    torch.cuda.synchronize()
    return tg, res, {n: (None if g is None else g.clone()) for n, g in tg.grads().items()}


def test_loss_counts_and_logits(g25, run, inputs):
    tg, res, _ = run
    enc, dec, _ = inputs
    gate_loss, gate_logit = float(g25["gate_loss"]), float(g25["gate_logit"])
    assert gate_loss >= 2e-4 and gate_logit >= 1e-3          # never below g21's
    err = abs(float(res["loss"]) - float(g25["loss"])) / abs(float(g25["loss"]))
    print(f"[text grad, fp16 linear + attention] loss {float(res['loss']):.9f} against {float(g25['loss']):.9f} ({err:.2e} relative, gate {gate_loss:.1e})")
    assert err < gate_loss
    assert int(res["total"]) == int(g25["total"]) and int(res["correct"]) == int(g25["correct"])
    with torch.no_grad():
        lg = tg.logits(enc, dec)
    pos = torch.tensor(TG.LOGIT_POS, device=DEV)
    for h in range(3):
        ref = g25[f"logits{h}"]
        err = np.abs(lg[h][:, pos].double().cpu().numpy() - ref).max()
        print(f"[text grad, fp16 linear + attention] logits {h}: max error {err:.2e} of range {np.abs(ref).max():.2f} ({err / np.abs(ref).max():.2e}, gate {gate_logit:.1e})")
        assert err <= gate_logit * np.abs(ref).max() + 1e-7


def test_every_parameter_gradient(g25, run):
    tg, _, grads = run
    gate = float(g25["gate_grad"])
    assert gate >= 1e-3
    names = [str(n) for n in g25["grad_names"]]
    assert names == list(tg.params)
    amax = dict(zip(names, g25["grad_absmax"]))
    none = {str(n) for n in g25["grad_none"]}
    bad, worst, worst_norm = [], (0.0, ""), (0.0, "")
    for i, n in enumerate(names):
        g = grads[n]
        if n in none:
            assert g is None or float(g.abs().max()) == 0.0, n
            continue
        assert g is not None and g.shape == tg.params[n].shape and bool(torch.isfinite(g).all()), n
        mine = g.double().cpu().numpy().reshape(-1) / SCALE
        norm, ref = float(g25["grad_norms"][i]), g25["grad_picks"][i]
        nerr = abs(float(np.linalg.norm(mine)) - norm)
        if nerr > 1e-3 * norm + 1e-7 * np.sqrt(mine.size):
            bad.append((n, "norm", float(np.linalg.norm(mine)), norm))
        worst_norm = max(worst_norm, (nerr / max(norm, 1e-30), n))
        scale = float(amax[n])
        if n.endswith(".bias") and n[:-4] + "weight" in amax:
            scale = max(scale, float(amax[n[:-4] + "weight"]))
        err = float(np.abs(mine[g25["grad_pick_index"][i]] - ref).max())
        if err > gate * scale + 1e-7:
            bad.append((n, "entries", err, scale))
        worst = max(worst, (err / max(scale, 1e-30), n))
    print(f"[text grad, fp16 linear + attention] {len(names)} parameters, worst entry error / largest entry {worst[0]:.2e} ({worst[1]}), gate {gate:.1e}; "
          f"worst norm error {worst_norm[0]:.2e} relative ({worst_norm[1]})")
    assert not bad, bad[:8]


def test_two_calls_leave_the_same_bits_everywhere(g25, run, inputs):
    tg, res, grads = run
    again = tg.forward_backward(*inputs, grad_scale=SCALE)
    torch.cuda.synchronize()
    assert torch.equal(again["loss"], res["loss"])
    none = {str(n) for n in g25["grad_none"]}
    for n, g in tg.grads().items():
        if n in none and grads[n] is None:
            assert g is None, n
        else:
            assert g is not None and torch.equal(g, grads[n]), n


def test_logits_of_a_row_do_not_depend_on_the_batch(run, inputs):
    tg, _, _ = run
    enc, dec, _ = inputs
    with torch.no_grad():
        both = tg.logits(enc, dec)
        alone = tg.logits(enc[:1], dec[:1])
    for h in range(3):
        assert alone[h].shape[0] == 1 and torch.equal(alone[h][0], both[h][0]), h


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _abi(q, k, v, pad, dout, half):
    """(out, dq, dk, dv) of the C entry points on contiguous device tensors."""
    lib = L.load()
    sfx = "_f16" if half else ""
    B, Sq, E = q.shape
    Sk = k.shape[1]
    out, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    padp = pad.data_ptr() if pad is not None else None
    rc = getattr(lib, "ftc_text_attention" + sfx)(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, padp, out.data_ptr(), E, B, E // 64, Sq, Sk, _stream())
    assert rc == 0, lib.ftc_last_error()
    ws = torch.empty(int(getattr(lib, f"ftc_text_attention{sfx}_bwd_workspace_bytes")(B, E // 64, Sq, Sk)), dtype=torch.uint8, device=DEV)
    rc = getattr(lib, f"ftc_text_attention{sfx}_bwd")(q.data_ptr(), E, k.data_ptr(), E, v.data_ptr(), E, padp, dout.data_ptr(), E, dq.data_ptr(), E, dk.data_ptr(), E,
                                                      dv.data_ptr(), E, B, E // 64, Sq, Sk, ws.data_ptr(), _stream())
    assert rc == 0, lib.ftc_last_error()
    torch.cuda.synchronize()
    return out, dq, dk, dv


def _operands():
    g = torch.Generator().manual_seed(77)
    B, Sq, Sk, E = 2, 33, 41, 128
    q, k, v, dout = (torch.randn(B, n, E, generator=g).to(DEV) for n in (Sq, Sk, Sk, Sq))
    pad = (torch.rand(B, Sk, generator=g) < 0.3)
    pad[:, 0] = False
    return q, k, v, pad.to(torch.uint8).to(DEV), dout


@pytest.mark.parametrize("operands", ["fp16", "fp32", None])
def test_autograd_wrapper_is_the_c_abi_call(operands):
    """operands="fp16": the new entry points; "fp32" and the default (no argument): ftc_text_attention / ftc_text_attention_bwd, bit for bit."""
    q, k, v, pad, dout = _operands()
    want = _abi(q, k, v, pad, dout, operands == "fp16")
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = G.attention(*leaves, pad) if operands is None else G.attention(*leaves, pad, operands)
    out.backward(dout)
    torch.cuda.synchronize()
    for name, mine, ref in zip(("out", "dq", "dk", "dv"), (out.detach(), *(t.grad for t in leaves)), want):
        assert torch.equal(mine.view(torch.int32), ref.view(torch.int32)), (operands, name)
    if operands == "fp16":          # the mode is not a no-op on these operands
        plain = _abi(q, k, v, pad, dout, False)
        assert not torch.equal(plain[0], want[0])


def test_arguments(model):
    for kind in ("hip", "hip_fp16"):
        assert TextGrad(model, device=DEV, attention=kind).attention == kind
    with pytest.raises(ValueError):
        TextGrad(model, device=DEV, attention="torch")
    q, k, v, pad, _ = _operands()
    with pytest.raises(ValueError):
        G.attention(q, k, v, pad, "bf16")


def test_defaults_keep_their_bits(model, inputs):
    """TextGrad(model) and TextGrad(model, attention="hip") leave the same bits: the attention argument changed nothing; and attention="hip_fp16" does
    change them (the argument reaches the three attention sites)."""
    runs = {}
    for key, kw in (("default", {}), ("hip", dict(attention="hip")), ("f16", dict(attention="hip_fp16"))):
        tg = TextGrad(model, device=DEV, linear="hip", **kw)
        res = tg.forward_backward(*inputs)
        torch.cuda.synchronize()
        runs[key] = (res["loss"].clone(), {n: None if g is None else g.clone() for n, g in tg.grads().items()})
    assert torch.equal(runs["default"][0], runs["hip"][0])
    for n, g in runs["default"][1].items():
        assert (g is None and runs["hip"][1][n] is None) or torch.equal(g, runs["hip"][1][n]), n
    assert any(g is not None and not torch.equal(g, runs["f16"][1][n]) for n, g in runs["default"][1].items())


def test_a_scale_of_two_to_the_thirty_overflows(model, inputs):
    tg = TextGrad(model, device=DEV, linear="hip_fp16", attention="hip_fp16")
    res = tg.forward_backward(*inputs, grad_scale=2.0 ** 30)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res["loss"]))          # the forward does not see the scale
    for j in range(3):
        for part in ("weight", "bias"):
            g = tg.params[f"decoder.out_layers.{j}.{part}"].grad
            assert g is not None and not bool(torch.isfinite(g).all()), (j, part)
    g = tg.params["decoder.blocks.0.cross_attn.q_proj.weight"].grad          # behind an attention backward
    assert g is not None and not bool(torch.isfinite(g).all())


def _scaler(init_scale):
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    scaler.scale(torch.zeros(1, device="cuda"))                          # the scale tensor is made by the first scale(loss) of a loop
    return scaler


def _state(tg, opt):
    out = {}
    for n, p in tg.params.items():
        out[n] = p.detach().cpu().numpy().copy()
        for k in ("z", "exp_avg_sq"):
            if k in opt.state.get(p, {}):
                out[n, k] = opt.state[p][k].detach().cpu().numpy().copy()
    return out


def test_gradscaler_skips_the_overflowed_step_and_takes_the_next(model, inputs):
    tg = TextGrad(model, device=DEV, linear="hip_fp16", attention="hip_fp16")
    opt = RAdamScheduleFree(tg.parameters(), lr=2e-4)
    opt.train()
    books = lambda: [g["k"] for g in opt.param_groups]          # noqa: E731
    clean, big = _scaler(SCALE), _scaler(2.0 ** 30)
    tg.forward_backward(*inputs, grad_scale=clean.get_scale())
    clean.step(opt)
    clean.update()
    torch.cuda.synchronize()
    assert books() == [1] * len(opt.param_groups) and clean.get_scale() == SCALE
    before = _state(tg, opt)
    # the step at 2^30 is skipped: nothing is written, the count stands, the scale halves
    tg.forward_backward(*inputs, grad_scale=big.get_scale())
    big.step(opt)
    big.update()
    torch.cuda.synchronize()
    after = _state(tg, opt)
    assert set(after) == set(before)
    for k, b in before.items():
        S.assert_bytes(after[k], b, f"a skipped step wrote {k}")
    assert books() == [1] * len(opt.param_groups) and big.get_scale() == 2.0 ** 29
    # a following step at 65536 is taken
    tg.forward_backward(*inputs, grad_scale=clean.get_scale())
    clean.step(opt)
    clean.update()
    torch.cuda.synchronize()
    assert books() == [2] * len(opt.param_groups) and clean.get_scale() == SCALE
    moved = _state(tg, opt)
    assert any(not np.array_equal(moved[k], before[k]) for k in before)
    assert all(np.isfinite(v).all() for v in moved.values())
