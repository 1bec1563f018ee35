"""-m gpu: TextGrad(model, linear="hip") -- every linear layer of the recognizer's training forward and backward on the project's own kernels
(include/ftc_text_linear.h) -- against tests/golden/g21_text_grad.npz with the gates of tests/test_gpu_text_grad.py: every stored gradient entry
within 1e-3 of the parameter's largest reference entry (for a ``.bias`` also that of its sibling ``.weight``) + 1e-7; every parameter's L2 norm within
1e-3 relative + 1e-7 sqrt(numel); the loss within 2e-4 relative; the logits by the entry gate.  With every product in a fixed order, two calls leave
the same bits in EVERY ``.grad``, and the logits of a batch row do not depend on the rows it is batched with."""
import numpy as np
import pytest
import torch

import text_grad_fixture as TG
from findtextcenternet_amd import Transformer
from findtextcenternet_amd.text_grad import TextGrad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def g21():
    return TG.load()


@pytest.fixture(scope="module")
def model():
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    return m


@pytest.fixture(scope="module")
def run(model):
    tg = TextGrad(model, device=DEV, linear="hip")
    enc, dec, label = (torch.from_numpy(x).to(DEV) for x in TG.make_inputs())
    res = tg.forward_backward(enc, dec, label)
    torch.cuda.synchronize()
    return tg, (enc, dec, label), res, {n: (None if g is None else g.clone()) for n, g in tg.grads().items()}


def test_loss_counts_and_logits(g21, run):
    tg, (enc, dec, _), res, _ = run
    assert set(res) == {"loss", "correct", "total"}
    assert abs(float(res["loss"]) - float(g21["loss"])) < 2e-4 * abs(float(g21["loss"]))
    assert int(res["total"]) == int(g21["total"]) and int(res["correct"]) == int(g21["correct"])
    with torch.no_grad():
        lg = tg.logits(enc, dec)
    pos = torch.tensor(TG.LOGIT_POS, device=DEV)
    for h in range(3):
        ref = g21[f"logits{h}"]
        err = np.abs(lg[h][:, pos].double().cpu().numpy() - ref).max()
        print(f"[text grad, hip linear] logits {h}: max error {err:.2e} of range {np.abs(ref).max():.2f}")
        assert err <= 1e-3 * np.abs(ref).max() + 1e-7


def test_every_parameter_gradient(g21, run):
    tg, _, _, grads = run
    names = [str(n) for n in g21["grad_names"]]
    assert names == list(tg.params)
    amax = dict(zip(names, g21["grad_absmax"]))
    none = {str(n) for n in g21["grad_none"]}
    bad, worst = [], (0.0, "")
    for i, n in enumerate(names):
        g = grads[n]
        if n in none:
            assert g is None or float(g.abs().max()) == 0.0, n
            continue
        assert g is not None and g.shape == tg.params[n].shape, n
        mine = g.double().cpu().numpy().reshape(-1)
        norm, ref = float(g21["grad_norms"][i]), g21["grad_picks"][i]
        if abs(float(np.linalg.norm(mine)) - norm) > 1e-3 * norm + 1e-7 * np.sqrt(mine.size):
            bad.append((n, "norm", float(np.linalg.norm(mine)), norm))
        scale = float(amax[n])
        if n.endswith(".bias") and n[:-4] + "weight" in amax:
            scale = max(scale, float(amax[n[:-4] + "weight"]))
        err = float(np.abs(mine[g21["grad_pick_index"][i]] - ref).max())
        if err > 1e-3 * scale + 1e-7:
            bad.append((n, "entries", err, scale))
        worst = max(worst, (err / max(scale, 1e-30), n))
    print(f"[text grad, hip linear] {len(names)} parameters, worst entry error / largest entry {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad[:8]


def test_two_calls_leave_the_same_bits_everywhere(g21, run):
    tg, (enc, dec, label), res, grads = run
    again = tg.forward_backward(enc, dec, label)
    torch.cuda.synchronize()
    assert torch.equal(again["loss"], res["loss"])
    none = {str(n) for n in g21["grad_none"]}          # the self-attentions' unused pos_emb_k tables
    for n, g in tg.grads().items():
        if n in none and grads[n] is None:
            assert g is None, n
        else:
            assert g is not None and torch.equal(g, grads[n]), n


def test_grad_scale_is_exact(run):
    tg, (enc, dec, label), _, grads = run
    tg.forward_backward(enc, dec, label, grad_scale=65536.0)
    torch.cuda.synchronize()
    for n, g in tg.grads().items():
        if grads[n] is None:
            assert g is None
        else:
            assert torch.equal(g, grads[n] * 65536.0), n


def test_logits_of_a_row_do_not_depend_on_the_batch(run):
    tg, (enc, dec, _), _, _ = run
    with torch.no_grad():
        both = tg.logits(enc, dec)
        alone = tg.logits(enc[:1], dec[:1])
    for h in range(3):
        assert alone[h].shape[0] == 1 and torch.equal(alone[h][0], both[h][0]), h


def test_linear_argument(model):
    with pytest.raises(ValueError):
        TextGrad(model, device=DEV, linear="rocblas")
    assert TextGrad(model, device=DEV).linear == "torch" and TextGrad(model, device=DEV, linear="hip").linear == "hip"


def test_default_is_still_torch(model):
    enc, dec, label = (torch.from_numpy(x).to(DEV) for x in TG.make_inputs())
    a, b = TextGrad(model, device=DEV), TextGrad(model, device=DEV, linear="torch")
    import torch.nn.functional as F
    assert a.linear == b.linear == "torch" and a._lin is F.linear and b._lin is F.linear          # the same function on the same parameters
    for n in a.params:
        assert torch.equal(a.params[n], b.params[n])
    with torch.no_grad():
        for x, y in zip(a.logits(enc, dec), b.logits(enc, dec)):          # (torch's own GEMM promises no fixed order: close, not bits)
            assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())
