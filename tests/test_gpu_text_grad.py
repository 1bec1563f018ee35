"""-m gpu: TextGrad.forward_backward -- the recognizer's loss and every parameter gradient on the GPU -- against tests/golden/g21_text_grad.npz, which the
reference's own Transformer, loss_function3 and ``loss.backward()`` wrote in float64 on the CPU.

Gate, the one tests/test_gpu_train_step.py applies to g10_train_step.npz: every stored gradient entry within 1e-3 of the parameter's largest reference
entry (for a ``.bias`` also that of its sibling ``.weight``) + 1e-7 absolute; every parameter's L2 norm within 1e-3 relative + 1e-7 sqrt(numel); the
loss within 2e-4 relative; the logits by the entry gate."""
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
def run(g21):
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    tg = TextGrad(m, device=DEV)
    enc, dec, label = (torch.from_numpy(x).to(DEV) for x in TG.make_inputs())
    res = tg.forward_backward(enc, dec, label)
    torch.cuda.synchronize()
    return m, tg, (enc, dec, label), res, {n: (None if g is None else g.clone()) for n, g in tg.grads().items()}


def test_loss_counts_and_logits(g21, run):
    _, tg, (enc, dec, _), res, _ = run
    assert set(res) == {"loss", "correct", "total"}
    assert abs(float(res["loss"]) - float(g21["loss"])) < 2e-4 * abs(float(g21["loss"]))
    assert int(res["total"]) == int(g21["total"]) and int(res["correct"]) == int(g21["correct"])
    with torch.no_grad():
        lg = tg.logits(enc, dec)
    pos = torch.tensor(TG.LOGIT_POS, device=DEV)
    for h in range(3):
        ref = g21[f"logits{h}"]
        err = np.abs(lg[h][:, pos].double().cpu().numpy() - ref).max()
        print(f"[text grad] logits {h}: max error {err:.2e} of range {np.abs(ref).max():.2f}")
        assert err <= 1e-3 * np.abs(ref).max() + 1e-7


def test_every_parameter_gradient(g21, run):
    _, tg, _, _, grads = run
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
    print(f"[text grad] {len(names)} parameters, worst entry error / largest entry {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad[:8]


def test_grad_scale_is_exact(run):
    _, tg, (enc, dec, label), _, grads = run
    tg.forward_backward(enc, dec, label, grad_scale=65536.0)
    torch.cuda.synchronize()
    for n, g in tg.grads().items():
        if grads[n] is None:
            assert g is None
        else:
            assert torch.equal(g, grads[n] * 65536.0), n


def test_module_round_trip_and_forward(run):
    m, tg, (enc, dec, _), _, _ = run
    with torch.no_grad():
        lg = tg.logits(enc, dec)
        ref = m.to(DEV)(enc, dec)
    for a, b in zip(lg, ref):
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())
    n = "decoder.norm.bias"
    with torch.no_grad():
        tg.params[n].add_(1.0)
    tg.store_to_module()
    assert torch.equal(dict(m.named_parameters())[n].detach().cpu(), tg.params[n].detach().cpu())
    m.load_state_dict(TG.state_dict())
    tg.load_from_module()
    assert torch.equal(tg.params[n].detach().cpu(), TG.state_dict()[n])


def test_loss_function3_on_the_reference_case(g21):
    """The raw-logit case of the fixture through loss_function3: the reference's own function gave these numbers."""
    from findtextcenternet_amd.loss_func import loss_function3
    lg, lab, msk = TG.loss3_inputs()
    outs = [torch.from_numpy(x).to(DEV).requires_grad_(True) for x in lg]
    res = loss_function3(outs, torch.from_numpy(lab).to(DEV), torch.from_numpy(msk).to(DEV))
    assert abs(float(res["loss"].detach()) - float(g21["l3_loss"])) < 2e-4 * float(g21["l3_loss"])
    assert int(res["correct"]) == int(g21["l3_correct"]) and int(res["total"]) == int(g21["l3_total"])
    res["loss"].backward()
    for h in range(3):
        ref = g21[f"l3_grad{h}"]
        assert np.abs(outs[h].grad.cpu().numpy() - ref).max() <= 1e-3 * np.abs(ref).max() + 1e-7
        assert not outs[h].grad.cpu().numpy()[~msk].any()
