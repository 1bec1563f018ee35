"""CPU: tests/golden/g21_text_grad.npz (the reference's Transformer + loss_function3 + backward in float64, written by tests/golden/gen_golden_text_grad.py)
is consistent with itself and with what tests/test_gpu_text_grad.py regenerates: inputs, parameter names, stored indices, norms against entries, the
parameters without a gradient, and the raw-logit loss case against torch's float64 cross entropy.  Also what findtextcenternet_amd.text_grad refuses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import text_grad_fixture as TG
from findtextcenternet_amd import Transformer
from findtextcenternet_amd.schema import transformer_schema


@pytest.fixture(scope="module")
def g21():
    return TG.load()


def test_fixture_inputs_and_names(g21):
    enc, dec, label = TG.make_inputs()
    assert np.array_equal(g21["enc_input"].astype(np.float32), enc) and np.array_equal(g21["dec_input"], dec) and np.array_equal(g21["label_code"], label)
    assert int(g21["weight_seed"]) == TG.SEED_W and float(g21["gain"]) == TG.GAIN and tuple(g21["lengths"]) == TG.LENGTHS
    for b, n in enumerate(TG.LENGTHS):
        assert (enc[b, :n] != 0).any(-1).all() and not enc[b, n:].any()
        assert ((dec[b, :n] == TG.MSK) | (dec[b, :n] == label[b, :n])).all() and not dec[b, n:].any()
    assert int(g21["total"]) == int((dec == TG.MSK).sum()) > 8 and 0 <= int(g21["correct"]) <= int(g21["total"])
    names = [str(n) for n in g21["grad_names"]]
    assert names == list(transformer_schema(TG.DIMS)) == list(TG.state_dict())
    assert np.isfinite(float(g21["loss"])) and float(g21["loss"]) > 0
    for h, m in enumerate((1091, 1093, 1097)):
        assert g21[f"logits{h}"].shape == (2, len(TG.LOGIT_POS), m) and g21[f"logits{h}"].dtype == np.float64


def test_fixture_gradients_are_consistent(g21):
    sch = transformer_schema(TG.DIMS)
    none = {str(n) for n in g21["grad_none"]}
    assert none == {n for n in sch if n.endswith("pos_emb_k.encoding") and ("self_attn" in n or ".mha." in n)}
    for i, n in enumerate(g21["grad_names"]):
        n = str(n)
        numel = int(np.prod(sch[n][0]))
        assert np.array_equal(g21["grad_pick_index"][i], TG.pick_index(n, numel))
        picks, amax, norm = g21["grad_picks"][i], float(g21["grad_absmax"][i]), float(g21["grad_norms"][i])
        assert np.abs(picks).max() <= amax <= norm * (1 + 1e-12) and norm <= amax * np.sqrt(numel) * (1 + 1e-12)
        _, first = np.unique(g21["grad_pick_index"][i], return_index=True)
        assert np.sqrt((picks[first] ** 2).sum()) <= norm * (1 + 1e-12)
        assert (amax == 0) == (n in none)


def test_fixture_loss_case_is_the_plain_formula(g21):
    """loss_function3 on the stored raw logits, restated with torch's float64 cross entropy: the reference's numbers come out."""
    lg, lab, msk = TG.loss3_inputs()
    assert all(np.array_equal(lg[h], g21[f"l3_logits{h}"]) for h in range(3)) and np.array_equal(lab, g21["l3_labels"]) and np.array_equal(msk, g21["l3_mask"])
    mask = torch.from_numpy(msk)
    loss, hit = 0.0, torch.ones_like(mask)
    outs = [torch.from_numpy(x).double().requires_grad_(True) for x in lg]
    for o, m in zip(outs, (1091, 1093, 1097)):
        target = torch.from_numpy(np.mod(lab, m))                      # floor-modulus
        assert int(target.min()) >= 0
        loss = loss + F.cross_entropy(o.permute(0, 2, 1), target, reduction="none")[mask].mean()
        hit &= torch.argmax(o, -1) == target
    assert abs(float(loss.detach()) - float(g21["l3_loss"])) <= 1e-12 * float(g21["l3_loss"])
    assert int(g21["l3_total"]) == int(mask.sum()) == 6 and int(g21["l3_correct"]) == int((hit & mask).sum()) == 2
    loss.backward()
    for h in range(3):
        assert np.abs(outs[h].grad.numpy() - g21[f"l3_grad{h}"]).max() <= 1e-7
        assert not g21[f"l3_grad{h}"][~msk].any()


def test_text_grad_refuses_what_it_does_not_do():
    from findtextcenternet_amd import text_grad as G
    from findtextcenternet_amd.loss_func import loss_function3
    assert loss_function3 is G.loss_function3
    d = dict(TG.DIMS.__dict__, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        G.TextGrad(Transformer(**d))
    with pytest.raises(TypeError):
        G.TextGrad(torch.nn.Linear(2, 2))
    x = torch.zeros(1, 4, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        G.attention(x, x, x)
    with pytest.raises(RuntimeError, match="GPU only"):
        G.swiglu(torch.zeros(2, 16))
    with pytest.raises(ValueError):
        G.rownorm(a=None, tokens=None)
    with pytest.raises(ValueError):
        G.loss_function3([x, x, x], torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.bool))
