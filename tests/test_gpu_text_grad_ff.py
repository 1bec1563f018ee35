"""-m gpu: TextGrad(ff="fused") -- the SwiGLU feed-forward block as one autograd node on the residual forms of the linear kernels -- against
TextGrad() with ``ff`` left at its default, on the SMALL recognizer (E 128, 2 heads, 2 + 2 blocks) and ``text_grad_fixture.make_inputs()`` ([2, 400,
106]), for ``linear="hip"`` and for ``linear="hip_fp16", attention="hip_fp16"``.  Every sum is the one the default makes -- the wide product is the
same launch on the same operands, ``(sum + bias) + x`` and ``dx + dy`` are two-term fp32 additions -- so the gate is equality of bits: loss and
counts, the logits, every ``.grad`` (and ``None`` where it is ``None`` today).  Also: w1.weight and wg.weight of a block are slices of one storage,
16-byte aligned and contiguous; names and order of ``parameters()`` are the default's; store_to_module / load_from_module round-trips; ff="fused"
needs the HIP linear layers."""
import pytest
import torch

import text_grad_fixture as TG
from findtextcenternet_amd import Transformer
from findtextcenternet_amd.text_grad import TextGrad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 65536.0
MODES = {"hip": dict(linear="hip"), "hip_fp16": dict(linear="hip_fp16", attention="hip_fp16")}


@pytest.fixture(scope="module")
def model():
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    return m


@pytest.fixture(scope="module")
def inputs():
    return tuple(torch.from_numpy(x).to(DEV) for x in TG.make_inputs())


def _run(tg, inputs, scale):
    res = tg.forward_backward(*inputs, grad_scale=scale)
    with torch.no_grad():
        logits = [t.clone() for t in tg.logits(inputs[0], inputs[1])]
    torch.cuda.synchronize()
    return res, logits, {n: (None if g is None else g.clone()) for n, g in tg.grads().items()}


@pytest.mark.parametrize("mode", list(MODES))
def test_fused_is_the_default_bit_for_bit(model, inputs, mode):
    scale = SCALE if mode == "hip_fp16" else 1.0
    plain, fused = TextGrad(model, device=DEV, **MODES[mode]), TextGrad(model, device=DEV, ff="fused", **MODES[mode])
    assert plain.ff == "torch" and fused.ff == "fused"
    (res_p, log_p, grad_p), (res_f, log_f, grad_f) = _run(plain, inputs, scale), _run(fused, inputs, scale)
    assert torch.equal(res_p["loss"], res_f["loss"]) and bool(torch.isfinite(res_f["loss"]))
    assert int(res_p["correct"]) == int(res_f["correct"]) and int(res_p["total"]) == int(res_f["total"]) > 0
    for h in range(3):
        assert torch.equal(log_p[h], log_f[h]), f"logits {h}"
    assert list(grad_p) == list(grad_f)
    differ = []
    for n, g in grad_p.items():
        if g is None:
            assert grad_f[n] is None, n
            continue
        assert grad_f[n] is not None and grad_f[n].shape == g.shape and bool(torch.isfinite(g).all()), n
        if not torch.equal(g, grad_f[n]):
            differ.append((n, int((g != grad_f[n]).sum())))
    assert not differ, differ[:8]
    assert sum(g is None for g in grad_p.values()) > 0 and any(".ff.w1.weight" in n for n in grad_p)
    # the gradients of a block's w1 / wg are slices of one gradient buffer
    p = "encoder.blocks.0.ff"
    g1, gg = fused.params[p + ".w1.weight"].grad, fused.params[p + ".wg.weight"].grad
    assert g1.untyped_storage().data_ptr() == gg.untyped_storage().data_ptr() and g1.is_contiguous() and gg.is_contiguous()
    assert g1.data_ptr() % 16 == 0 and gg.data_ptr() % 16 == 0


def test_fused_parameters_are_views_of_one_buffer(model):
    plain, fused = TextGrad(model, device=DEV, linear="hip"), TextGrad(model, device=DEV, linear="hip", ff="fused")
    names = [n for n, _ in model.named_parameters()]
    assert list(fused.params) == list(plain.params) == names
    assert [p.shape for p in fused.parameters()] == [p.shape for p in plain.parameters()]
    E = TG.DIMS.embed_dim
    blocks = [f"encoder.blocks.{i}.ff" for i in range(TG.DIMS.enc_block_num)] + [f"decoder.blocks.{i}.ff" for i in range(TG.DIMS.dec_block_num)]
    seen = set()
    for p in blocks:
        for kind, width in (("weight", E), ("bias", 1)):
            a, b = fused.params[f"{p}.w1.{kind}"], fused.params[f"{p}.wg.{kind}"]
            assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr(), (p, kind)
            assert b.data_ptr() - a.data_ptr() == 4 * 2 * E * width                     # w1 first, wg right behind it: torch.cat([w1, wg])
            for t in (a, b):
                assert t.is_leaf and t.requires_grad and t.is_contiguous() and t.data_ptr() % 16 == 0 and t.shape[0] == 2 * E
            seen.add(a.untyped_storage().data_ptr())
            assert torch.equal(a, plain.params[f"{p}.w1.{kind}"]) and torch.equal(b, plain.params[f"{p}.wg.{kind}"])
        pa, pb = plain.params[p + ".w1.weight"], plain.params[p + ".wg.weight"]
        assert pa.untyped_storage().data_ptr() != pb.untyped_storage().data_ptr()
    assert len(seen) == 2 * len(blocks)                                                   # one weight and one bias buffer per block
    for n in names:
        assert torch.equal(fused.params[n], plain.params[n]), n


def test_store_and_load_round_trip():
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    tg = TextGrad(m, device=DEV, linear="hip", ff="fused")
    ptrs = {n: p.data_ptr() for n, p in tg.params.items()}
    tg.store_to_module()
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    with torch.no_grad():                                     # write through the views, store, wipe, load: what was written comes back
        for i, p in enumerate(tg.parameters()):
            p.mul_(1.0 + 0.125 * (i % 3)).add_(0.5)
    want = {n: p.detach().clone() for n, p in tg.params.items()}
    tg.store_to_module()
    with torch.no_grad():
        for p in tg.parameters():
            p.zero_()
    tg.load_from_module()
    for n, p in tg.params.items():
        assert torch.equal(p.detach(), want[n]) and p.data_ptr() == ptrs[n], n
    w14, b14 = tg._ff_buffers["decoder.blocks.1.ff"]
    assert torch.equal(w14, torch.cat([want["decoder.blocks.1.ff.w1.weight"], want["decoder.blocks.1.ff.wg.weight"]], 0))
    assert torch.equal(b14, torch.cat([want["decoder.blocks.1.ff.w1.bias"], want["decoder.blocks.1.ff.wg.bias"]], 0))


def test_fused_needs_the_hip_linear_layers(model):
    with pytest.raises(ValueError):
        TextGrad(model, device=DEV, ff="fused")
    with pytest.raises(ValueError):
        TextGrad(model, device=DEV, linear="torch", ff="fused")
    with pytest.raises(ValueError):
        TextGrad(model, device=DEV, linear="hip", ff="cat")
    assert TextGrad(model, device=DEV).ff == "torch"
