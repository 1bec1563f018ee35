"""-m gpu: TextGrad(model, linear="hip_fp16") -- every linear layer of the recognizer's training forward and backward on fp16 operands
(include/ftc_text_linear_f16.h), run as the reference's AMP step runs: forward_backward(..., grad_scale=65536.0), gradients divided by 65536 -- against
tests/golden/g23_text_grad_f16.npz (the reference's float64 step with exactly that rounding in its linear layers, tests/golden/gen_golden_text_grad_f16.py)
at the g21 gates of tests/test_gpu_text_grad_linear.py: the loss within 2e-4 relative; the logits and every stored gradient entry within 1e-3 of the
largest reference entry (for a ``.bias`` also that of its sibling ``.weight``) + 1e-7; every parameter's L2 norm within 1e-3 relative + 1e-7 sqrt(numel).
What separates the two is fp32 against float64 accumulation and the roundings that such a difference flips -- and a flipped rounding moves an operand
by a whole fp16 ulp, so this distance is NOT the 1e-6 of the fp32 mode.  Measured on an MI355X: loss 1.3e-6 relative; logits 3.0e-4 of range (one
logit of 13.02 off by 2^-8); worst entry error / largest entry 1.4e-4 (decoder.blocks.1.cross_attn.k_proj.weight).  The generator's own construction
run in float32 on the CPU lands at the same distances from the fixture (logits 2^-8, gradients 1.5e-4 at the same parameter): it is what fp32
sums cost under a rounding, not the kernel.

Also: two calls leave the same bits in every ``.grad``; a batch row's logits are the bits of that row run alone; grad_scale = 2^30 leaves non-finite
entries (the loss gradient times 2^30 is far above 65504); ``torch.amp.GradScaler`` then skips ``RAdamScheduleFree``'s step and halves its scale, and a
step at 65536 is taken."""
import numpy as np
import pytest
import torch

import step_operands as S
import text_grad_fixture as TG
from findtextcenternet_amd import RAdamScheduleFree, Transformer
from findtextcenternet_amd.text_grad import TextGrad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 65536.0
G23 = TG.PATH.replace("g21_text_grad.npz", "g23_text_grad_f16.npz")


@pytest.fixture(scope="module")
def g23():
    g = np.load(G23)
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
    tg = TextGrad(model, device=DEV, linear="hip_fp16")
    res = tg.forward_backward(*inputs, grad_scale=SCALE)
    torch.cuda.synchronize()
    return tg, res, {n: (None if g is None else g.clone()) for n, g in tg.grads().items()}


def test_fixture_is_the_fp16_step(g23):
    """The fixture is g21's step with rounded operands: the same inputs, names and picks, distances of the size rounding to 11 bits gives."""
    g21 = TG.load()
    assert [str(n) for n in g23["grad_names"]] == [str(n) for n in g21["grad_names"]] and (g23["grad_pick_index"] == g21["grad_pick_index"]).all()
    assert int(g23["total"]) == int(g21["total"]) and [str(n) for n in g23["grad_none"]] == [str(n) for n in g21["grad_none"]]
    assert 1e-4 < float(g23["g21_grad_distance"]) < 1e-2 and 1e-5 < float(g23["g21_logit_distance"]) < 1e-3 and 1e-7 < float(g23["g21_loss_distance"]) < 1e-4
    # at scale 65536 no linear layer sees a dy that fp16 cannot hold, and next to none below its smallest subnormal
    assert float(g23["dy_absmax"]) < 65504.0 and int(g23["dy_below_2m24"]) <= 1e-5 * int(g23["dy_nonzero"])


def test_loss_counts_and_logits(g23, run, inputs):
    tg, res, _ = run
    enc, dec, _ = inputs
    assert set(res) == {"loss", "correct", "total"}
    print(f"[text grad, fp16 linear] loss {float(res['loss']):.9f} against {float(g23['loss']):.9f}")
    assert abs(float(res["loss"]) - float(g23["loss"])) < 2e-4 * abs(float(g23["loss"]))
    assert int(res["total"]) == int(g23["total"]) and int(res["correct"]) == int(g23["correct"])
    with torch.no_grad():
        lg = tg.logits(enc, dec)
    pos = torch.tensor(TG.LOGIT_POS, device=DEV)
    for h in range(3):
        ref = g23[f"logits{h}"]
        err = np.abs(lg[h][:, pos].double().cpu().numpy() - ref).max()
        print(f"[text grad, fp16 linear] logits {h}: max error {err:.2e} of range {np.abs(ref).max():.2f} ({err / np.abs(ref).max():.2e})")
        assert err <= 1e-3 * np.abs(ref).max() + 1e-7


def test_every_parameter_gradient(g23, run):
    tg, _, grads = run
    names = [str(n) for n in g23["grad_names"]]
    assert names == list(tg.params)
    amax = dict(zip(names, g23["grad_absmax"]))
    none = {str(n) for n in g23["grad_none"]}
    bad, worst = [], (0.0, "")
    for i, n in enumerate(names):
        g = grads[n]
        if n in none:
            assert g is None or float(g.abs().max()) == 0.0, n
            continue
        assert g is not None and g.shape == tg.params[n].shape and bool(torch.isfinite(g).all()), n
        mine = g.double().cpu().numpy().reshape(-1) / SCALE
        norm, ref = float(g23["grad_norms"][i]), g23["grad_picks"][i]
        if abs(float(np.linalg.norm(mine)) - norm) > 1e-3 * norm + 1e-7 * np.sqrt(mine.size):
            bad.append((n, "norm", float(np.linalg.norm(mine)), norm))
        scale = float(amax[n])
        if n.endswith(".bias") and n[:-4] + "weight" in amax:
            scale = max(scale, float(amax[n[:-4] + "weight"]))
        err = float(np.abs(mine[g23["grad_pick_index"][i]] - ref).max())
        if err > 1e-3 * scale + 1e-7:
            bad.append((n, "entries", err, scale))
        worst = max(worst, (err / max(scale, 1e-30), n))
    print(f"[text grad, fp16 linear] {len(names)} parameters, worst entry error / largest entry {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad[:8]


def test_two_calls_leave_the_same_bits_everywhere(g23, run, inputs):
    tg, res, grads = run
    again = tg.forward_backward(*inputs, grad_scale=SCALE)
    torch.cuda.synchronize()
    assert torch.equal(again["loss"], res["loss"])
    none = {str(n) for n in g23["grad_none"]}
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


def test_a_scale_of_two_to_the_thirty_overflows(model, inputs):
    tg = TextGrad(model, device=DEV, linear="hip_fp16")
    res = tg.forward_backward(*inputs, grad_scale=2.0 ** 30)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res["loss"]))          # the forward does not see the scale
    for j in range(3):
        for part in ("weight", "bias"):
            g = tg.params[f"decoder.out_layers.{j}.{part}"].grad
            assert g is not None and not bool(torch.isfinite(g).all()), (j, part)


def _scaler(init_scale):
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    scaler.scale(torch.zeros(1, device="cuda"))                          # the scale tensor is made by the first scale(loss) of a loop
    return scaler


def _books(opt):
    return [g["k"] for g in opt.param_groups]


def _state(tg, opt):
    out = {}
    for n, p in tg.params.items():
        out[n] = p.detach().cpu().numpy().copy()
        for k in ("z", "exp_avg_sq"):
            if k in opt.state.get(p, {}):
                out[n, k] = opt.state[p][k].detach().cpu().numpy().copy()
    return out


def test_gradscaler_skips_the_overflowed_step_and_takes_the_next(model, inputs):
    tg = TextGrad(model, device=DEV, linear="hip_fp16")
    opt = RAdamScheduleFree(tg.parameters(), lr=2e-4)
    opt.train()
    clean, big = _scaler(SCALE), _scaler(2.0 ** 30)
    # a first step at 65536 is taken: there is state to watch afterwards
    tg.forward_backward(*inputs, grad_scale=clean.get_scale())
    clean.step(opt)
    clean.update()
    torch.cuda.synchronize()
    assert _books(opt) == [1] * len(opt.param_groups) and clean.get_scale() == SCALE
    before = _state(tg, opt)
    assert any(isinstance(k, tuple) and k[1] == "z" for k in before) and any(isinstance(k, tuple) and k[1] == "exp_avg_sq" for k in before)
    # the step at 2^30 is skipped: nothing is written, the count stands, the scale halves
    tg.forward_backward(*inputs, grad_scale=big.get_scale())
    big.step(opt)
    big.update()
    torch.cuda.synchronize()
    after = _state(tg, opt)
    assert set(after) == set(before)
    for k, b in before.items():
        S.assert_bytes(after[k], b, f"a skipped step wrote {k}")
    assert _books(opt) == [1] * len(opt.param_groups) and big.get_scale() == 2.0 ** 29
    # a following step at 65536 is taken
    tg.forward_backward(*inputs, grad_scale=clean.get_scale())
    clean.step(opt)
    clean.update()
    torch.cuda.synchronize()
    assert _books(opt) == [2] * len(opt.param_groups) and clean.get_scale() == SCALE
    moved = _state(tg, opt)
    assert any(not np.array_equal(moved[k], before[k]) for k in before)          # (the schedule's first steps move the state, not yet the parameters)
    assert all(np.isfinite(v).all() for v in moved.values())


def test_linear_argument(model):
    for kind in ("torch", "hip", "hip_fp16"):
        assert TextGrad(model, device=DEV, linear=kind).linear == kind
    with pytest.raises(ValueError):
        TextGrad(model, device=DEV, linear="rocblas")
