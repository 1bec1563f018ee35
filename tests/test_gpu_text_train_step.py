"""-m gpu: TextTrainStep -- forward, loss, backward, unscale / skip, optimizer and scale update of the recognizer's AMP step replayed as one HIP
graph -- against the plain loop

    tg.forward_backward(enc, dec, label, grad_scale=scaler.scale_tensor); scaler.step(opt); scaler.update()

on an independent TextGrad built with today's arguments (``ff`` at its default), its own RAdamScheduleFree(schedule="device") and its own AmpScaler.
SMALL recognizer, ``text_grad_fixture.make_inputs(seed)`` ([2, 400, 106]), scale 65536.  Every gate is equality of bits: after every step the loss,
the counts and the scale; at the end every parameter, ``z``, ``exp_avg_sq`` and ``.grad``, and the synced schedule.  Eight steps on different batches,
the fifth with a NaN in ``enc_input`` (skipped on the device: the scale halves, k stays behind by one) with ONE capture; an lr halved after step 3
captures again; ``opt.eval(); opt.train()`` between replays needs no capture; ``load_state_dict`` drops the graph and the next call is eager; a second
shape gets its own graph and the first one's is kept; what the step cannot drive is refused before any GPU work."""
import numpy as np
import pytest
import torch

import text_grad_fixture as TG
from findtextcenternet_amd import AmpScaler, RAdamScheduleFree, TextTrainStep, Transformer
from findtextcenternet_amd.text_grad import TextGrad

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 65536.0
MODE = dict(linear="hip_fp16", attention="hip_fp16")


@pytest.fixture(scope="module")
def model():
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    return m


@pytest.fixture(scope="module")
def batches():
    """Eight batches [2, 400, 106]; number 4 (the fifth step) carries one NaN in enc_input."""
    out = []
    for i in range(8):
        enc, dec, label = (torch.from_numpy(x).to(DEV) for x in TG.make_inputs(2101 + i))
        if i == 4:
            enc[1, 3, 17] = float("nan")
        out.append((enc, dec, label))
    return out


def _make(model, graph, lr=2e-4):
    tg = TextGrad(model, device=DEV, ff="fused", **MODE) if graph else TextGrad(model, device=DEV, **MODE)
    opt = RAdamScheduleFree(tg.parameters(), lr=lr, schedule="device")
    opt.train()
    scaler = AmpScaler(init_scale=SCALE)
    step = TextTrainStep(tg, opt, scaler) if graph else None
    return tg, opt, scaler, step


def _plain(tg, opt, scaler, batch):
    res = tg.forward_backward(*batch, grad_scale=scaler.scale_tensor)
    scaler.step(opt)
    scaler.update()
    return res


def _same_step(res, ref, scaler, ref_scaler, meta):
    assert torch.equal(res["loss"], ref["loss"]) or (bool(torch.isnan(res["loss"])) and bool(torch.isnan(ref["loss"]))), (meta, float(res["loss"]), float(ref["loss"]))
    assert int(res["correct"]) == int(ref["correct"]) and int(res["total"]) == int(ref["total"]), meta
    assert scaler.get_scale() == ref_scaler.get_scale(), meta


def _same_state(a, b, meta=""):
    """(tg, opt) pairs: parameters, z, exp_avg_sq and .grad bit for bit (NaN patterns included), the synced schedule equal."""
    (tg_a, opt_a), (tg_b, opt_b) = a, b
    assert list(tg_a.params) == list(tg_b.params)
    for n in tg_a.params:
        pa, pb = tg_a.params[n], tg_b.params[n]
        pairs = [("param", pa.detach(), pb.detach()), ("grad", pa.grad, pb.grad)]
        for k in ("z", "exp_avg_sq"):
            pairs.append((k, opt_a.state.get(pa, {}).get(k), opt_b.state.get(pb, {}).get(k)))
        for kind, x, y in pairs:
            assert (x is None) == (y is None), (meta, n, kind)
            if x is not None:
                assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32)), (meta, n, kind)
    opt_a.sync_schedule()
    opt_b.sync_schedule()
    for ga, gb in zip(opt_a.param_groups, opt_b.param_groups):
        for k in ("k", "lr_max", "weight_sum", "scheduled_lr", "lr"):
            assert ga[k] == gb[k], (meta, k, ga[k], gb[k])


def test_eight_steps_one_capture(model, batches):
    tg, opt, scaler, step = _make(model, True)
    rtg, ropt, rscaler, _ = _make(model, False)
    outs = None
    for i, batch in enumerate(batches):
        res = step(*batch)
        ref = _plain(rtg, ropt, rscaler, batch)
        _same_step(res, ref, scaler, rscaler, f"step {i + 1}")
        if outs is None:
            outs = res
        assert all(res[k] is outs[k] for k in ("loss", "correct", "total"))          # static outputs
        assert res["loss"].dim() == 0 and res["loss"].is_cuda and res["correct"].dtype == torch.int64
        assert step.captures == (0 if i == 0 else 1)
        if i == 4:
            assert bool(torch.isnan(res["loss"]))
    _same_state((tg, opt), (rtg, ropt), "after eight steps")
    assert scaler.get_scale() == 32768.0 and [g["k"] for g in opt.param_groups] == [7] * len(opt.param_groups)
    assert step.captures == 1 and step.graphs == [(2, 400, 400)]
    # the gradients live at fixed, 16-byte aligned addresses
    ptrs = [p.grad.data_ptr() for p in tg.parameters() if p.grad is not None]
    step(*batches[0])
    _plain(rtg, ropt, rscaler, batches[0])
    assert ptrs == [p.grad.data_ptr() for p in tg.parameters() if p.grad is not None] and all(a % 16 == 0 for a in ptrs)
    assert sum(p.grad is None for p in tg.parameters()) == sum(p.grad is None for p in rtg.parameters()) > 0
    _same_state((tg, opt), (rtg, ropt), "after a ninth step")
    # eager() is the same step with no graph; reset() drops the graph and the next call captures again
    step.eager(*batches[1])
    _plain(rtg, ropt, rscaler, batches[1])
    step.reset()
    assert step.graphs == []
    step(*batches[2])
    _plain(rtg, ropt, rscaler, batches[2])
    assert step.captures == 2
    _same_state((tg, opt), (rtg, ropt), "after eager, reset and a new capture")


def test_lr_change_captures_again(model, batches):
    tg, opt, scaler, step = _make(model, True)
    rtg, ropt, rscaler, _ = _make(model, False)
    for i in range(6):
        if i == 3:
            for o in (opt, ropt):
                for g in o.param_groups:
                    g["lr"] = g["lr"] * 0.5
        res, ref = step(*batches[i]), _plain(rtg, ropt, rscaler, batches[i])
        _same_step(res, ref, scaler, rscaler, f"step {i + 1}")
        assert step.captures == (0, 1, 1, 2, 2, 2)[i]
    _same_state((tg, opt), (rtg, ropt), "lr halved after step 3")
    assert opt.param_groups[0]["lr"] == 1e-4


def test_eval_and_train_between_replays(model, batches):
    tg, opt, scaler, step = _make(model, True)
    rtg, ropt, rscaler, _ = _make(model, False)
    for i in range(5):
        if i == 3:
            for o in (opt, ropt):
                o.eval()
            with pytest.raises(Exception, match="train"):
                step(*batches[i])
            for o in (opt, ropt):
                o.train()
        res, ref = step(*batches[i]), _plain(rtg, ropt, rscaler, batches[i])
        _same_step(res, ref, scaler, rscaler, f"step {i + 1}")
    assert step.captures == 1
    _same_state((tg, opt), (rtg, ropt), "eval / train between replays")


def test_load_state_dict_drops_the_graph(model, batches):
    tg, opt, scaler, step = _make(model, True)
    rtg, ropt, rscaler, _ = _make(model, False)
    for i in range(2):
        step(*batches[i]), _plain(rtg, ropt, rscaler, batches[i])
    sd, rsd = opt.state_dict(), ropt.state_dict()
    for i in range(2, 4):
        step(*batches[i]), _plain(rtg, ropt, rscaler, batches[i])
    assert step.captures == 1 and step.graphs
    opt.load_state_dict(sd)
    ropt.load_state_dict(rsd)
    assert step.graphs == []
    for i in range(4, 6):
        res, ref = step(*batches[i]), _plain(rtg, ropt, rscaler, batches[i])
        _same_step(res, ref, scaler, rscaler, f"step {i + 1}")
        assert step.captures == (1, 2)[i - 4]                # the call after the load is an eager one, the next captures
    _same_state((tg, opt), (rtg, ropt), "after load_state_dict")


def test_a_second_shape_gets_its_own_graph(model, batches):
    tg, opt, scaler, step = _make(model, True)
    rtg, ropt, rscaler, _ = _make(model, False)
    one = [tuple(t[:1].clone() for t in b) for b in batches[:3]]
    order = [batches[0], batches[1], one[0], one[1], batches[2], one[2], batches[3]]
    captures = (0, 1, 1, 2, 2, 2, 2)
    for i, batch in enumerate(order):
        res, ref = step(*batch), _plain(rtg, ropt, rscaler, batch)
        _same_step(res, ref, scaler, rscaler, f"call {i + 1}")
        assert step.captures == captures[i], i
    assert step.graphs == [(1, 400, 400), (2, 400, 400)]          # least recently used first
    _same_state((tg, opt), (rtg, ropt), "two shapes")


def test_refusals(model):
    tg = TextGrad(model, device=DEV, ff="fused", **MODE)
    opt = RAdamScheduleFree(tg.parameters(), lr=2e-4, schedule="device")
    with pytest.raises(ValueError, match="device"):
        TextTrainStep(tg, RAdamScheduleFree(tg.parameters(), lr=2e-4), AmpScaler())
    with pytest.raises(TypeError, match="AmpScaler"):
        TextTrainStep(tg, opt, torch.amp.GradScaler("cuda"))
    with pytest.raises(ValueError, match="linear"):
        t = TextGrad(model, device=DEV)
        TextTrainStep(t, RAdamScheduleFree(t.parameters(), schedule="device"), AmpScaler())
    with pytest.raises(ValueError, match="parameters"):
        TextTrainStep(tg, RAdamScheduleFree(tg.parameters()[:-1], schedule="device"), AmpScaler())
    with pytest.raises(ValueError, match="parameters"):
        other = TextGrad(model, device=DEV, **MODE)
        TextTrainStep(tg, RAdamScheduleFree(other.parameters(), schedule="device"), AmpScaler())
    with pytest.raises(TypeError):
        TextTrainStep(model, opt, AmpScaler())
    step = TextTrainStep(tg, opt, AmpScaler())
    assert step.captures == 0 and step.graphs == []
