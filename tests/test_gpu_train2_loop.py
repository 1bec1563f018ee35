"""-m gpu: the detector fine-tune loop of the reference (train2.py:186-204) on the project's own pieces, at B 2 x 128 x 128 in fp32 with the synth
inputs of tests/test_gpu_train_step.py.

train2.py:186-204 verbatim, twice per iteration -- ``fmask = model.get_fmask(labelmap, fmask)``; ``heatmap, decoder_outputs = model(image, fmask)``;
``rawloss = loss_function(fmask, map, idmap, heatmap, decoder_outputs)``; ``loss = CoWloss(rawloss)``; ``loss *= weight``; ``loss.backward()``;
``optimizer.step()``; ``optimizer.zero_grad()`` -- with ``optimizer = RAdam(all_params, lr=lr)`` (train2.py:110) and the second batch of an iteration
passed through ``ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5)`` first (train2.py:30, 194), on the device.

  * the in-place ``loss *= weight`` on CoWloss's output reaches the backward: with weight 0.5 every gradient is 0.5 x the weight-1 gradient of a twin
    model that is handed the same parameters before every step, bit for bit (a power-of-two scale is exact through a linear backward);
  * after two iterations (four optimizer steps) the parameters are those of the float32 model of tests/radam_plain_operands.py applied to the recorded
    gradients, bit for bit.
"""
import numpy as np
import pytest
import torch

import radam_plain_operands as P
import step_operands as S
import synth
from findtextcenternet_amd import ColorJitter, RAdam
from findtextcenternet_amd.loss_func import CoVWeightingLoss, loss_function
from findtextcenternet_amd.train_step import COV_KEYS, TrainStep
from gpu_harness import fresh_model

pytestmark = pytest.mark.gpu
B, H, W, ITERS, LR = 2, 128, 128, 2, 1e-3


def _model():
    return fresh_model("fp32").to("cuda").train()


def _train_step(model, cov, image, labelmap, idmap, fmask):
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):          # train2.py's train_step, as train1.py's
        heatmap, decoder_outputs = model(image, fmask)
        rawloss = loss_function(fmask, labelmap, idmap, heatmap, decoder_outputs)
        loss = cov(rawloss)
    return loss, rawloss


@pytest.fixture(scope="module")
def runs():
    batches = []
    for seed in (161, 163, 165, 167):
        x = torch.from_numpy(synth.page_images(seed, B, H, W)).permute(0, 3, 1, 2).contiguous().cuda()
        label, idmap = synth.train_labels(seed + 1, B, H // 4, W // 4)
        batches.append((x, torch.from_numpy(label).cuda(), torch.from_numpy(idmap).cuda().long()))
    probs = TrainStep(_model()).stochastic_depth_probs()
    rng = np.random.Generator(np.random.PCG64(19))
    keeps = [{n: torch.from_numpy((rng.random(B) < 1 - p).astype(np.float32) / np.float32(1 - p)) for n, p in probs.items()} for _ in batches]
    transform = ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.5)          # train2.py:30

    model, twin = _model(), _model()
    all_params = list(filter(lambda p: p.requires_grad, model.parameters()))                # train2.py:109-110
    twin_params = list(filter(lambda p: p.requires_grad, twin.parameters()))
    optimizer = RAdam(all_params, lr=LR)
    CoWloss, twin_cov = CoVWeightingLoss(device="cuda", losses=COV_KEYS), CoVWeightingLoss(device="cuda", losses=COV_KEYS)
    start = [p.detach().cpu().numpy().copy() for p in all_params]
    CoWloss.train()
    twin_cov.train()
    optimizer.zero_grad()
    fmask = twin_fmask = None
    weight, grads, twin_grads, losses, jittered = 0.5, [], [], [], []
    torch.manual_seed(2)
    step = 0
    for it in range(ITERS):
        for second in (False, True):
            image, labelmap, idmap = batches[step]
            if second:
                before = image
                image = transform(image)                                                    # train2.py:194, on the device
                jittered.append((before, image))
            # the loop under test
            model.stochastic_depth_keep = keeps[step]
            fmask = model.get_fmask(labelmap, fmask)
            loss, rawloss = _train_step(model, CoWloss, image, labelmap, idmap, fmask)
            unweighted = float(loss.detach())
            loss *= weight
            loss.backward()
            grads.append([p.grad.detach().cpu().numpy().copy() for p in all_params])
            # the twin: the same parameters, weight 1
            twin.stochastic_depth_keep = keeps[step]
            twin_fmask = twin.get_fmask(labelmap, twin_fmask)
            twin_loss, _ = _train_step(twin, twin_cov, image, labelmap, idmap, twin_fmask)
            twin_loss *= 1
            twin_loss.backward()
            twin_grads.append([p.grad.detach().cpu().numpy().copy() for p in twin_params])
            losses.append((unweighted, float(loss), float(twin_loss)))
            optimizer.step()
            optimizer.zero_grad()
            with torch.no_grad():
                for a, b in zip(twin_params, all_params):
                    a.copy_(b)
                    a.grad = None
            step += 1
    torch.cuda.synchronize()
    final = [p.detach().cpu().numpy().copy() for p in all_params]
    return dict(start=start, grads=grads, twin_grads=twin_grads, losses=losses, final=final, optimizer=optimizer, jittered=jittered, n=len(all_params))


def test_inplace_loss_weight_reaches_every_gradient(runs):
    assert len(runs["grads"]) == 2 * ITERS
    for step, (gs, ts, (unweighted, weighted, twin)) in enumerate(zip(runs["grads"], runs["twin_grads"], runs["losses"])):
        assert np.isfinite(unweighted) and weighted == 0.5 * unweighted and twin == unweighted, (step, unweighted, weighted, twin)
        moved = 0
        for i, (g, t) in enumerate(zip(gs, ts)):
            S.assert_bits(g, np.float32(0.5) * t, (f"step {step}", f"parameter {i}"))
            moved += bool(np.any(t))
        assert moved > runs["n"] // 2, (step, moved)


def test_parameters_are_the_float32_models_on_the_recorded_gradients(runs):
    model = P.RAdamPlainModel([(runs["start"], dict(lr=LR))])
    for gs in runs["grads"]:
        model.step([gs])
    changed = 0
    for i, (got, want, p0) in enumerate(zip(runs["final"], model.params[0], runs["start"])):
        S.assert_bits(got, want, f"parameter {i} after {2 * ITERS} steps")
        changed += not np.array_equal(got, p0)
    assert changed > runs["n"] // 2
    opt = runs["optimizer"]
    assert opt.launches == 2 * ITERS == model.launches                                     # one group, every parameter with a gradient: one launch per step
    assert all(float(opt.state[p]["step"]) == 2 * ITERS for p in opt.param_groups[0]["params"])


def test_second_batch_of_an_iteration_was_jittered_on_the_device(runs):
    assert len(runs["jittered"]) == ITERS
    for before, after in runs["jittered"]:
        assert after.is_cuda and after.shape == before.shape and after.data_ptr() != before.data_ptr()
        assert float(after.min()) >= 0 and float(after.max()) <= 1 and not torch.equal(before, after)
