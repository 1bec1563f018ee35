"""-m gpu: findtextcenternet_amd.optim.RAdamScheduleFree -- one ftc_radam_schedulefree_step launch per group and step, one ftc_schedulefree_lerp launch
per group for train() / eval() -- through the class.

  fixture      every case of g22 (the reference's own optimizer on the CPU, tests/golden/gen_golden_radam.py) at the gate of tests/test_gpu_optim.py,
               2e-6 relative + 1e-7: the trajectory, the final state, eval(), train() again; the schedule rows to the last float64 bit
  bitwise      everything else against radam_operands.RAdamModel (float32 NumPy, the kernel's operation order): two groups, GradScaler with a clean and
               with a skipped step, state round trips, and six steps of the small recognizer of tests/text_grad_fixture.py on TextGrad's gradients
"""
import copy

import numpy as np
import pytest
import torch

import radam_operands as R
import step_operands as S
from findtextcenternet_amd import RAdamScheduleFree

pytestmark = pytest.mark.gpu
_CASES = list(range(len(R.RADAM_CASES)))


def _np(t):
    return t.detach().cpu().numpy()


def _cuda_params(arrs):
    return [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in arrs]


def _set_grads(ps, gs, scale=1.0):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else torch.from_numpy(g.copy()).cuda() * scale


def _scaler():
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    scaler.scale(torch.zeros(1, device="cuda"))                          # the scale tensor is made by the first scale(loss) of a loop
    return scaler


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLD)


@pytest.mark.parametrize("ci", _CASES)
def test_fused_step_tracks_the_reference_optimizer(ci, gold):
    def make(params0, kwargs):
        ps = _cuda_params(params0)
        opt = RAdamScheduleFree(ps, **kwargs)
        with pytest.raises(Exception, match="Optimizer was not in train mode when step is called"):
            opt.step()
        return opt, ps, lambda gs: _set_grads(ps, gs), lambda p: opt.state[p]

    got = R.run_case(ci, make, _np)
    assert np.array_equal(got["sched"].view(np.int64), gold[f"c{ci}_sched"].view(np.int64)), (got["sched"], gold[f"c{ci}_sched"])
    for step in range(R.RADAM_STEPS):
        assert R.within_gate(got["steps"][step], gold[f"c{ci}_steps"][step]), (ci, step)
    for kind in ("z", "v", "eval", "train"):
        assert R.within_gate(got[kind], gold[f"c{ci}_{kind}"]), (ci, kind)
    want = R.model_case(ci)                                          # and the whole run bitwise against the model, the two swaps included
    for kind in R.FIXTURE_KINDS:
        S.assert_bits(got[kind], want[kind], (ci, kind))


def _class_pair():
    params, grads = R.class_inputs()
    model = R.RAdamModel([(p, g["kwargs"]) for p, g in zip(params, R.CLASS_GROUPS)])
    ps = [_cuda_params(grp) for grp in params]
    opt = RAdamScheduleFree([dict(params=grp, **g["kwargs"]) for grp, g in zip(ps, R.CLASS_GROUPS)])
    return params, grads, model, ps, opt


def _assert_class_equal(opt, ps, model, params, what, grads_too=True):
    torch.cuda.synchronize()
    for gi, grp in enumerate(ps):
        for pi, p in enumerate(grp):
            w = f"{what} group {gi} parameter {pi}"
            S.assert_bits(_np(p), model.params[gi][pi], (w, "p"))
            if (gi, pi) == R.CLASS_NO_GRAD:
                assert len(opt.state[p]) == 0, w
                S.assert_bytes(_np(p), params[gi][pi], (w, "untouched"))
                continue
            if grads_too:
                S.assert_bits(_np(p.grad), model.grad_out[(gi, pi)], (w, "p.grad"))
            S.assert_bits(_np(opt.state[p]["z"]), model.state[(gi, pi)]["z"], (w, "z"))
            S.assert_bits(_np(opt.state[p]["exp_avg_sq"]), model.state[(gi, pi)]["v"], (w, "exp_avg_sq"))


def test_radam_through_the_optimizer_class_exact():
    """Two parameter groups (lr, betas, weight_decay, silent_sgd_phase differ: one crosses from the silent, one from the SGD phase), one parameter whose
    .grad is None; nine steps: p, p.grad, z and exp_avg_sq bitwise after every step, then eval() and train(); the parameter without a gradient
    untouched and without state throughout."""
    params, grads, model, ps, opt = _class_pair()
    opt.train()
    model.train()
    for step, gs in enumerate(grads):
        for gi, grp in enumerate(ps):
            _set_grads(grp, gs[gi])
        versions = [p._version for grp in ps for p in grp]
        opt.step()
        model.step(gs)
        _assert_class_equal(opt, ps, model, params, f"step {step}")
        moved = [p._version > v for v, p in zip(versions, (p for grp in ps for p in grp))]
        assert moved == [True, True, False, True, True]                  # the raw-pointer writes are announced
        assert [g["k"] for g in opt.param_groups] == [step + 1] * 2
    for to_train in (False, True, True):
        (opt.train if to_train else opt.eval)()
        (model.train if to_train else model.eval)()
        _assert_class_equal(opt, ps, model, params, f"train_mode {to_train}", grads_too=False)
    assert all(g["train_mode"] for g in opt.param_groups)


def test_gradscaler_clean_steps_equal_plain_steps():
    """torch.amp.GradScaler on its generic path: gradients pre-multiplied by 65536 (a power of two: unscale_ is exact), across the phase crossing."""
    params, grads, model, ps, opt = _class_pair()
    scaler = _scaler()
    opt.train()
    model.train()
    for step, gs in enumerate(grads[:7]):
        for gi, grp in enumerate(ps):
            _set_grads(grp, gs[gi], 65536.0)
        scaler.step(opt)
        scaler.update()
        model.step(gs)
        _assert_class_equal(opt, ps, model, params, f"scaled step {step}")
    assert scaler.get_scale() == 65536.0 and [g["k"] for g in opt.param_groups] == [7, 7]


def test_gradscaler_skips_a_step_with_an_infinite_gradient():
    params, grads, model, ps, opt = _class_pair()
    scaler = _scaler()
    opt.train()
    model.train()
    for gs in grads[:6]:
        for gi, grp in enumerate(ps):
            _set_grads(grp, gs[gi], 65536.0)
        scaler.step(opt)
        scaler.update()
        model.step(gs)
    torch.cuda.synchronize()
    tensors = [t for grp in ps for p in grp for t in [p] + [opt.state[p][k] for k in ("z", "exp_avg_sq") if k in opt.state[p]]]
    before = [_np(t).copy() for t in tensors]
    books = [(g["k"], g["lr_max"], g["weight_sum"], g["scheduled_lr"]) for g in opt.param_groups]
    for gi, grp in enumerate(ps):
        _set_grads(grp, grads[6][gi], 65536.0)
    ps[1][1].grad[3, 2] = float("inf")
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    for t, b in zip(tensors, before):
        S.assert_bytes(_np(t), b, "a skipped step wrote")
    assert [(g["k"], g["lr_max"], g["weight_sum"], g["scheduled_lr"]) for g in opt.param_groups] == books and books[0][0] == 6
    assert scaler.get_scale() == 32768.0
    for gi, grp in enumerate(ps):                                        # the next clean step is the model's step k + 1 = 7
        _set_grads(grp, grads[6][gi], 32768.0)
    scaler.step(opt)
    scaler.update()
    model.step(grads[6])
    _assert_class_equal(opt, ps, model, params, "the step after the skipped one")
    assert [g["k"] for g in opt.param_groups] == [7, 7]


def test_state_round_trips_rebuild_the_pointer_table():
    """state_dict() -> load_state_dict() into a fresh instance and into the live one (new state tensors behind unchanged parameter and gradient
    addresses), and copy.deepcopy (the table cache is not copied): the next step is bitwise the live one."""
    params, grads, model, ps, opt = _class_pair()
    opt.train()
    for gs in grads[:6]:
        for gi, grp in enumerate(ps):
            _set_grads(grp, gs[gi])
        opt.step()
    saved = copy.deepcopy(opt.state_dict())
    assert set(saved["state"][0]) == {"z", "exp_avg_sq"} and saved["param_groups"][0]["k"] == 6 and saved["param_groups"][0]["train_mode"] is True
    snap = [[p.detach().clone() for p in grp] for grp in ps]
    twin = copy.deepcopy(opt)
    assert "_tables" not in twin.__dict__ and "_tables" in opt.__dict__
    for gi, grp in enumerate(ps):
        _set_grads(grp, grads[6][gi])
    opt.step()
    torch.cuda.synchronize()
    live = [[(_np(p).copy(), {k: _np(v).copy() for k, v in opt.state[p].items()}) for p in grp] for grp in ps]

    def same_as_live(o, groups, what):
        torch.cuda.synchronize()
        for gi, grp in enumerate(groups):
            for pi, p in enumerate(grp):
                S.assert_bits(_np(p), live[gi][pi][0], (what, gi, pi, "p"))
                assert set(o.state[p]) == set(live[gi][pi][1]), (what, gi, pi)
                for k, v in live[gi][pi][1].items():
                    S.assert_bits(_np(o.state[p][k]), v, (what, gi, pi, k))
        assert [g["k"] for g in o.param_groups] == [7, 7] and [g["weight_sum"] for g in o.param_groups] == [g["weight_sum"] for g in opt.param_groups]

    fresh_ps = [[torch.nn.Parameter(t.clone()) for t in grp] for grp in snap]
    fresh = RAdamScheduleFree([dict(params=grp) for grp in fresh_ps])
    fresh.load_state_dict(copy.deepcopy(saved))                       # (a load may adopt the tensors it is given)
    twin_ps = [g["params"] for g in twin.param_groups]
    for o, groups, what in ((fresh, fresh_ps, "fresh instance"), (twin, twin_ps, "deep copy")):
        for gi, grp in enumerate(groups):
            _set_grads(grp, grads[6][gi])
        o.step()
        same_as_live(o, groups, what)
    books = [g["weight_sum"] for g in opt.param_groups]
    with torch.no_grad():
        for grp, sgrp in zip(ps, snap):
            for p, s in zip(grp, sgrp):
                p.copy_(s)
    opt.load_state_dict(copy.deepcopy(saved))                # the live instance: NEW z / exp_avg_sq tensors, old addresses in the cached table
    for gi, grp in enumerate(ps):
        for p, g in zip(grp, grads[6][gi]):
            if g is not None:
                p.grad.copy_(torch.from_numpy(g))
    opt.step()
    assert [g["weight_sum"] for g in opt.param_groups] == books
    same_as_live(opt, ps, "reloaded live instance")


def test_cpu_parameters_fail_loudly():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = RAdamScheduleFree([p])
    opt.train()
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()


def test_recognizer_trains_on_textgrad_gradients_exact():
    """train3.py:120-121 on the project's own pieces: RAdamScheduleFree(tg.parameters(), lr=2e-4) over the small recognizer, six steps on one batch
    (four silent, the crossing, one more).  Per step the gradients TextGrad left are copied to the host and the NumPy model applied to THOSE: every
    parameter, z and exp_avg_sq bitwise.  The self-attention pos_emb_k tables have no gradient: no state, not moved.  After eval() the module gets x."""
    import text_grad_fixture as TG
    from findtextcenternet_amd import Transformer
    from findtextcenternet_amd.text_grad import TextGrad
    m = Transformer(**TG.DIMS.__dict__)
    m.load_state_dict(TG.state_dict())
    tg = TextGrad(m, device="cuda:0")
    names = [n for n, _ in m.named_parameters()]
    plist = tg.parameters()
    assert len(plist) == len(names) and all(p is tg.params[n] for p, n in zip(plist, names))
    assert [tuple(p.shape) for p in plist] == [tuple(p.shape) for p in m.parameters()]
    opt = RAdamScheduleFree(plist, lr=2e-4)
    start = [_np(p).copy() for p in plist]
    model = R.RAdamModel([(start, dict(lr=2e-4))])
    enc, dec, label = (torch.from_numpy(a).cuda() for a in TG.make_inputs())
    opt.train()
    model.train()
    unread = None
    for step in range(6):
        res = tg.forward_backward(enc, dec, label)
        assert np.isfinite(float(res["loss"]))
        gs = [None if p.grad is None else _np(p.grad).copy() for p in plist]
        if unread is None:                                                 # the tables no kernel reads: a self-attention's pos_emb_k
            unread = [i for i, g in enumerate(gs) if g is None]
            assert unread and all("pos_emb_k" in names[i] and "cross_attn" not in names[i] for i in unread)
        assert [i for i, g in enumerate(gs) if g is None] == unread
        opt.step()
        model.step([gs])
        torch.cuda.synchronize()
        for i, p in enumerate(plist):
            S.assert_bits(_np(p), model.params[0][i], (step, names[i], "p"))
            if i in unread:
                assert len(opt.state[p]) == 0
                S.assert_bytes(_np(p), start[i], (step, names[i], "untouched"))
                continue
            S.assert_bits(_np(opt.state[p]["z"]), model.state[(0, i)]["z"], (step, names[i], "z"))
            S.assert_bits(_np(opt.state[p]["exp_avg_sq"]), model.state[(0, i)]["v"], (step, names[i], "exp_avg_sq"))
    moved = sum(1 for i, p in enumerate(plist) if i not in unread and not np.array_equal(_np(p), start[i]))
    assert moved > len(plist) // 2 and opt.param_groups[0]["k"] == 6 and opt.param_groups[0]["scheduled_lr"] > 0
    opt.eval()
    model.eval()
    tg.store_to_module()
    for i, (n, p) in enumerate(m.named_parameters()):
        S.assert_bits(_np(p), model.params[0][i], (n, "x in the module"))
