"""-m gpu: findtextcenternet_amd.optim.RAdam -- torch.optim.RAdam as one ftc_radam_step launch per group and distinct step value -- through the class.

  fixture      every case of g27 (torch.optim.RAdam's own single-tensor path on the CPU, tests/golden/gen_golden_radam_plain.py) at the gate of
               tests/test_gpu_optim.py, 2e-6 relative + 1e-7: the trajectory, the final exp_avg / exp_avg_sq, the step values exactly
  bitwise      the same runs against radam_plain_operands.RAdamPlainModel (float32 NumPy, the kernel's operation order)
  state        state_dict() into a CPU torch.optim.RAdam and back into a fresh instance, continuing under the gate on both sides
  launches     read from the class: one per group while every active parameter has the same step value, one per distinct value otherwise
"""
import copy

import numpy as np
import pytest
import torch

import radam_plain_operands as P
import step_operands as S
from findtextcenternet_amd import RAdam

pytestmark = pytest.mark.gpu
_CASES = list(range(len(P.PLAIN_CASES)))


def _np(t):
    return t.detach().cpu().numpy()


def _params(arrs, device="cuda"):
    return [torch.nn.Parameter(torch.from_numpy(a.copy()).to(device)) for a in arrs]


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else torch.from_numpy(g.copy()).to(p.device)


@pytest.fixture(scope="module")
def gold():
    return np.load(P.GOLD)


@pytest.mark.parametrize("ci", _CASES)
def test_fused_step_tracks_torch_optim_radam(ci, gold):
    made = []

    def make(params0, kwargs):
        ps = _params(params0)
        opt = RAdam(ps, **kwargs)
        made.append(opt)
        return opt, ps, lambda gs: _set_grads(ps, gs), lambda p: opt.state[p]

    got = P.run_case(ci, make, _np)
    for step in range(P.PLAIN_STEPS):
        assert P.within_gate(got["steps"][step], gold[f"c{ci}_steps"][step]), (ci, step)
    for kind in ("m", "v"):
        assert P.within_gate(got[kind], gold[f"c{ci}_{kind}"]), (ci, kind)
    assert got["step"].tolist() == gold[f"c{ci}_step"].tolist() == [8.0, 6.0, 8.0, 8.0]
    want = P.model_case(ci)                                          # and the whole run bitwise against the model
    for kind in P.FIXTURE_KINDS:
        S.assert_bits(got[kind], want[kind], (ci, kind))
    opt = made[0]
    assert opt.launches == want["launches"] == 12                    # steps 1-4 one launch, steps 5-8 two: parameter 1 lags two steps behind
    st = opt.state[opt.param_groups[0]["params"][0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0


def test_one_launch_per_group_and_versions_move():
    """Two groups with different hyper-parameters, every parameter with a gradient on every step: one launch per group and step; the raw-pointer
    writes are announced through the version counters; a parameter without a gradient is not touched and gets no state."""
    rng = np.random.Generator(np.random.PCG64(31))
    shapes = [[(4097,), (3, 3, 3, 3)], [(37, 5), (1,), (8,)]]
    kw = [dict(lr=1e-3, weight_decay=0.01), dict(lr=5e-3, betas=(0.8, 0.99), weight_decay=0.01, decoupled_weight_decay=True)]
    arrs = [[rng.standard_normal(s).astype(np.float32) for s in grp] for grp in shapes]
    ps = [_params(grp) for grp in arrs]
    opt = RAdam([dict(params=grp, **k) for grp, k in zip(ps, kw)])
    model = P.RAdamPlainModel([(grp, k) for grp, k in zip(arrs, kw)])
    for step in range(7):
        gs = [[None if (gi, pi) == (1, 2) else (rng.standard_normal(s) * 0.1).astype(np.float32) for pi, s in enumerate(grp)] for gi, grp in enumerate(shapes)]
        for grp, g in zip(ps, gs):
            _set_grads(grp, g)
        versions = [p._version for grp in ps for p in grp]
        opt.step()
        model.step(gs)
        assert opt.launches == 2 * (step + 1) == model.launches
        assert [p._version > v for v, p in zip(versions, (p for grp in ps for p in grp))] == [True, True, True, True, False]
        torch.cuda.synchronize()
        for gi, grp in enumerate(ps):
            for pi, p in enumerate(grp):
                S.assert_bits(_np(p), model.params[gi][pi], (step, gi, pi, "p"))
                if (gi, pi) == (1, 2):
                    assert len(opt.state[p]) == 0
                    S.assert_bytes(_np(p), arrs[gi][pi], "untouched")
                    continue
                S.assert_bits(_np(opt.state[p]["exp_avg"]), model.state[(gi, pi)]["m"], (step, gi, pi, "exp_avg"))
                S.assert_bits(_np(opt.state[p]["exp_avg_sq"]), model.state[(gi, pi)]["v"], (step, gi, pi, "exp_avg_sq"))
                S.assert_bytes(_np(p.grad), gs[gi][pi], "the gradient is not written")
                assert float(opt.state[p]["step"]) == step + 1


def test_state_dict_moves_to_torch_optim_radam_and_back():
    """Four steps here, state_dict() into torch.optim.RAdam on the CPU, two steps on both; torch's state_dict() into a FRESH instance of this class, two
    more steps on both: parameters and state agree under the gate throughout, the per-parameter step values exactly (the parameter that had no
    gradient on steps 3 and 4 stays two behind)."""
    ci = 1
    params0, grads = P.plain_case(ci)
    kwargs = P.PLAIN_CASES[ci]["kwargs"]
    ps = _params(params0)
    opt = RAdam(ps, **kwargs)
    for gs in grads[:4]:
        _set_grads(ps, gs)
        opt.step()
    saved = copy.deepcopy(opt.state_dict())
    assert set(saved["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and [float(saved["state"][i]["step"]) for i in range(4)] == [4.0, 2.0, 4.0, 4.0]
    cps = _params([_np(p) for p in ps], "cpu")
    ref = torch.optim.RAdam(cps, foreach=False, **kwargs)
    ref.load_state_dict(saved)
    assert all(ref.state[p]["exp_avg"].device.type == "cpu" for p in cps)

    def same(a_opt, a_ps, b_opt, b_ps, what):
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(a_ps, b_ps)):
            assert P.within_gate(_np(a), _np(b)), (what, i, "p")
            for k in ("exp_avg", "exp_avg_sq"):
                assert P.within_gate(_np(a_opt.state[a][k]), _np(b_opt.state[b][k])), (what, i, k)
            assert float(a_opt.state[a]["step"]) == float(b_opt.state[b]["step"]), (what, i)

    same(opt, ps, ref, cps, "after the load")
    for gs in grads[4:6]:
        _set_grads(ps, gs)
        _set_grads(cps, gs)
        opt.step()
        ref.step()
        same(opt, ps, ref, cps, "torch continues")
    back = copy.deepcopy(ref.state_dict())
    fresh_ps = _params([_np(p) for p in cps])
    fresh = RAdam(fresh_ps, **kwargs)
    fresh.load_state_dict(back)
    assert all(fresh.state[p]["exp_avg"].is_cuda for p in fresh_ps) and [float(fresh.state[p]["step"]) for p in fresh_ps] == [6.0, 4.0, 6.0, 6.0]
    for gs in grads[6:]:
        for group in (ps, cps, fresh_ps):
            _set_grads(group, gs)
        opt.step()
        ref.step()
        fresh.step()
        same(fresh, fresh_ps, ref, cps, "back from torch")
        same(fresh, fresh_ps, opt, ps, "back from torch against the uninterrupted run")
    want = P.model_case(ci)                                          # the uninterrupted run is still the model's, bitwise
    S.assert_bits(P.gather([_np(p) for p in ps]), want["steps"][-1], "uninterrupted")
    twin = copy.deepcopy(opt)                                        # the table cache and the step mirror are not copied
    assert "_tables" not in twin.__dict__ and "_tables" in opt.__dict__ and "_step_mirror" not in twin.__dict__


def test_refusals():
    p = torch.nn.Parameter(torch.zeros(8))
    opt = RAdam([p])
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    q = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match="maximize=True is not supported"):
        RAdam([q], maximize=True)
    opt = RAdam([q])
    opt.param_groups[0]["capturable"] = True                         # set after construction, as a loaded state dict could
    q.grad = torch.ones(8, device="cuda")
    with pytest.raises(ValueError, match="capturable=True is not supported"):
        opt.step()
    torch.cuda.synchronize()
    assert opt.launches == 0 and not q.detach().any()
    h = torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float16))
    h.grad = torch.ones(8, device="cuda", dtype=torch.float16)
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        RAdam([h]).step()
