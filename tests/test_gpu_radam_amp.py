"""-m gpu: RAdamScheduleFree(schedule="device") and AmpScaler through the classes -- the schedule on the device (ftc_radam_sf_schedule), the project's own
scan (ftc_amp_nonfinite_scan) and the update on device scalars (ftc_radam_schedulefree_step_dev), one launch per group.

  host mode      the yardstick: the same class with schedule="host" under torch.amp.GradScaler's generic path (tests/test_gpu_radam.py pins it against the
                 reference's fixture and the NumPy model); everything here is bit for bit against it, and against radam_device_operands.RAdamDeviceModel
  capture        scaler.step(opt); scaler.update() inside torch.cuda.graph: one stream, a linear chain.  A capture refuses any host read of the device, so
                 this is the proof that the step is sync-free; host mode cannot pass it (GradScaler's generic path reads found_inf with .item())
"""
import copy

import numpy as np
import pytest
import torch

import radam_device_operands as D
import radam_operands as R
import step_operands as S
from findtextcenternet_amd import AmpScaler, RAdamScheduleFree

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _cuda_params(arrs):
    return [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in arrs]


def _set_grads(ps, gs, scale=1.0):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else torch.from_numpy(g.copy()).cuda() * scale


def _torch_scaler(**kw):
    scaler = torch.amp.GradScaler("cuda", init_scale=D.CLASS_SCALE, **kw)
    scaler.scale(torch.zeros(1, device="cuda"))                          # the scale tensor is made by the first scale(loss) of a loop
    return scaler


def _make(schedule, params=None):
    params = R.class_inputs()[0] if params is None else params
    ps = [_cuda_params(grp) for grp in params]
    opt = RAdamScheduleFree([dict(params=grp, **g["kwargs"]) for grp, g in zip(ps, R.CLASS_GROUPS)], schedule=schedule)
    opt.train()
    return ps, opt


def _snapshot(ps, opt):
    torch.cuda.synchronize()
    out = []
    for grp in ps:
        for p in grp:
            st = opt.state[p]
            out.append((_np(p).copy(), None if "z" not in st else _np(st["z"]).copy(), None if "z" not in st else _np(st["exp_avg_sq"]).copy()))
    return out


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("p", "z", "exp_avg_sq"), x, y):
            assert (u is None) == (v is None), (what, i, name)
            if u is not None:
                S.assert_bits(u, v, (what, f"tensor {i}", name))


def _scaled_run(schedule, make_scaler, steps=R.CLASS_STEPS):
    """CLASS_GROUPS, nine steps, gradients times the current scale, an inf in one element of group 1 before step 4 -> snapshots per step, ..."""
    grads = R.class_inputs()[1]
    ps, opt = _make(schedule)
    scaler = make_scaler()
    scale, shots, scales = D.CLASS_SCALE, [], []
    for step, gs in enumerate(grads[:steps], 1):
        for gi, grp in enumerate(ps):
            _set_grads(grp, gs[gi], scale)
        if step == D.CLASS_INF_STEP:
            gi, pi, at = D.CLASS_INF_AT
            ps[gi][pi].grad[at] = float("inf")
        scaler.step(opt)
        scaler.update()
        shots.append(_snapshot(ps, opt))
        scale = scaler.get_scale()
        scales.append(scale)
    return ps, opt, scaler, shots, scales


def _model_snapshot(m):
    out = []
    for gi, grp in enumerate(m.params):
        for pi, p in enumerate(grp):
            st = m.state.get((gi, pi))
            out.append((p, None if st is None else st["z"], None if st is None else st["v"]))
    return out


@pytest.fixture(scope="module")
def host_run():
    """The yardstick, computed once: host mode under torch.amp.GradScaler."""
    ps, opt, scaler, shots, scales = _scaled_run("host", _torch_scaler)
    return dict(shots=shots, scales=scales, groups=copy.deepcopy([{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]))


@pytest.mark.parametrize("which", ["GradScaler", "AmpScaler"])
def test_device_mode_equals_host_mode_under_a_scaler(which, host_run):
    make = _torch_scaler if which == "GradScaler" else (lambda: AmpScaler(init_scale=D.CLASS_SCALE))
    ps, opt, scaler, shots, scales = _scaled_run("device", make)
    for step, (a, b) in enumerate(zip(shots, host_run["shots"]), 1):
        _assert_same(a, b, (which, f"step {step}"))
    assert scales == host_run["scales"] == [65536.0] * 3 + [32768.0] * 6 and scaler.get_scale() == 32768.0
    model, trace, mscale = D.class_run(own_scan=which == "AmpScaler")
    _assert_same(shots[-1], _model_snapshot(model), (which, "the NumPy model"))
    assert [g["k"] for g in opt.param_groups] == [0, 0]                       # the mirrors are stale until they are synced
    opt.sync_schedule()
    for g, h, m in zip(opt.param_groups, host_run["groups"], model.groups):
        assert g["k"] == h["k"] == 8
        for key in ("lr_max", "weight_sum", "scheduled_lr"):
            assert g[key] == m[key], (which, key)                             # the model of the contract: every float64 bit
            assert abs(g[key] - h[key]) <= D.GATE64 * abs(h[key]), (which, key, g[key], h[key])
    if which == "AmpScaler":                                                  # the one stated difference: a skipped step leaves the gradients scaled
        ps2, opt2 = _make("device")
        s2 = AmpScaler(init_scale=D.CLASS_SCALE)
        for gi, grp in enumerate(ps2):
            _set_grads(grp, R.class_inputs()[1][0][gi], D.CLASS_SCALE)
        ps2[1][1].grad[3, 2] = float("nan")
        kept = [None if p.grad is None else _np(p.grad).copy() for grp in ps2 for p in grp]
        s2.step(opt2)
        s2.update()
        torch.cuda.synchronize()
        for p, g in zip((p for grp in ps2 for p in grp), kept):
            if g is not None:
                S.assert_bytes(_np(p.grad), g, "a skipped step wrote a gradient")
        assert s2.get_scale() == 32768.0


def test_scale_grows_on_schedule_as_torchs():
    mk_t = lambda: _torch_scaler(growth_interval=2)                           # noqa: E731
    mk_a = lambda: AmpScaler(init_scale=D.CLASS_SCALE, growth_interval=2)     # noqa: E731
    _, _, st, shots_t, scales_t = _scaled_run("host", mk_t)
    _, _, sa, shots_a, scales_a = _scaled_run("device", mk_a)
    assert scales_a == scales_t == [65536.0, 131072.0, 131072.0, 65536.0, 65536.0, 131072.0, 131072.0, 262144.0, 262144.0]
    for step, (a, b) in enumerate(zip(shots_a, shots_t), 1):
        _assert_same(a, b, f"growth step {step}")
    sd = sa.state_dict()
    assert sd["scale"] == 262144.0 and sd["growth_interval"] == 2 and sd["_growth_tracker"] == st.state_dict()["_growth_tracker"]
    other = AmpScaler()
    other.load_state_dict(sd)
    assert other.get_scale() == 262144.0 and other.state_dict() == sd


def test_amp_step_is_captured_into_a_graph_and_replays_the_eager_run():
    """One eager warm-up step, then scaler.step(opt); scaler.update() captured on static gradient buffers and replayed six times, one of them with a
    NaN: parameters, state, schedule and scale equal the eager device-mode run bit for bit.  Capture is the proof of 'no host read'."""
    grads = R.class_inputs()[1]
    live = [(gi, pi) for gi, g in enumerate(R.CLASS_GROUPS) for pi in range(len(g["shapes"])) if (gi, pi) != R.CLASS_NO_GRAD]

    def fill(ps, step, scale_t):
        for gi, pi in live:
            g = torch.from_numpy(grads[step][gi][pi]).cuda() * scale_t
            if step == 4 and (gi, pi) == (0, 0):
                g[4096] = float("nan")                                         # the lone element of the second chunk
            if ps[gi][pi].grad is None:
                ps[gi][pi].grad = g.clone()
            else:
                ps[gi][pi].grad.copy_(g)

    # eager
    ps_e, opt_e = _make("device")
    sc_e = AmpScaler(init_scale=D.CLASS_SCALE)
    for step in range(7):
        fill(ps_e, step, sc_e.scale_tensor)
        sc_e.step(opt_e)
        sc_e.update()
    # captured
    ps_g, opt_g = _make("device")
    sc_g = AmpScaler(init_scale=D.CLASS_SCALE)
    fill(ps_g, 0, sc_g.scale_tensor)
    sc_g.step(opt_g)
    sc_g.update()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sc_g.step(opt_g)
        sc_g.update()
    for step in range(1, 7):
        fill(ps_g, step, sc_g.scale_tensor)
        graph.replay()
    _assert_same(_snapshot(ps_g, opt_g), _snapshot(ps_e, opt_e), "graph replay against eager")
    assert sc_g.get_scale() == sc_e.get_scale() == 32768.0
    opt_g.sync_schedule()
    opt_e.sync_schedule()
    for a, b in zip(opt_g.param_groups, opt_e.param_groups):
        assert a["k"] == b["k"] == 6 and (a["lr_max"], a["weight_sum"], a["scheduled_lr"]) == (b["lr_max"], b["weight_sum"], b["scheduled_lr"])


def _plain_steps(opt, ps, grads, lo, hi):
    for gs in grads[lo:hi]:
        for gi, grp in enumerate(ps):
            _set_grads(grp, gs[gi])
        opt.step()


def test_plain_step_in_device_mode_equals_host_mode():
    """No scaler: schedule and update launches only, the bits of host mode over the phase crossing; an infinite gradient gives NaN and k advances."""
    grads = R.class_inputs()[1]
    ps_h, opt_h = _make("host")
    ps_d, opt_d = _make("device")
    for step in range(R.CLASS_STEPS):
        _plain_steps(opt_h, ps_h, grads, step, step + 1)
        _plain_steps(opt_d, ps_d, grads, step, step + 1)
        _assert_same(_snapshot(ps_d, opt_d), _snapshot(ps_h, opt_h), f"plain step {step + 1}")
        for p, q in zip((p for grp in ps_d for p in grp if p.grad is not None), (p for grp in ps_h for p in grp if p.grad is not None)):
            S.assert_bits(_np(p.grad), _np(q.grad), f"the gradient left by step {step + 1}")
    for ps, opt in ((ps_h, opt_h), (ps_d, opt_d)):
        for gi, grp in enumerate(ps):
            _set_grads(grp, grads[0][gi])
        ps[1][1].grad[3, 2] = float("inf")
        opt.step()
    opt_d.sync_schedule()
    assert [g["k"] for g in opt_d.param_groups] == [g["k"] for g in opt_h.param_groups] == [10, 10]
    _assert_same(_snapshot(ps_d, opt_d), _snapshot(ps_h, opt_h), "after an infinite gradient")
    assert np.isnan(_np(ps_d[1][1])[3, 2]) and np.isfinite(_np(ps_d[1][1])[0, 0])


def test_state_dict_moves_between_host_mode_and_device_mode():
    params, grads = R.class_inputs()
    ps_d, opt_d = _make("device")
    ps_h, opt_h = _make("host")
    _plain_steps(opt_d, ps_d, grads, 0, 5)
    _plain_steps(opt_h, ps_h, grads, 0, 5)
    sd_d, sd_h = copy.deepcopy(opt_d.state_dict()), copy.deepcopy(opt_h.state_dict())
    assert [g["k"] for g in sd_d["param_groups"]] == [5, 5] == [g["k"] for g in sd_h["param_groups"]]          # state_dict() synced first
    assert list(sd_d["param_groups"][0]) == list(sd_h["param_groups"][0])
    now = [[_np(p).copy() for p in grp] for grp in ps_d]
    ps_h2, opt_h2 = _make("host", now)                                         # device -> host
    opt_h2.load_state_dict(sd_d)
    ps_d2, opt_d2 = _make("device", now)                                       # host -> device
    opt_d2.load_state_dict(sd_h)
    twin = copy.deepcopy(opt_d)                                                # and a deep copy of the live device-mode instance
    ps_t = [g["params"] for g in twin.param_groups]
    assert twin._schedule == "device" and [g["k"] for g in twin.param_groups] == [5, 5]
    runs = [(ps_d, opt_d), (ps_h, opt_h), (ps_h2, opt_h2), (ps_d2, opt_d2), (ps_t, twin)]
    for step in (5, 6):
        shots = []
        for ps, opt in runs:
            _plain_steps(opt, ps, grads, step, step + 1)
            shots.append(_snapshot(ps, opt))
        for i, s in enumerate(shots[1:], 1):
            _assert_same(s, shots[0], (f"step {step + 1}", f"run {i}"))
    for ps, opt in runs:
        opt.sync_schedule()
        assert [g["k"] for g in opt.param_groups] == [7, 7]
    opt_d.load_state_dict(sd_h)                                                # the live instance: its device schedule goes back to step 5
    opt_d.sync_schedule()
    assert [g["k"] for g in opt_d.param_groups] == [5, 5]


def test_textgrad_step_without_a_host_read():
    """The small recognizer: forward_backward(grad_scale=scaler.scale_tensor) leaves the .grad bits of grad_scale=65536.0, and three steps of
    AmpScaler + device mode equal three steps of GradScaler + host mode (parameters, z, exp_avg_sq)."""
    import text_grad_fixture as TG
    from findtextcenternet_amd import Transformer
    from findtextcenternet_amd.text_grad import TextGrad

    def make(schedule):
        m = Transformer(**TG.DIMS.__dict__)
        m.load_state_dict(TG.state_dict())
        tg = TextGrad(m, device="cuda:0")
        opt = RAdamScheduleFree(tg.parameters(), lr=2e-4, silent_sgd_phase=False, schedule=schedule)
        opt.train()
        return tg, opt

    enc, dec, label = (torch.from_numpy(a).cuda() for a in TG.make_inputs())
    tg_h, opt_h = make("host")
    tg_d, opt_d = make("device")
    sc_h, sc_d = _torch_scaler(), AmpScaler(init_scale=D.CLASS_SCALE)
    for step in range(3):
        tg_h.forward_backward(enc, dec, label, grad_scale=65536.0)
        tg_d.forward_backward(enc, dec, label, grad_scale=sc_d.scale_tensor)
        torch.cuda.synchronize()
        for p, q in zip(tg_d.parameters(), tg_h.parameters()):
            assert (p.grad is None) == (q.grad is None)
            if p.grad is not None:
                S.assert_bits(_np(p.grad), _np(q.grad), (step, "p.grad"))
        sc_h.step(opt_h)
        sc_h.update()
        sc_d.step(opt_d)
        sc_d.update()
        torch.cuda.synchronize()
        moved = 0
        for p, q in zip(tg_d.parameters(), tg_h.parameters()):
            S.assert_bits(_np(p), _np(q), (step, "p"))
            if p.grad is not None:
                S.assert_bits(_np(opt_d.state[p]["z"]), _np(opt_h.state[q]["z"]), (step, "z"))
                S.assert_bits(_np(opt_d.state[p]["exp_avg_sq"]), _np(opt_h.state[q]["exp_avg_sq"]), (step, "exp_avg_sq"))
                moved += 1
        assert moved > len(tg_d.parameters()) // 2
    assert sc_d.get_scale() == sc_h.get_scale() == 65536.0
    opt_d.sync_schedule()
    assert opt_d.param_groups[0]["k"] == opt_h.param_groups[0]["k"] == 3
