"""CPU: the exact BatchNorm operands of tests/bn_operands.py, proved without a GPU.

  * every case tests/test_gpu_exact_bn.py launches is built here; a builder runs its own proofs (exact sums, the four dyadic rows, v / dt / zh fp32 values at
    every step, every pre-activation in a saturated regime, the cancellation ratio of the hard family) and raises when one fails;
  * the float64 models agree with torch.nn.functional.batch_norm(training=True) and its autograd in float64 on the same operands;
  * layout() -- the launch arithmetic restated -- shows that the case lists reach, for each op, every Q, the scalar kernels, a second trip with a masked
    tail in every unrolled loop, empty chunks and chunks that cross an image boundary while the per-image operands differ; the table is printed;
  * discrimination: a dropped row, tail or chunk, a missed per-image reload and an fp32 accumulation each fail the very check the GPU module applies.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import bn_operands as N
from findtextcenternet_amd import _lib as L

CASES = {"bnstat": dict(N.bnstat_cases()), "bnact": dict(N.bnact_cases()), "bnbwd": dict(N.bnbwd_cases())}
BUILD = {"bnstat": N.bnstat_case, "bnact": N.bnact_case, "bnbwd": N.bnbwd_case}
MODEL = {"bnstat": lambda c, drop=None: N.bnstat_model64(c.x, c.gamma, c.beta, c.eps, c.mom, c.run0, drop), "bnact": N.bnact_model64, "bnbwd": N.bnbwd_model64}
CHECK = {"bnstat": N.check_bnstat, "bnact": N.check_bnact, "bnbwd": N.check_bnbwd}


@functools.lru_cache(maxsize=None)
def case(op, cid):
    return BUILD[op](**CASES[op][cid])


def _small(op):
    return [i for i, kw in CASES[op].items() if kw["shape"][0] * kw["shape"][1] * kw["shape"][2] <= 10000]


def _lay(op, cid):
    kw = CASES[op][cid]
    return N.layout(op, kw["shape"], kw.get("idt", L.F32), kw.get("P", 1))


def test_the_gpu_module_runs_these_cases():
    import test_gpu_exact_bn as T
    assert T._STAT == CASES["bnstat"] and T._ACT == CASES["bnact"] and T._BWD == CASES["bnbwd"]


@pytest.mark.parametrize("op", ["bnstat", "bnact", "bnbwd"])
def test_every_case_is_exact_and_its_own_model_passes_the_gpu_checks(op):
    for cid in CASES[op]:
        c = case(op, cid)
        if c.shape[0] * c.shape[1] * c.shape[2] <= 10000:               # (the large cases: the builder's proofs only; their model IS c.ref)
            CHECK[op](c, *N.as_kernel_output(op, c, MODEL[op](c)), cid)


def test_regimes_of_the_activated_cases():
    """pass: every v >= PASS_MIN; mixed: blocked channels v <= BLOCK_MAX, at least a quarter of them, both kinds in every 32-channel group; the derivative
    the model uses is the fp32 value of both kernel forms (libm, exp2 / rcp) at the two regime edges."""
    import numpy as np
    for op in ("bnact", "bnbwd"):
        for cid, kw in CASES[op].items():
            if kw["regime"] == "none":
                continue
            c = case(op, cid)
            x = c.x if op == "bnact" else c.z
            v = x.double() * c.ss[0].double() + c.ss[1].double()
            blocked = (v <= N.X.BLOCK_MAX).reshape(-1, c.C)
            assert bool(((v >= N.X.PASS_MIN).reshape(-1, c.C) | blocked).all())
            assert bool((blocked.all(0) | ~blocked.any(0)).all())
            n = int(blocked.all(0).sum())
            assert n == 0 if kw["regime"] == "pass" else 4 * n >= c.C - 3, (cid, n)
    with np.errstate(over="ignore"):
        for t, want in ((np.float32(N.X.PASS_MIN), 1.0), (np.float32(N.X.BLOCK_MAX), 0.0), (np.float32(19.0), 1.0), (np.float32(-129.0), 0.0)):
            s_libm = np.float32(1) / (np.float32(1) + np.exp(-t, dtype=np.float32))
            s_fast = np.float32(1) / (np.float32(1) + np.exp2(np.float32(-1.4426950408889634) * t, dtype=np.float32))
            for s in (s_libm, s_fast):
                assert float(s * (np.float32(1) + t * (np.float32(1) - s))) == want, (t, s)


# ---- the models against torch ------------------------------------------------------------------------------------------------------

def _close(a, b, rel=1e-6):
    return float((a - b).abs().max()) <= rel * float(b.abs().max()) + 1e-30


@pytest.mark.parametrize("cid", [i for i in _small("bnstat") if "one_row" not in i])          # (torch refuses batch statistics over one value per channel: next test)
def test_bnstat_model_against_torch_float64(cid):
    c = case("bnstat", cid)
    x = c.x.reshape(c.M, c.C).double()
    rm = c.run0[0].double().clone() if c.run0 is not None else None
    rv = c.run0[1].double().clone() if c.run0 is not None else None
    y = F.batch_norm(x, rm, rv, c.gamma.double(), c.beta.double(), True, c.mom, c.eps)
    r = c.ref.rows
    assert _close(x * r[0] + r[1], y, 1e-9 if c.family == "exact" else 1e-6)              # (hard family: torch's own one-pass variance cancels)
    assert _close(r[2], x.mean(0), 1e-14) and _close(r[3], 1.0 / torch.sqrt(x.var(0, unbiased=False) + c.eps), 1e-9)
    if rm is not None:
        assert _close(c.ref.run[0], rm, 1e-12) and _close(c.ref.run[1], rv, 1e-9)


def test_one_row_bnstat_reference():
    """M = 1: mean = x, var = 0, istd = 1 / sqrt(eps), the running variance takes var itself (no M / (M - 1))."""
    c = case("bnstat", "hard_f32_one_row_c12")
    x = c.x.reshape(c.C).double()
    assert torch.equal(c.ref.mean, x) and float(c.ref.var.abs().max()) == 0.0
    assert torch.equal(c.ref.rows[3], torch.full((c.C,), 1.0 / c.eps ** 0.5, dtype=torch.float64))
    assert torch.equal(c.ref.run[1], 0.75 * c.run0[1].double())


@pytest.mark.parametrize("cid", _small("bnact"))
def test_bnact_model_against_torch_float64(cid):
    c = case("bnact", cid)
    B, H, W, C = c.shape
    y = F.batch_norm(c.x.double().permute(0, 3, 1, 2), None, None, _gamma_of(c), _beta_of(c), True, N.MOM, N.EPS).permute(0, 2, 3, 1)
    y = y if c.regime == "none" else F.silu(y)
    if c.res is not None:
        y = y * (c.keep.double() if c.keep is not None else torch.ones(B, dtype=torch.float64))[:, None, None, None] + c.res.double()
    assert _close(c.ref.out, y)
    rows = -(-H * W // c.P)
    for p in range(c.P):
        want = y.reshape(B, H * W, C)[:, p * rows:(p + 1) * rows].sum(1)
        assert float((c.ref.sums[:, p] - want).abs().max()) <= 1e-6 * float(y.abs().max()) * rows


def _gamma_of(c):
    return c.ss[0].double() * 2.0                                       # scale = gamma * istd, istd = 0.5


def _beta_of(c):
    return c.ss[1].double() + c.ss[2].double() * c.ss[0].double()       # shift = beta - mean * scale


@pytest.mark.parametrize("cid", _small("bnbwd"))
def test_bnbwd_model_against_torch_autograd_float64(cid):
    c = case("bnbwd", cid)
    B, H, W, C = c.shape
    z = c.z.double().clone().requires_grad_(True)
    gm, bt = _gamma_of(c).clone().requires_grad_(True), _beta_of(c).clone().requires_grad_(True)
    y = F.batch_norm(z.permute(0, 3, 1, 2), None, None, gm, bt, True, N.MOM, N.EPS).permute(0, 2, 3, 1)
    y = y if c.regime == "none" else F.silu(y)
    if c.keep is not None:
        y = y * c.keep.double()[:, None, None, None]
    gin = c.gy.double() if c.ga is None else c.gy.double() * c.ga.double()[:, None, None, :] + c.gb.double()[:, None, None, :]
    y.backward(gin)
    scale = float(gin.abs().max()) * 4
    assert float((c.ref.out.reshape(c.shape) - z.grad).abs().max()) <= 1e-6 * scale
    assert float((c.ref.s1 - bt.grad).abs().max()) <= 1e-6 * scale * c.M and float((c.ref.s2 - gm.grad).abs().max()) <= 1e-6 * scale * c.M


# ---- what the case lists reach ------------------------------------------------------------------------------------------------------

def _coverage():
    """kernel -> path -> fact -> first case that supplies it."""
    table = {}
    for op in CASES:
        for cid in CASES[op]:
            for k in _lay(op, cid):
                row = table.setdefault(k.kernel, {}).setdefault(k.path, {})
                facts = {"runs": True, ">= 2 trips": k.trips >= 2, ">= 2 trips, masked tail": bool(k.multi_masked), "masked tail": bool(k.masked),
                         "empty chunk": bool(k.empty), "empty chunk under the 512 cap": bool(k.empty) and k.nchunk == 512 and k.kernel != "bnbwd_apply_kernel",
                         "cut channel block": getattr(k, "cut_block", False)}
                if op == "bnbwd":
                    c = CASES[op][cid]
                    facts["chunk crosses an image, per-image operands differ"] = bool(k.cross) and c["variant"] in ("keep", "gate")
                if op == "bnstat":
                    facts["16-bit input"] = CASES[op][cid].get("idt", L.F32) != L.F32
                for f, v in facts.items():
                    if v:
                        row.setdefault(f, cid)
    return table


def test_the_case_lists_reach_every_path(capsys):
    t = _coverage()
    with capsys.disabled():
        print("\nexact BatchNorm cases: kernel / path / fact <- first case that supplies it")
        for kern in t:
            for path in sorted(t[kern], key=lambda p: (p == "scalar", -int(p[1:]) if p != "scalar" else 0)):
                for f, cid in t[kern][path].items():
                    print(f"  {kern:26s} {path:7s} {f:52s} <- {cid}")
    every_q = {f"Q{q}" for q in (64, 32, 16, 8, 4, 2, 1)}
    for kern in ("bnstat_partial_q_kernel", "bnact_q_kernel", "bnbwd_partial_kernel", "bnbwd_apply_kernel"):
        assert set(t[kern]) == every_q, (kern, set(t[kern]))
        assert any(">= 2 trips, masked tail" in t[kern][p] for p in t[kern]), kern
    assert all(N.pick_q(C) == q for C, q in N.Q_OF_C.items())
    # BNACT reaches a second, masked trip at EVERY Q (its image sizes are chosen for that); the scalar kernels make many trips
    assert all(">= 2 trips, masked tail" in t["bnact_q_kernel"][p] for p in every_q)
    for kern in ("bnstat_partial_kernel", "bnact_kernel"):
        assert ">= 2 trips, masked tail" in t[kern]["scalar"] and "cut channel block" in t[kern]["scalar"]
    assert "16-bit input" in t["bnstat_partial_kernel"]["scalar"]
    # BNSTAT's scalar kernel on fp32 with C % 4 != 0, and on 16-bit input with a cut channel block
    assert {kw["shape"][3] for kw in CASES["bnstat"].values() if kw.get("idt", L.F32) == L.F32 and kw["shape"][3] % 4} >= {9, 66}
    assert any(kw.get("idt", L.F32) != L.F32 and kw["shape"][3] % 64 for kw in CASES["bnstat"].values())
    # the named multi-trip shapes
    assert ">= 2 trips, masked tail" in t["bnstat_partial_q_kernel"]["Q32"] and "empty chunk under the 512 cap" in t["bnstat_partial_q_kernel"]["Q32"]
    assert ">= 2 trips, masked tail" in t["bnstat_partial_q_kernel"]["Q1"]
    assert ">= 2 trips, masked tail" in t["bnbwd_partial_kernel"]["Q8"] and "empty chunk under the 512 cap" in t["bnbwd_partial_kernel"]["Q8"]
    assert ">= 2 trips, masked tail" in t["bnbwd_apply_kernel"]["Q64"] and "empty chunk" in t["bnbwd_apply_kernel"]["Q64"]
    assert any("empty chunk" in t["bnact_q_kernel"][p] for p in every_q) and "empty chunk" in t["bnact_kernel"]["scalar"]      # P = HW + 5
    for kern in ("bnbwd_partial_kernel", "bnbwd_apply_kernel"):
        assert any("chunk crosses an image, per-image operands differ" in t[kern][p] for p in t[kern]), kern
    a = N.layout("bnbwd", (2, 160, 205, 256))[1]
    assert (a.nchunk, a.rows, a.trips) == (4096, 17, 2) and 1929 in a.cross and 1929 in a.multi_masked and a.empty[0] == 3859
    s = N.layout("bnstat", (2, 5, 3277, 128))[0]
    assert (s.nchunk, s.rows, s.trips, s.empty) == (512, 65, 2, list(range(505, 512)))
    p = N.layout("bnbwd", (2, 128, 257, 96))[0]
    assert (p.nchunk, p.rows, p.trips, p.empty) == (512, 129, 2, [511]) and 255 in p.cross


def test_the_axes_of_the_case_lists():
    """Every value of every axis the GPU module's docstrings name, and the pairs that matter, occur."""
    st = CASES["bnstat"].values()
    assert {(kw.get("idt", L.F32), kw["family"], kw["running"]) for kw in st} >= {(d, f, r) for d in (L.F32, L.BF16, L.F16) for f in ("exact", "hard") for r in (True, False)}
    ac = list(CASES["bnact"].values())
    forms = {(kw["idt"] == L.F32, kw["odt"] == L.F32, kw["tc"]) for kw in ac}
    assert forms == {(i, o, t) for i in (True, False) for o in (True, False) for t in (L.BF16, L.F16)}
    assert all(kw["out2"] for kw in ac if kw["idt"] == L.F32 and kw["odt"] == L.F32)
    for tc in (L.BF16, L.F16):
        sub = [kw for kw in ac if kw["tc"] == tc]
        assert {kw["res"] for kw in sub} == {L.F32, tc, None}
        assert {kw["regime"] for kw in sub} == {"none", "pass", "mixed"}
        assert {(kw["keep"], kw["res"] is not None) for kw in sub} >= {(True, True), (False, True)}
        assert {kw["sums"] for kw in sub} == {True, False}
        assert {("one", "three", "beyond")[(kw["P"] > 1) + (kw["P"] > 3)] for kw in sub} == {"one", "three", "beyond"}
        assert {(kw["res"], kw["idt"] == L.F32, kw["odt"] == L.F32) for kw in sub if kw["res"] == tc} >= {(tc, True, True), (tc, False, False)}
    assert all(kw["P"] in (1, 3, kw["shape"][1] * kw["shape"][2] + 5) and (kw["shape"][1] * kw["shape"][2]) % 3 for kw in ac)
    bw = list(CASES["bnbwd"].values())
    assert {(kw["wd"], kw["zdt"]) for kw in bw} == set(N.BNBWD_TYPES)
    for wd, zdt in N.BNBWD_TYPES:
        sub = [kw for kw in bw if (kw["wd"], kw["zdt"]) == (wd, zdt)]
        assert {kw["outputs"] for kw in sub} == ({"out"} if wd == L.F32 else {"out", "out2", "both"}), (wd, zdt)
        assert {kw["variant"] for kw in sub} == {"plain", "keep", "gate", "slice_accum"}, (wd, zdt)
        assert {kw["regime"] for kw in sub} == {"none", "pass", "mixed"}, (wd, zdt)
    big = [kw for op in CASES for kw in CASES[op].values() if kw["shape"][0] * kw["shape"][1] * kw["shape"][2] > 10000]
    assert len(big) == 4                                                  # one large shape per kernel with an unrolled loop that needs one


def test_accumulate_without_an_fp32_output_is_refused():
    """FTC_FLAG_ACCUM adds onto `out`; with out2 alone the kernel had nothing to add to and silently wrote the plain gradient: the op is refused now."""
    import ctypes as C
    from test_abi_and_plan import _op
    lib, h = L.load(), C.c_void_p()
    op = dict(kind=L.OP_BNBWD, flags=L.FLAG_ACCUM, act=L.ACT_NONE, w_dtype=L.BF16, in_dtype=L.F32, B=2, H=4, W=8, Cin=16, in_=0, in2=4096, scale=8192, out=12288, out2=16384,
              aux=20480)
    assert lib.ftc_plan_create(_op(**op), 1, 1 << 16, 0, C.byref(h)) == 0, lib.ftc_last_error()
    lib.ftc_plan_destroy(h)
    del op["out"]
    assert lib.ftc_plan_create(_op(**op), 1, 1 << 16, 0, C.byref(h)) == -1 and b"FTC_FLAG_ACCUM" in lib.ftc_last_error()
    op["flags"] = 0
    assert lib.ftc_plan_create(_op(**op), 1, 1 << 16, 0, C.byref(h)) == 0, lib.ftc_last_error()
    lib.ftc_plan_destroy(h)
    assert not any(kw["variant"] == "slice_accum" and kw["outputs"] == "out2" for kw in CASES["bnbwd"].values())


# ---- discrimination ---------------------------------------------------------------------------------------------------------------

def _fails(op, c, drop, only=None):
    """The GPU module's check of case c refuses the model with the fault `drop`; only: keep the right answer in every output but that one."""
    good, bad = N.as_kernel_output(op, c, MODEL[op](c)), N.as_kernel_output(op, c, MODEL[op](c, drop))
    CHECK[op](c, *good)
    got = bad if only is None else tuple(b if i == only else g for i, (g, b) in enumerate(zip(good, bad)))
    with pytest.raises(AssertionError):
        CHECK[op](c, *got)
    return True


@pytest.mark.parametrize("cid", ["exact_f32_c256", "exact_f32_c12", "exact_f32_c9", "exact_bf16_c96", "hard_f32_c96", "hard_f16_c96", "exact_f32_two_trips_q32_empty_chunks",
                                 "exact_f32_two_trips_q1"])
def test_bnstat_checks_catch_a_dropped_row_tail_or_chunk(cid):
    c = case("bnstat", cid)
    k = _lay("bnstat", cid)[0]
    last = c.M - 1
    second_trip = k.RL * k.U if k.trips >= 2 else 1                   # the first row of lane 0's second trip in chunk 0
    for rows in ((0, 1), (last, last + 1), (second_trip, second_trip + 1), (k.rows, min(c.M, 2 * k.rows))):
        if rows[0] < rows[1] <= c.M:
            assert _fails("bnstat", c, {"rows": rows}, only=0)
    if c.run0 is not None:
        assert _fails("bnstat", c, {"rows": (0, 1)}, only=1)


@pytest.mark.parametrize("cid", ["hard_f32_c96", "hard_f32_c12", "hard_f32_c9", "hard_f16_c96"])
def test_bnstat_checks_catch_an_fp32_accumulation(cid):
    """... which passes the 2e-6 max-norm bound of the tolerance test on Gaussian data: here the variance is wrong in its leading digits."""
    c = case("bnstat", cid)
    assert _fails("bnstat", c, {"fp32": True}, only=0)


@pytest.mark.parametrize("cid", [i for i, kw in CASES["bnact"].items() if kw["shape"][3] in (256, 12, 9)])
def test_bnact_checks_catch_a_dropped_row_and_a_stale_keep(cid):
    c = case("bnact", cid)
    HW = c.shape[1] * c.shape[2]
    assert not bool((c.ref.out == 0).all())
    for rows in ((0, 1), (HW - 1, HW)):
        assert _fails("bnact", c, {"rows": rows}, only=0)
        if c.has_out2:
            assert _fails("bnact", c, {"rows": rows}, only=1)
        if c.want_sums:
            assert _fails("bnact", c, {"rows": rows}, only=2)
    if c.keep is not None:
        for b in range(1, c.shape[0]):
            assert float(c.keep[b]) != float(c.keep[b - 1])
            assert _fails("bnact", c, {"image": b}, only=0)


@pytest.mark.parametrize("cid", [i for i, kw in CASES["bnbwd"].items() if kw["shape"][3] in (256, 96, 12) and kw["shape"][0] * kw["shape"][1] * kw["shape"][2] <= 10000]
                         + ["partial_two_trips_q8"])
def test_bnbwd_checks_catch_a_dropped_row_chunk_and_a_missed_reload(cid):
    """A row left out of the partial sums shows in gbeta, ggamma and coef (per channel, bitwise) and, through coef, in out; stale keep / ga / gb of the
    previous image shows in all of them -- under the ragged-M bound too."""
    c = case("bnbwd", cid)
    part, _ = _lay("bnbwd", cid)
    last = c.M - 1
    rows_list = [(0, 1), (last, last + 1)] + ([(part.rows, min(c.M, 2 * part.rows))] if part.nchunk > 1 else [])
    if part.trips >= 2:
        rows_list.append((part.RL * part.U, part.RL * part.U + 1))
    for rows in rows_list:
        touched = bool((c.ref.dt[rows[0]:rows[1]] != 0).any())
        if not touched:                                                 # (keep = 0 or a blocked channel everywhere in those rows: nothing to lose)
            continue
        for only in (0, 1, 2):                                          # gbeta, ggamma, coef
            assert _fails("bnbwd", c, {"rows": rows}, only=only)
        out_i = 3 if c.outputs != "out2" else 4
        assert _fails("bnbwd", c, {"rows": rows}, only=out_i)
    if c.variant in ("keep", "gate"):
        for b in range(1, c.shape[0]):
            assert _fails("bnbwd", c, {"image": b})
            assert _fails("bnbwd", c, {"image": b}, only=3 if c.outputs != "out2" else 4)


# ---- the resolvers of csrc/train_choice.h against the launch arithmetic restated in bn_operands.layout ------------------------------------------------

@pytest.fixture(scope="module")
def train_choice_host(tmp_path_factory):
    import train_choice_host as H
    return H.build(tmp_path_factory.mktemp("train_choice"))


def _grid_x(k, C):
    """layout(): the Q kernels run on grid (C / 4Q, chunks ...), the scalar kernels on ((C + 63) / 64, chunks ...)."""
    return (C + 63) // 64 if k.path == "scalar" else C // (4 * k.Q)


def _bn_agrees(op, shape, lay, got, meta):
    why, _, inst, launch = got
    B, H, W, C = shape
    assert why == "", (meta, why)
    k = lay[0]
    assert inst.get("family", "q") == ("scalar" if k.path == "scalar" else "q") and inst["Q"] == (k.Q or 0), (meta, inst)
    if op == "bnstat":
        assert (launch["M"], launch["nchunk"], launch["grid"], launch["final"]) == (B * H * W, k.nchunk, (_grid_x(k, C), k.nchunk), (C + 15) // 16), (meta, launch)
    elif op == "bnact":
        assert (launch["P"], launch["grid"]) == (k.nchunk, (_grid_x(k, C), k.nchunk, B)), (meta, launch)
    else:
        a = lay[1]
        assert (k.Q, k.RL) == (a.Q, a.RL)
        assert (launch["M"], launch["nchunk"], launch["ach"]) == (B * H * W, k.nchunk, a.nchunk), (meta, launch)
        assert (launch["partial"], launch["final"], launch["apply"]) == ((_grid_x(k, C), k.nchunk), (C + 15) // 16, (_grid_x(a, C), a.nchunk)), (meta, launch)


def _bn_op(op, kw):
    import train_choice_host as H
    if op == "bnstat":
        return H.bnstat(kw["shape"], kw.get("idt", L.F32))
    if op == "bnact":
        return H.bnact(kw["shape"], kw["idt"], kw["odt"], kw["tc"], kw["P"], kw["res"], kw["out2"])
    return H.bnbwd(kw["shape"], kw["wd"], kw["zdt"], kw["outputs"], kw["variant"] == "slice_accum")


@pytest.mark.parametrize("op", ["bnstat", "bnact", "bnbwd"])
def test_resolver_equals_layout_on_every_gpu_case(op, train_choice_host):
    """Every case of the three GPU case lists: the family, Q, chunk counts and grids the launcher takes from the resolver are layout()'s, the type arguments
    are the case's, and the label is the one the op always had."""
    got = train_choice_host([_bn_op(op, kw) for kw in CASES[op].values()])
    for (cid, kw), g in zip(CASES[op].items(), got):
        _bn_agrees(op, kw["shape"], _lay(op, cid), g, cid)
        inst, launch = g[2], g[3]
        if op == "bnstat":
            assert inst["T"] == N.DT_NAME[kw.get("idt", L.F32)] and g[1] == f"bnstat_partial+final<{inst['T']}>", (cid, g)
        elif op == "bnact":
            assert (inst["TI"], inst["TO"], inst["TC"]) == tuple(N.DT_NAME[kw[t]] for t in ("idt", "odt", "tc")) and launch["res"] == int(kw["res"] is not None), (cid, g)
            assert g[1] == f"bnact_kernel<{inst['TI']},{inst['TO']}>", (cid, g)
        else:
            assert (inst["fast"], inst["TC"], inst["ZT"]) == (int(kw["wd"] != L.F32), N.DT_NAME[kw["wd"]], N.DT_NAME[kw["zdt"]]), (cid, g)
            assert launch["accum"] == int(kw["variant"] == "slice_accum") and g[1] == "bnbwd_partial+final+apply", (cid, g)
    assert {g[2]["Q"] for g in got} >= {64, 32, 16, 8, 4, 2, 1}


# B H W of the sweeps.  M = 1 and 7: the apply pass of BNBWD has one chunk (M / 8 + 1 = 1); 130 and 135: 17 chunks, the clamp, at every width but those whose
# 16384 Q / C is 15 or 16; 8192: M / 8 + 1 = 1025 bounds the wide layouts only.  The BNACT sweep takes H W of each as the rows of one image.
_BN_SHAPES = [(1, 1, 1), (1, 1, 7), (2, 5, 13), (3, 5, 9), (2, 64, 64)]
_DTS = (L.F32, L.BF16, L.F16)


def test_bnstat_resolver_equals_layout_over_every_width_and_type(train_choice_host):
    """C = 1 .. 1056 x the shapes x the three input types: the Q kernel exactly for fp32 input with C % 4 == 0, the scalar kernel otherwise."""
    keys = [(shape + (C,), dt) for C in range(1, 1057) for shape in _BN_SHAPES for dt in _DTS]
    for (shape, dt), g in zip(keys, train_choice_host([_bn_op("bnstat", dict(shape=shape, idt=dt)) for shape, dt in keys])):
        _bn_agrees("bnstat", shape, N.layout("bnstat", shape, dt), g, (shape, dt))
        assert (g[2]["family"] == "q") == (dt == L.F32 and shape[3] % 4 == 0) and g[2]["T"] == N.DT_NAME[dt]
    # 512 chunks at the most (layout() on the two large shapes of the case list is part of the test above); 2^31 - 1 rows and more: the scalar kernel, whose
    # row index is 64 bits wide (launch_bnstat: `o.in_dtype == FTC_F32 && C % 4 == 0 && M < 0x7fffffffL`)
    (_, _, inst, launch), (_, _, inst1, _) = train_choice_host([_bn_op("bnstat", dict(shape=(2, 32768, 32768, 8))), _bn_op("bnstat", dict(shape=(2, 32768, 32767, 8)))])
    assert (inst["family"], inst["Q"], launch["M"], launch["nchunk"], launch["grid"]) == ("scalar", 0, 2 ** 31, 512, (1, 512)) and (inst1["family"], inst1["Q"]) == ("q", 2)
    bad = train_choice_host([_bn_op("bnstat", dict(shape=(1, 1, 1, 0))), _bn_op("bnstat", dict(shape=(1, 1, 1, 8), idt=7)), _bn_op("bnstat", dict(shape=(0, 1, 1, 8)))])
    assert [g[0] for g in bad] == ["bnstat: Cin must be positive", "bnstat: unknown dtype", "B/H/W must be positive"]


def test_bnact_resolver_equals_layout_over_every_width_and_type(train_choice_host):
    """C = 1 .. 1056 x the shapes x P in {0 (= 1), 1, 3, H W + 5} x the plan's three storage forms (fp32 in and out, the 16-bit type in and out, 16-bit in and
    fp32 out): the Q kernel exactly for C % 4 == 0, whatever the types; FTC_BNACT_SCALAR: the scalar kernel at every width."""
    forms = [(L.F32, L.F32, L.BF16), (L.BF16, L.BF16, L.BF16), (L.F16, L.F32, L.F16)]
    keys = [((4,) + shape[1:] + (C,), P, f) for C in range(1, 1057) for shape in _BN_SHAPES[1:4] for P in (0, 1, 3, shape[1] * shape[2] + 5) for f in forms]
    ops = [_bn_op("bnact", dict(shape=shape, idt=f[0], odt=f[1], tc=f[2], P=P, res=None, out2=False)) for shape, P, f in keys]
    for (shape, P, f), g in zip(keys, train_choice_host(ops)):
        _bn_agrees("bnact", shape, N.layout("bnact", shape, f[0], P), g, (shape, P, f))
        assert (g[2]["family"] == "q") == (shape[3] % 4 == 0) and (g[2]["TI"], g[2]["TO"], g[2]["TC"]) == tuple(N.DT_NAME[t] for t in f)
    for value, fam in (("1", "scalar"), ("0", "q"), ("", "q")):
        sw = train_choice_host(ops[:600], env={"FTC_BNACT_SCALAR": value})
        assert all(g[0] == "" and g[2]["family"] == ("q" if fam == "q" and k[0][3] % 4 == 0 else "scalar") and g[3]["grid"][0] == (k[0][3] // (4 * g[2]["Q"]) if g[2]["Q"] else (k[0][3] + 63) // 64)
                   for k, g in zip(keys, sw)), value


def test_bnbwd_resolver_equals_layout_over_every_width_and_type(train_choice_host):
    """C = 1 .. 1056 x the shapes x (w_dtype, z type) in (fp32, fp32), (bf16, bf16), (fp16, fp32): widths that are no multiple of 4 are refused with plan
    creation's message; the apply pass has one chunk, M / 8 + 1 chunks under the clamp, and 16384 Q / C chunks where the clamp does not bind."""
    forms = [(L.F32, L.F32), (L.BF16, L.BF16), (L.F16, L.F32)]
    keys = [(shape + (C,), f) for C in range(1, 1057) for shape in _BN_SHAPES for f in forms]
    got = train_choice_host([_bn_op("bnbwd", dict(shape=shape, wd=f[0], zdt=f[1], outputs="out" if f[0] == L.F32 else "both", variant="plain")) for shape, f in keys])
    one = clamped = free = 0
    for (shape, f), g in zip(keys, got):
        if shape[3] % 4:
            assert g[0] == "bnbwd: Cin must be a positive multiple of 4", (shape, g)
            continue
        lay = N.layout("bnbwd", shape)
        _bn_agrees("bnbwd", shape, lay, g, (shape, f))
        assert (g[2]["fast"], g[2]["TC"], g[2]["ZT"]) == (int(f[0] != L.F32), N.DT_NAME[f[0]], N.DT_NAME[f[1]])
        M, raw, ach = shape[0] * shape[1] * shape[2], (4096 * 4 * lay[1].Q) // shape[3], g[3]["ach"]
        one += ach == 1
        clamped += 1 < ach == M // 8 + 1 < raw
        free += 1 < ach == raw < M // 8 + 1
    assert one and clamped and free, (one, clamped, free)
