"""CPU checks of tests/exact_operands.py: every case the -m gpu exact-operand modules launch passes assert_exact_case (the builders call
it), its float64 reference equals plain fp32 PyTorch bit for bit (so the order of summation really does not matter), and references with
one term misplaced differ from the true one -- what the bitwise comparison on the GPU is able to see."""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import test_gpu_exact_bwd as EB
import test_gpu_exact_conv as EC
from findtextcenternet_amd import _lib as L
from test_gpu_bwd_ops import WG_CASES
from test_gpu_conv_fuzz import _case, _case_f32
from test_gpu_ops import CONV_CASES, CONV_MODES, HALO_CASES, SPLITK_CASES


def _fp32_conv(c):
    """The same convolution in plain fp32 (one summation order among many)."""
    xin = c.xin.permute(0, 3, 1, 2)
    if c.w.dim() == 5:
        z = torch.cat([F.conv2d(xin[b:b + 1], c.w[b], None, c.stride, c.pad) for b in range(c.B)])
    else:
        z = F.conv2d(xin, c.w, None, c.stride, c.pad)
    z = z.permute(0, 2, 3, 1) + c.bias
    return z + c.res if c.res is not None else z


def _check_conv(c):
    X.assert_bits_equal(_fp32_conv(c).contiguous(), c.z.float(), "fp32 F.conv2d against the float64 reference")
    assert torch.equal(c.want.double(), c.z) or c.odt != L.F32


_TABLE = [(c, m) for c in CONV_CASES for m in CONV_MODES if EC._mode_ok(c, m)] + \
         [(c, m) for c in HALO_CASES[-2:] + SPLITK_CASES for m in CONV_MODES if m[0] in ("f32", "bf16", "bf16_f32out", "f16", "f16_f32out", "f32x3")]


@pytest.mark.parametrize("case,mode", _TABLE, ids=[f"{c[0]}-{m[0]}" for c, m in _TABLE])
def test_table_cases_are_exact_and_order_free(case, mode):
    _check_conv(X.table_case(case, mode))


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_cases_are_exact_and_order_free(seed):
    d = _case(9000 + seed)
    _check_conv(X.fuzz_case(d))
    if d["wdt"] == L.BF16:
        _check_conv(X.fuzz_case(d, f16=True))
    if seed < 10:
        _check_conv(X.fuzz_case(_case_f32(7000 + seed), x3=True))


def test_px144_c32_and_epilogue_cases_are_exact_and_order_free():
    for shape in EC._PX_SHAPES:
        for variant in ("plain", "res_copy", "res_kblock", "per_image", "slices"):
            for dt in (L.BF16, L.F16):
                _check_conv(X.px144_case(shape, dt, variant, False))
            if variant in ("plain", "res_copy", "per_image"):
                _check_conv(X.px144_case(shape, L.F32, variant, True))
    for shape in [(2, 32, 48), (1, 21, 19), (1, 7, 50)]:
        for dt in (L.BF16, L.F16, 3):
            _check_conv(X.c32_case(shape, dt))
    _check_conv(X.dual_output_case())
    for dt in (L.F32, L.BF16):
        c = X.border_bias_case(dt)
        ring = X.border_index(c.H, c.W)
        assert sorted(set(ring.flatten().tolist())) == [0, 1, 2, 4, 5, 6, 8, 9, 10]          # interior, four edges, four corners
    for args in [(3, 2, 20, 12, 64, 192, 41), (3, 2, 20, 12, 64, 2, 41), (1, 2, 20, 12, 64, 1, 72), (6, 1, 33, 17, 192, 1, 200), (3, 2, 16, 48, 32, 2, 41), (1, 1, 40, 24, 96, 4, 107)]:
        c = X.grouped_case(*args)
        for i in range(args[0]):
            z32 = F.conv2d(c.x[i].permute(0, 3, 1, 2), c.w[i], c.bias[i], 1, 1).permute(0, 2, 3, 1).contiguous()
            X.assert_bits_equal(z32, c.z[i].float(), "grouped conv in fp32")
    for shape in [(2, 32, 48), (1, 21, 19)]:
        for mode in ("bf16", "f32", "f32x3"):
            X.top_fuse_case(shape, mode)
    for shape in [(1, 21, 13, 72, 1), (1, 21, 13, 72, 2), (2, 48, 48, 128, 2)]:
        for dt in (L.F32, L.BF16, L.F16):
            c = X.depthwise_case(*shape, dt, seed=11)
            z32 = F.conv2d(c.x.permute(0, 3, 1, 2), c.w, c.bias, shape[4], 1, 1, shape[3]).permute(0, 2, 3, 1).contiguous()
            X.assert_bits_equal(z32, c.z.float(), "depthwise conv in fp32")


@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_cases_are_exact_and_order_free(case):
    for wd, io in EB._WG_CFG:
        c = X.wgrad_case(case, wd, io)
        w = torch.zeros(c.Cout, c.Cin, c.k, c.k, requires_grad=True)
        F.conv2d(c.xe.permute(0, 3, 1, 2), w, None, c.stride, c.pad).backward(c.dz.permute(0, 3, 1, 2).contiguous())
        X.assert_bits_equal(w.grad + c.pre, c.want, f"fp32 autograd weight gradient {case[0]}")


def test_other_backward_cases_are_exact():
    for _, shape, stride in X.DWBWD_CASES:
        c = X.dwbwd_case(*shape, stride, seed=shape[3] + stride)
        xx, ww = c.x.clone().requires_grad_(True), c.w.clone().requires_grad_(True)
        F.conv2d(xx.permute(0, 3, 1, 2), ww, None, stride, 1, 1, shape[3]).backward(c.dz.permute(0, 3, 1, 2))
        X.assert_bits_equal(xx.grad, c.want_dx, "fp32 autograd depthwise data gradient")
        X.assert_bits_equal(ww.grad + c.pre, c.want_dw, "fp32 autograd depthwise weight gradient")
    for co, off in [(1, 0), (2, 1), (1, 8)]:
        X.topdgrad_colsum_case(co, off, seed=co + off)
    for C0 in (32, 24):
        X.stemwgrad_case(C0, seed=C0)
    for (B, H, W, Cin, Cout, _), wd in [((2, 16, 16, 32, 128, 3), L.F32), ((1, 12, 20, 64, 256, 3), L.BF16)]:
        c = X.stride2_dgrad_case(B, H, W, Cin, Cout, wd, seed=Cin)
        x = torch.zeros(B, Cin, H, W, requires_grad=True)
        F.conv2d(x, c.w, None, 2, 1).backward(c.dz.permute(0, 3, 1, 2))
        X.assert_bits_equal(x.grad.permute(0, 2, 3, 1).contiguous(), c.want, "fp32 autograd stride-2 data gradient")


def test_assert_exact_case_refuses_inexact_operands():
    g = X.gen(1)
    x, w = X.acts((1, 4, 4, 8), g), X.weights((8, 8, 1, 1), 3, g)
    X.assert_exact_case([x, w], 8, [], [(x, L.BF16), (w, L.F16)])
    with pytest.raises(AssertionError):
        X.assert_exact_case([x, w], 2 ** 21, [])                                   # sum |terms| * 2^s reaches 2^23
    with pytest.raises(AssertionError):
        X.assert_exact_case([x, w + 2.0 ** -12], 8, [], [(w + 2.0 ** -12, L.BF16)])        # 1/8 + 2^-12 needs ten bits
    with pytest.raises(AssertionError):
        X.assert_exact_case([x, torch.full((1,), 1 / 3)], 8)                           # not dyadic
    with pytest.raises(AssertionError):
        X.assert_exact_case([x * 16384, w * 16], 8, [], [], L.F16, torch.full((1,), 70000.0, dtype=torch.float64))
    a = torch.zeros(2, 5, 6, 40)
    b = a.clone()
    b[1, 4, 0, 33] = 0.25
    with pytest.raises(AssertionError) as e:
        X.assert_bits_equal(b, a, "report")
    msg = str(e.value)
    assert "1 of 2400" in msg and "(b=1, y=4, x=0, ch=33)" in msg and "border row True, border col True" in msg and "ch%32 1" in msg
    assert "in image 24/24/24/24" in msg and "over batch 22/54/54/54" in msg
    X.assert_bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))


# ---- sensitivity: a reference with one term misplaced differs from the true one ---------------------------------------------------

_SENS = {"sliced_3x3": (next(c for c in CONV_CASES if c[0] == "fpn_slice_in"), CONV_MODES[1]),
         "stride2_3x3": (next(c for c in CONV_CASES if c[0] == "odd_hw_s2"), CONV_MODES[0]),
         "pw_se": (next(c for c in CONV_CASES if c[0] == "pw_project_se_res"), CONV_MODES[1])}


def _ref(c, x=None, w=None, cin_off=None):
    """The reference of case c with some operands replaced; x is the (SE-scaled) input slice."""
    if cin_off is not None:
        x = c.x_full[..., cin_off:cin_off + c.Cin]
        x = x * c.sc[:, None, None, :] if c.sc is not None else x
    x = c.xin if x is None else x
    w = c.w if w is None else w
    z = X.conv_ref64(x, w, c.stride, c.pad) + c.bias.double()
    return z + c.res.double() if c.res is not None else z


@pytest.mark.parametrize("name", list(_SENS))
def test_mutated_references_differ(name):
    c = X.table_case(*_SENS[name])
    assert torch.equal(_ref(c), c.z)
    # 1. one tap dropped at one border pixel: output pixel (0, 0, Wo-1) loses the term of its centre tap for input channel 0
    y_in, x_in = 0, (c.Wo - 1) * c.stride
    z = c.z.clone()
    z[0, 0, c.Wo - 1] -= c.xin[0, y_in, x_in, 0].double() * c.w[:, 0, c.k // 2, c.k // 2].double()
    assert int((z != c.z).sum()) >= 1 and int((z != c.z).sum()) <= c.Cout
    # 2. cin_off moved by one unit (eight channels: the 16-byte chunk of a 16-bit tensor)
    wide = c if c.CinT > c.Cin else None
    if wide is None:                                    # cases that read the whole tensor: the same operands inside a wider buffer
        g = X.gen(3)
        wide = X.SimpleNamespace(**vars(c))
        wide.x_full = torch.cat([X.acts((c.B, c.H, c.W, 8), g), c.x_full, X.acts((c.B, c.H, c.W, 8), g)], -1)
        wide.cin_off = 8
        assert torch.equal(_ref(wide, cin_off=8), c.z)
    assert int((_ref(wide, cin_off=wide.cin_off - 8) != c.z).sum()) >= 1
    # 3. the last K block (32 channels of the last tap) omitted
    w = c.w.clone()
    w[:, -32:, -1, -1] = 0
    assert int((_ref(c, w=w) != c.z).sum()) >= 1
    # 4. one in-image value used where padding belongs: the output at (0, 0) reads x[0, 0] once more, through the tap that lies outside the image
    if c.k == 3:
        z = c.z.clone()
        z[0, 0, 0] += c.xin[0, 0, 0, 0].double() * c.w[:, 0, 0, 0].double()
    else:                                                # 1x1: no padding; the neighbouring pixel's value in its place
        x = c.xin.clone()
        j = int(torch.nonzero(x[0, 0, :, 0] != x[0, 0, 0, 0])[0])
        x[0, 0, 0, 0] = x[0, 0, j, 0]
        z = _ref(c, x=x)
    assert int((z != c.z).sum()) >= 1


# ---- FTC_OP_DWBWD: the resolver of csrc/train_choice.h against launch_dwbwd restated (exact_operands.dwbwd_layout) -------------------------------------

@pytest.fixture(scope="module")
def train_choice_host(tmp_path_factory):
    import train_choice_host as H
    return H.build(tmp_path_factory.mktemp("train_choice"))


def _dwbwd_agrees(shape, stride, halves, got):
    why, lab, inst, launch = got
    lay = X.dwbwd_layout(*shape, stride, data=halves != "weight", weight=halves != "data")
    assert why == "" and lab == f"dwbwd_data+weight<s{stride}>", (shape, stride, halves, why, lab)
    d, w = lay.data, lay.weight
    assert inst["data"] == ("-" if d is None else "q" if d.kernel == "dwbwd_data_q_kernel" else "general") and inst["weight"] == ("-" if w is None else "q"), (shape, inst)
    assert (inst["Q"], launch["want"], launch["grid"]) == ((d.Q, d.want, d.grid) if d else (0, 0, (0, 0))), (shape, stride, halves, inst, launch)
    assert (inst["wQ"], launch["nchunk"], launch["wgrid"], launch["wfinal"]) == ((w.Q, w.nchunk, w.grid, w.final_grid) if w else (0, 0, (0, 0), 0)), (shape, stride, halves, inst, launch)
    return lay


def test_dwbwd_gpu_cases_reach_every_lane_layout_of_both_passes(train_choice_host):
    import train_choice_host as H
    ops = [H.dwbwd(shape, stride) for _, shape, stride in X.DWBWD_CASES]
    lays = [_dwbwd_agrees(shape, stride, "both", got) for (_, shape, stride), got in zip(X.DWBWD_CASES, train_choice_host(ops))]
    assert {k.data.Q for k in lays} == {64, 32, 16, 8, 4, 2, 1} and {k.weight.Q for k in lays} == {16, 8, 4, 2, 1}
    by_id = {cid: k for (cid, _, _), k in zip(X.DWBWD_CASES, lays)}
    assert [(by_id[i].data.Q, by_id[i].weight.Q) for i in ("5x5x4_s1", "5x5x16_s2", "6x5x64_s1", "5x5x256_s2")] == [(1, 1), (4, 4), (16, 16), (64, 16)]
    assert all(k.data.kernel == "dwbwd_data_q_kernel" for k in lays)


# B H W of the sweep: the row-chunk clamp Mi / (4 RL) + 1 of the data pass is active at every Q on the first (Mi = 25), at the wider Q only on the next two, and
# inactive at every Q on the last; the weight pass has 1, 1, 12 | 27 and 257 | 65 chunks (stride 1 | 2)
_DW_SHAPES = [(1, 5, 5), (2, 12, 10), (3, 48, 48), (2, 160, 205)]


def test_dwbwd_resolver_equals_the_restated_launcher_over_every_width(train_choice_host):
    """Every C from 1 to 1056 x the shapes above x stride 1 | 2 x (both halves, data alone, weight alone): widths that are no multiple of 4 are refused with
    plan creation's message, every other op resolves to the kernel, Q, row chunks and grids launch_dwbwd took."""
    import train_choice_host as H
    keys = [(shape + (Cc,), stride, halves) for Cc in range(1, 1057) for shape in _DW_SHAPES for stride in (1, 2) for halves in ("both", "data", "weight")]
    got = train_choice_host([H.dwbwd(shape, stride, halves) for shape, stride, halves in keys])
    clamped = free = low = 0
    for (shape, stride, halves), g in zip(keys, got):
        if shape[3] % 4:
            assert g[0] == "dwbwd: Cin % 4 == 0, stride 1 | 2", (shape, g)
            continue
        lay = _dwbwd_agrees(shape, stride, halves, g)
        if lay.data:
            raw, most = (2048 * 4 * lay.data.Q) // shape[3], shape[0] * shape[1] * shape[2] // (4 * (256 // lay.data.Q)) + 1
            clamped += lay.data.want == most < raw
            free += 1 < lay.data.want == raw < most
            low += lay.data.want == 1
    assert clamped and free and low, (clamped, free, low)          # the upper clamp active, inactive, and a single chunk
    none = train_choice_host([dict(H.dwbwd((1, 5, 5, 8), 1), _refs=("in2",)), dict(H.dwbwd((1, 5, 5, 8), 1), stride=3), dict(H.dwbwd((1, 5, 5, 8), 2), Ho=5)])
    assert [g[0] for g in none] == ["dwbwd: neither out (data gradient) nor out2 (weight gradient)", "dwbwd: Cin % 4 == 0, stride 1 | 2", "dwbwd: Ho/Wo inconsistent"]


def test_dwbwd_general_kernel_from_2_31_input_pixels_and_under_the_switch(train_choice_host):
    """B H W >= 2^31 - 1: the data pass runs dwbwd_data_kernel on 16384 workgroups; one pixel row less: the Q kernel.  FTC_DWBWD_DATA_OLD: the general
    kernel at any size; "0" and empty leave the default."""
    import train_choice_host as H
    big, under = (2, 32768, 32768), (1, 32768, 65535)
    assert big[0] * big[1] * big[2] == 2 ** 31 and under[0] * under[1] * under[2] < 2 ** 31 - 1
    keys = [(shape + (Cc,), stride, "both") for shape in (big, under) for Cc in (4, 24, 96, 256, 1056) for stride in (1, 2)] + [(big[:2] + (32768 - 1, 8), 1, "data")]
    lays = [_dwbwd_agrees(*k, g) for k, g in zip(keys, train_choice_host([H.dwbwd(*k) for k in keys]))]
    assert all((k.data.kernel, k.data.grid) == ("dwbwd_data_kernel", (16384, 1)) for key, k in zip(keys, lays) if key[0][:3] == big)
    assert all(k.data.kernel == "dwbwd_data_q_kernel" for key, k in zip(keys, lays) if key[0][:3] != big)
    small = H.dwbwd((1, 5, 5, 8), 1)
    for value, want in (("1", "general"), ("yes", "general"), ("0", "q"), ("", "q")):
        (why, _, inst, launch), = train_choice_host([small], env={"FTC_DWBWD_DATA_OLD": value})
        assert why == "" and inst["data"] == want and (want == "q" or launch["grid"] == (1, 1)), (value, inst, launch)
