"""CPU (no GPU): the C-ABI library loads and exports every symbol include/ftc.h declares, plan
validation works through ftc_plan_create, and the host-side plan / weight-packing logic is sound."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from findtextcenternet_amd import _lib as L
from findtextcenternet_amd.model import FtcModel
from findtextcenternet_amd import tuning
from findtextcenternet_amd.weights import deterministic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "ftc.h")).read()
    declared = sorted(set(re.findall(r"\b(ftc_[a-z_0-9]+)\s*\(", hdr)))
    assert set(declared) == set(L.EXPORTS), (declared, L.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.ftc_abi_version() == L.FTC_ABI_VERSION
    assert C.sizeof(L.Op) == 24 * 4 + 11 * 16 and C.sizeof(L.Ref) == 16 and C.sizeof(L.Tile) == 32
    assert C.sizeof(L.Tensor) == 56 and C.sizeof(L.PlanInfo) == 48 and C.sizeof(L.OpInfo) == 96


def test_device_info_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = L.load()
    n = C.c_int()
    buf = C.create_string_buffer(64)
    assert lib.ftc_device_info(C.byref(n), buf, 64) == -3           # FTC_ERR_NO_DEVICE
    assert b"device" in lib.ftc_last_error().lower() or b"hip" in lib.ftc_last_error().lower()


def _op(**f):
    op = (L.Op * 1)()
    for k, v in f.items():
        if k in ("in_", "in2", "out", "w", "w2", "bias", "bias2", "scale", "shift", "aux", "out2"):
            r = getattr(op[0], k)
            r.base, r.offset = L.BASE_WORKSPACE, v
        else:
            setattr(op[0], k, v)
    return op


def test_plan_create_validates_ops():
    lib = L.load()
    h = C.c_void_p()
    good = dict(kind=L.OP_CONV, in_dtype=L.F32, out_dtype=L.F32, w_dtype=L.F32, B=1, H=8, W=8, Ho=8, Wo=8, Cin=32, Cin_total=32,
                Cout=64, Cout_total=64, ksize=3, stride=1, in_=0, out=65536, w=131072, bias=262144)
    assert lib.ftc_plan_create(_op(**good), 1, 1 << 20, 0, C.byref(h)) == 0
    assert lib.ftc_plan_num_ops(h) == 1
    lib.ftc_plan_destroy(h)
    for bad, msg in [(dict(good, Cin=30), b"Cin"), (dict(good, Ho=7), b"Ho/Wo"), (dict(good, ksize=5), b"ksize"),
                     (dict(good, in_=8), b"16-byte"), (dict(good, out=1 << 21), b"out of range"),
                     (dict(good, kind=99), b"unknown op"), (dict(good, flags=L.FLAG_RESIDUAL), b"in2")]:
        assert lib.ftc_plan_create(_op(**bad), 1, 1 << 20, 0, C.byref(h)) == -1
        assert msg in lib.ftc_last_error(), (msg, lib.ftc_last_error())
    # operand EXTENTS are checked, not just start offsets: an output that starts inside the workspace but runs past its end,
    # a weight matrix larger than the blob, a fused top convolution without its tap matrix
    ws = 1 << 20
    out_bytes = 1 * 8 * 8 * 64 * 4
    assert lib.ftc_plan_create(_op(**dict(good, out=ws - out_bytes)), 1, ws, 0, C.byref(h)) == 0
    lib.ftc_plan_destroy(h)
    assert lib.ftc_plan_create(_op(**dict(good, out=ws - out_bytes + 16)), 1, ws, 0, C.byref(h)) == -1 and b"offset + extent" in lib.ftc_last_error()
    wop = _op(**good)
    wop[0].w.base, wop[0].w.offset = L.BASE_WEIGHTS, 0
    assert lib.ftc_plan_create(wop, 1, ws, 64 * 9 * 32 * 4, C.byref(h)) == 0
    lib.ftc_plan_destroy(h)
    assert lib.ftc_plan_create(wop, 1, ws, 64 * 9 * 32 * 4 - 16, C.byref(h)) == -1 and b"weights operand out of range" in lib.ftc_last_error()
    top = dict(kind=L.OP_CONV, flags=L.FLAG_TOP_FUSE, act=L.ACT_GELU, in_dtype=L.BF16, out_dtype=L.BF16, w_dtype=L.BF16, B=1, H=16, W=16, Ho=16, Wo=16,
               Cin=256, Cin_total=256, Cout=192, Cout_total=192, ksize=3, stride=1, aux0=65, aux1=12, in_=0, out=1 << 19, w=0, bias=0)
    assert lib.ftc_plan_create(_op(**top), 1, 1 << 21, 0, C.byref(h)) == -1 and b"w2" in lib.ftc_last_error()
    dw = dict(kind=L.OP_DWCONV, act=L.ACT_SILU, in_dtype=L.BF16, out_dtype=L.BF16, B=1, H=8, W=8, Ho=8, Wo=8, Cin=64, Cout=64, ksize=3, stride=1, aux0=1,
              in_=0, out=8192, w=16384, bias=32768, aux=ws - 64 * 4 + 16)
    assert lib.ftc_plan_create(_op(**dw), 1, ws, 0, C.byref(h)) == -1 and b"aux" in lib.ftc_last_error()
    # running without a device / with NULL bases is an error, not a crash
    assert lib.ftc_plan_create(_op(**good), 1, 1 << 20, 0, C.byref(h)) == 0
    bases = (C.c_void_p * L.NUM_BASES)()
    assert lib.ftc_plan_run(h, bases, None, 0, -1) == -1 and b"NULL" in lib.ftc_last_error()
    lib.ftc_plan_destroy(h)


@pytest.fixture(scope="module")
def sd():
    return deterministic_state_dict(0, prefix_detector=False)


@pytest.fixture(scope="module")
def models(sd):
    """Library-side models (ftc_create: host-only, works without a GPU) of the seeded checkpoint, one per numeric mode."""
    return {mode: FtcModel(sd, mode) for mode in ("fp32", "bf16")}


def _blob(model, name, dtype, shape):
    off = model.offset(name)
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return model.weights_host()[off:off + n].view(dtype).reshape(shape).copy()


def test_create_rejects_bad_checkpoints(sd):
    bad = dict(sd)
    del bad["keyheatmap.top_conv.0.bias"]
    with pytest.raises(L.FtcError, match="keyheatmap.top_conv.0.bias"):
        FtcModel(bad, "fp32")
    bad = dict(sd)
    bad["backbone.features.4.0.block.2.fc1.weight"] = torch.zeros(24, 383, 1, 1)
    with pytest.raises(L.FtcError, match="shape"):
        FtcModel(bad, "bf16")
    with pytest.raises(L.FtcError, match="model_size"):
        FtcModel(sd, "fp32", "xxl")
    m = FtcModel(sd, "bf16")
    with pytest.raises(L.FtcError, match="multiples of 32"):
        m.plan(1, 100, 768)
    # TextDetectorModel keys (detector.* + decoder.*) are accepted as they come out of model.pt
    full = deterministic_state_dict(0)
    mf = FtcModel(full, "bf16")
    lib = L.load()
    # ... and then the SimpleDecoder is packed too (3 x (2048x128 + 2048x2048 + modulo x 2048) bf16 + fp32 biases)
    assert 38_000_000 < mf.weights_bytes - m.weights_bytes < 42_000_000 and mf.offset("decoder.0.l1.w") > 0
    assert lib.ftc_decoder_workspace_bytes(mf.handle, 2048) > 0
    assert lib.ftc_decoder_workspace_bytes(m.handle, 2048) == -1 and b"decoder" in lib.ftc_last_error()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_plan_structure_flops_and_arena(models, mode):
    pl = models[mode].plan(2, 768, 768)                  # built AND validated (ftc_plan_create rules) inside the library
    # forward work of the reference network: 432.50 GMAC = 865.0 GFLOP per image
    assert abs(sum(m.flops for m in pl.meta) / 2 / 1e9 - 865.0006) < 0.01
    kinds = [m.kind for m in pl.meta]
    assert kinds.count("dwconv3x3") == 80 and kinds.count("se") == 80 and kinds.count("stem") == 1 and kinds[-1] == "nms"
    # nine heads x three levels of upsample+concat and conv, nine top convs: grouped launches count once per instance
    inst = [max(1, pl.ops[i].groups) for i in range(len(kinds))]
    # (the last level forms its input in the convolution's loader and reads the shared tap, no upcat launch; round 5: in the fp32 / fp16x3 plans too)
    n_up = 2
    assert sum(n for k, n in zip(kinds, inst) if k == "upcat") == 9 * n_up and kinds.count("upcat") == n_up
    # the eight map heads' top convolutions live in the epilogue of the last FPN level (+ one TAPSUM); round 5: in the fp32 / fp16x3 plans too
    fused_top = 8
    # round 6, 16-bit plans: the 7 stride-1 Fused-MBConv blocks of stage 2 are ONE launch each (FTC_OP_FMBCONV: 3x3 expand + 1x1 project; stage 3's
    # Cin = 96 runs K steps of 32 and measured slower fused: FTC_FMBFUSE_ALL=1)
    fmb = kinds.count("conv3x3+conv1x1")
    assert fmb == (7 if mode == "bf16" else 0) and sum(pl.ops[i].kind == L.OP_FMBCONV for i in range(len(kinds))) == fmb
    assert sum(n for k, n in zip(kinds, inst) if k.startswith("conv")) == 20 + 16 + 160 + 1 + 1 + 27 + 9 - fused_top - fmb
    assert kinds.count("tapsum") == (1 if fused_top else 0)
    # arena: no two simultaneously-live buffers overlap
    live = {}
    ops = pl.ops
    spans = {}
    for i in range(len(ops)):
        for fld in ("in_", "in2", "out", "aux", "scale", "out2"):
            r = getattr(ops[i], fld)
            if r.base == L.BASE_WORKSPACE:
                s = spans.setdefault(r.offset, [i, i])
                s[1] = i
    assert max(spans) < pl.workspace_bytes and pl.workspace_bytes < 0.5 * pl.info.total_buffer_bytes
    assert pl.h == 192 and pl.w == 192 and pl.info.weights_bytes == models[mode].weights_bytes
    # the same op list is accepted by the op-list entry point
    h = C.c_void_p()
    assert L.load().ftc_plan_create(pl.ops, len(pl.ops), pl.workspace_bytes, pl.info.weights_bytes, C.byref(h)) == 0
    L.load().ftc_plan_destroy(h)


def test_bn_fold_and_kmajor_layout_match_torch(sd, models):
    """ftc_create: conv + eval BatchNorm == conv with folded weights + bias, in the K-major layout."""
    name = "backbone.features.2.1.block.0"
    w = sd[name + ".0.weight"]
    cout, cin, k, _ = w.shape
    wk = torch.from_numpy(_blob(models["fp32"], name + ".w", np.float32, (cout, k * k, cin)))
    b = torch.from_numpy(_blob(models["fp32"], name + ".b", np.float32, (cout,)))
    x = torch.randn(1, cin, 9, 9)
    ref = F.batch_norm(F.conv2d(x, w, None, 1, 1), sd[name + ".1.running_mean"], sd[name + ".1.running_var"], sd[name + ".1.weight"],
                       sd[name + ".1.bias"], False, 0.0, 1e-3)
    mine = F.conv2d(x, wk.reshape(cout, k, k, cin).permute(0, 3, 1, 2), b, 1, 1)
    assert float((ref - mine).abs().max()) < 1e-5


def test_merged_fpn_level0_border_bias_is_exact(sd, models):
    """The nine per-head (in_bn -> conv3x3 -> BN) at the 1/32 tap packed as ONE conv with a
    16-case border bias equals the reference composition (Leafmap.forward i=0, detector.py:194-197)."""
    C4, N = 1280, 9 * 192
    wk = torch.from_numpy(_blob(models["fp32"], "heads.L0.w", np.float32, (N, 3, 3, C4))).permute(0, 3, 1, 2)
    b16 = torch.from_numpy(_blob(models["fp32"], "heads.L0.b", np.float32, (16, N)))
    x = torch.randn(1, C4, 4, 5)
    y = F.conv2d(x, wk, None, 1, 1)
    H, W = 4, 5
    for oy in range(H):
        for ox in range(W):
            idx = (oy == 0) | ((oy == H - 1) << 1) | ((ox == 0) << 2) | ((ox == W - 1) << 3)
            y[0, :, oy, ox] += b16[idx]
    for hi, name in enumerate(["keyheatmap", "feature"]):
        h = {"keyheatmap": 0, "feature": 8}[name]
        xin = F.batch_norm(x, sd[f"{name}.in_bn.3.running_mean"], sd[f"{name}.in_bn.3.running_var"], sd[f"{name}.in_bn.3.weight"],
                           sd[f"{name}.in_bn.3.bias"], False, 0.0, 1e-5)
        ref = F.batch_norm(F.conv2d(xin, sd[f"{name}.upsamplers.0.0.weight"], None, 1, 1), sd[f"{name}.upsamplers.0.1.running_mean"],
                           sd[f"{name}.upsamplers.0.1.running_var"], sd[f"{name}.upsamplers.0.1.weight"],
                           sd[f"{name}.upsamplers.0.1.bias"], False, 0.0, 1e-5)
        assert float((ref - y[:, h * 192:(h + 1) * 192]).abs().max()) < 2e-4


def test_tuning_table_entries_are_legal(models):
    import json
    with open(tuning.TABLE_PATH) as f:
        tab = {k: int(v) for k, v in json.load(f)["choices"].items()}
    assert tab
    for k, v in tab.items():
        assert 0 <= v <= 0xfff and (v & 15) - 1 < len(tuning.CFG_NAMES), (k, v)
        assert tuning.describe(v)
    # the table compiled into the library (build.py: csrc/build/tuning_table.inc) is the committed JSON: the bench plan carries its choices
    pl = models["bf16"].plan(8, 768, 768)
    hits = 0
    for i in range(len(pl.ops)):
        if pl.ops[i].kind == L.OP_CONV:
            want = tab.get(tuning.signature(pl.ops[i]))
            if want:
                hits += 1
                assert pl.ops[i].aux0 == want, (pl.meta[i].name, pl.ops[i].aux0, want)
    assert hits > 80                     # (round 6: the 28 convolutions of the stride-1 Fused-MBConv blocks became 14 FTC_OP_FMBCONV launches: 122 -> 94)


def test_drop_in_module_schema_and_loud_failures():
    from findtextcenternet_amd import CenterNetDetector, TextDetectorModel
    from findtextcenternet_amd.schema import text_detector_schema
    m = TextDetectorModel(pre_weights=False)
    keys = list(m.state_dict().keys())
    assert keys == list(text_detector_schema("xl").keys()) and len(keys) == 2444
    m.load_state_dict(deterministic_state_dict(0))               # strict load of the reference key set
    det = CenterNetDetector(m.detector).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        det(torch.zeros(1, 3, 64, 64))
    with pytest.raises(TypeError):
        CenterNetDetector(torch.nn.Identity())


def test_tf_npz_importer_matches_reference_load_weight(tmp_path):
    """Our TF-checkpoint importer against the reference's own load_weight (models/detector.py:30-121),
    run in the build container on a synthetic npz: per-tensor digests in tests/golden/g5_tf_import_digest.json.gz."""
    import gzip
    import hashlib
    import json
    from findtextcenternet_amd import CenterNetDetection, load_tf_efficientnetv2_npz
    from findtextcenternet_amd.weights import tf_efficientnetv2_npz_names
    with gzip.open(os.path.join(ROOT, "tests", "golden", "g5_tf_import_digest.json.gz"), "rt") as f:
        ref = json.load(f)
    det = CenterNetDetection(pre_weights=False)
    sd = det.state_dict()
    rng = np.random.Generator(np.random.PCG64(ref["seed"]))
    arrs = {}
    for key, name, perm in tf_efficientnetv2_npz_names("xl"):
        shape = tuple(sd[key].shape)
        if perm is not None:
            shape = tuple(np.array(shape)[np.argsort(perm)])
        arrs[name] = rng.standard_normal(shape).astype(np.float32)
    path = str(tmp_path / "synthetic-xl.npz")
    np.savez(path, **arrs)
    bias_before = sd["backbone.features.4.0.block.2.fc1.bias"].clone()
    assert load_tf_efficientnetv2_npz(det, path) is True
    after = det.state_dict()
    assert len(ref["digest"]) == 1550
    for key, d in ref["digest"].items():
        assert hashlib.sha1(after[key].contiguous().numpy().tobytes()).hexdigest()[:16] == d, key
    assert torch.equal(after["backbone.features.4.0.block.2.fc1.bias"], bias_before)     # SE biases are not imported (reference quirk)
    assert load_tf_efficientnetv2_npz(det, str(tmp_path / "missing.npz")) is False


def test_adamw_schedulefree_host_schedule_matches_reference_fixture():
    """The float64 per-step scalars of findtextcenternet_amd.optim.step_scalars against what the reference's own optimizer
    recorded in its param_group (scheduled_lr, lr_max, weight_sum) -- tests/golden/g6_adamw_schedulefree.npz."""
    import synth
    from findtextcenternet_amd.optim import step_scalars
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "g6_adamw_schedulefree.npz"))
    for ci, cfg in enumerate(synth.ADAMW_CASES):
        kw = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_steps=0, r=0.0, weight_lr_power=2.0)
        kw.update(cfg["kwargs"])
        group = dict(kw, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
        for step in range(cfg["steps"]):
            sc = step_scalars(group)
            group["k"] += 1
            want = gold[f"c{ci}_sched"][step]
            assert [group["scheduled_lr"], group["lr_max"], group["weight_sum"]] == list(want)
            assert 0 < sc["bias_correction2"] <= 1 and sc["lr"] == group["scheduled_lr"]


@pytest.mark.parametrize("size", ["s", "m", "l"])
def test_library_builds_plans_for_the_other_model_sizes(size):
    """ftc_create + plan construction for the EfficientNetV2-S / -M / -L variants the reference can instantiate
    (models/detector.py:131-136): other stage depths, tap widths (Leafmap.in_dims :151-158) and, for 's', one stage fewer."""
    from findtextcenternet_amd.schema import STAGES
    sd_ = deterministic_state_dict(0, model_size=size, prefix_detector=False, with_decoder=False)
    for mode in ("fp32", "bf16"):
        m = FtcModel(sd_, mode, size)
        pl = m.plan(2, 128, 160)
        kinds = [x.kind for x in pl.meta]
        n_mb = sum(r[6] for r in STAGES[size] if r[0] == "mb")
        assert kinds.count("dwconv3x3") == n_mb == kinds.count("se") and kinds[0] == "stem" and kinds[-1] == "nms"
        assert pl.h == 32 and pl.w == 40
    with pytest.raises(L.FtcError, match="shape|missing"):
        FtcModel(sd_, "fp32", "xl")                          # a checkpoint of another size is rejected, not mis-read


def test_mbconv_slice_rejects_shapes_it_cannot_hold():
    lib = L.load()
    base = dict(kind=L.OP_MBHEAD, act=L.ACT_SILU, in_dtype=L.BF16, out_dtype=L.BF16, w_dtype=L.BF16, B=1, H=24, W=24, Ho=24, Wo=24, Cin=64, Cout=128,
                ksize=3, stride=1, aux0=0)
    for bad in (dict(H=25, Ho=25), dict(Cout=192), dict(Cin=48), dict(in_dtype=L.F32), dict(stride=2), dict(H=12, Ho=12, W=50, Wo=50)):
        op = (L.Op * 1)()
        for k, v in dict(base, **bad).items():
            setattr(op[0], k, int(v))
        for f in ("in_", "w2", "bias2", "w", "bias", "out", "aux"):
            r = getattr(op[0], f)
            r.base, r.offset = L.BASE_WORKSPACE, 0
        h = C.c_void_p()
        assert lib.ftc_plan_create(op, 1, 1 << 30, 0, C.byref(h)) != 0 and b"mbhead" in lib.ftc_last_error()


def test_px144_tile_configs_are_validated_and_planned(models):
    """The 144-pixel 1x1 kernel (aux0 low nibble 8..11, csrc/conv1x1_px144.hip) is refused where its tiles do not divide the op, and the bf16 batch-8
    plan runs the MBConv project convolutions of stages 4-7 on it (the tuning table's choice)."""
    lib = L.load()
    h = C.c_void_p()
    ok = dict(kind=L.OP_CONV, flags=L.FLAG_RESIDUAL, in_dtype=L.BF16, out_dtype=L.F32, w_dtype=L.BF16, res_dtype=L.F32, B=2, H=24, W=24, Ho=24, Wo=24,
              Cin=512, Cin_total=512, Cout=640, Cout_total=640, ksize=1, stride=1, in_=0, in2=1 << 22, out=1 << 23, w=1 << 21, bias=1 << 20)
    for aux0 in (8, 9, 10):                     # 640 = 10 x 64 = 8 x 80 = 5 x 128
        assert lib.ftc_plan_create(_op(**dict(ok, aux0=aux0)), 1, 1 << 25, 0, C.byref(h)) == 0, lib.ftc_last_error()
        lib.ftc_plan_destroy(h)
    for bad in (dict(ok, aux0=11),                               # 640 % 96
                dict(ok, aux0=8, H=16, W=16, Ho=16, Wo=16),      # 256 pixels per image: 144 does not divide
                dict(ok, aux0=8, Cin=480, Cin_total=480),        # K step 64
                dict(ok, aux0=8, out_dtype=L.BF16),              # fp32 output only
                dict(ok, aux0=8, act=L.ACT_SILU),
                dict(ok, aux0=8, ksize=3),
                dict(ok, aux0=8, in_dtype=L.F32, w_dtype=L.F32, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16)):      # fp16x3 needs BOTH operands pre-split
        assert lib.ftc_plan_create(_op(**bad), 1, 1 << 26, 0, C.byref(h)) == -1, bad
        assert b"x144" in lib.ftc_last_error() or b"conv" in lib.ftc_last_error()
    x3 = dict(ok, in_dtype=L.F32, w_dtype=L.F32, flags=L.FLAG_RESIDUAL | L.FLAG_SPLIT16 | L.FLAG_PRESPLIT, w=1 << 24, in_=1 << 22, in2=0)
    assert lib.ftc_plan_create(_op(**dict(x3, aux0=8)), 1, 1 << 26, 0, C.byref(h)) == 0, lib.ftc_last_error()
    lib.ftc_plan_destroy(h)
    pl = models["bf16"].plan(8, 768, 768)
    px = [pl.meta[i].name for i in range(len(pl.ops)) if pl.ops[i].kind == L.OP_CONV and 8 <= (pl.ops[i].aux0 & 15) <= 11 and not pl.ops[i].aux0 & 64]
    assert len(px) >= 70 and all(".block.3" in n or ".block.2" in n for n in px), (len(px), px[:4])


def test_fp16x3_plans_build_with_every_documented_switch(sd, monkeypatch):
    """Round-5 advisor (medium): the tuning table's signature drops FTC_FLAG_PRESPLIT, so an fp16x3 project convolution built WITHOUT
    pre-split operands (any of the switches below) used to inherit a 144-pixel-tile hint that is only legal with them, and
    ftc_plan_create refused the whole batch-8 / batch-32 plan.  apply_tuning now adopts a hint only if the op validates with it."""
    m = FtcModel(sd, "fp16x3")
    cases = [({"FTC_NO_PRESPLIT": "1"}, 8), ({"FTC_NO_MBSLICE_X3": "1"}, 8), ({"FTC_NO_MBSLICE": "1"}, 32), ({"FTC_MBSLICE_MINWG": "1000000"}, 32)]
    for env, B in cases:                         # (the plan cache is keyed by the switches: the same shape under each)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = m.plan(B, 768, 768)
        for k in env:
            monkeypatch.delenv(k)
        px = [i for i in range(len(pl.ops)) if pl.ops[i].kind == L.OP_CONV and 8 <= (pl.ops[i].aux0 & 15) <= 11 and not pl.ops[i].aux0 & 64]
        assert all(pl.ops[i].flags & L.FLAG_PRESPLIT for i in px), env
        if "FTC_NO_PRESPLIT" in env:
            assert not px
    # and the default plan does run the fused heads and the 144-pixel tiles
    pl = m.plan(16, 768, 768)
    n_head = sum(pl.ops[i].kind == L.OP_MBHEAD for i in range(len(pl.ops)))
    px = [i for i in range(len(pl.ops)) if pl.ops[i].kind == L.OP_CONV and 8 <= (pl.ops[i].aux0 & 15) <= 11 and not pl.ops[i].aux0 & 64]
    assert n_head >= 70, n_head


def test_round6_kernels_are_selected_by_the_plans_that_bench_runs(sd, models):
    """The batch-8 plans of the two modes bench.py reports -- bf16 (`value`) and fp16x3 (`config.contract_mode`) -- run stage 1 on the resident 32 -> 32 kernel
    (csrc/conv3x3_c32.hip: 4 launches) and the stride-1 blocks of stage 2 as one launch each (FTC_OP_FMBCONV: 7); the exact-fp32 plan keeps the generic kernels."""
    lib = L.load()
    buf = C.create_string_buffer(160)

    def labels(m):
        pl = m.plan(8, 768, 768)
        out = []
        for i in range(len(pl.ops)):
            L.check(lib.ftc_op_kernel_label(C.byref(pl.ops[i]), buf, 160), "ftc_op_kernel_label")
            out.append(buf.value.decode())
        return out
    for mode, m in (("bf16", models["bf16"]), ("fp16x3", FtcModel(sd, "fp16x3")), ("fp32", models["fp32"])):
        lab = labels(m)
        n_c32 = sum(l.startswith("conv3x3_c32<") for l in lab)
        n_fmb = sum(l.startswith("fmbconv_fused<") for l in lab)
        assert (n_c32, n_fmb) == ((4, 7) if mode != "fp32" else (0, 0)), (mode, n_c32, n_fmb)
        if mode == "fp16x3":
            assert all("f16x3" in l for l in lab if l.startswith(("conv3x3_c32<", "fmbconv_fused<")))


def test_fused_block_switches_change_the_plan_and_it_still_validates(models, monkeypatch):
    """FTC_NO_FMBFUSE=1 keeps the two-launch form of the Fused-MBConv blocks, FTC_FMBFUSE_ALL=1 also fuses stage 3 (measured slower):
    both plans build and pass ftc_plan_create's validation."""
    m = models["bf16"]
    key = (4, 768, 768)                          # (the plan cache is keyed by the switches: one shape under all three settings)
    for env, want in (({"FTC_NO_FMBFUSE": "1"}, 0), ({"FTC_FMBFUSE_ALL": "1"}, 14), ({}, 7)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        pl = m.plan(*key)
        for k in env:
            monkeypatch.delenv(k)
        assert sum(pl.ops[i].kind == L.OP_FMBCONV for i in range(len(pl.ops))) == want, env
        assert abs(sum(mm.flops for mm in pl.meta) / key[0] / 1e9 - 865.0006) < 0.01          # the same network either way


# ---- the kernel choice of FTC_OP_CONV (csrc/conv_choice.h) -----------------------------------------------------------------------

@pytest.mark.parametrize("part", ["table", "fuzz", "special", "every_aux0"])
def test_conv_choice_sweep_matches_the_recorded_one(part):
    """Which (op, aux0) pairs ftc_plan_create accepts, the full error text of the others and every kernel label, entry by entry against
    tests/golden/conv_choices.json.gz (written by tests/conv_choice_sweep.py --write before the choice moved into conv_resolve)."""
    import conv_choice_sweep as S
    gold = S.load_golden()
    want = gold["parts"][part]
    got = S.replay(part)
    assert len(got) == len(want)
    ents = S.entries(part)
    for i, ((lab, err), (li, ei)) in enumerate(zip(got, want)):
        assert (lab, err) == (gold["labels"][li], None if ei < 0 else gold["errors"][ei]), (part, i, ents[i])
    assert sum(err is None for _, err in got) == {"table": 4186, "fuzz": 943, "special": 241, "every_aux0": 191 + 263 + 247 + 389 + 95}[part]


def test_conv_choice_of_every_op_of_the_xl_plans_matches_the_recorded_one(sd, models):
    """(kind, aux0, label) of every op of the xl plans at 768 x 768 in the modes and batch sizes bench.py and the GPU suite run."""
    import conv_choice_sweep as S
    gold = S.load_golden()
    ms = dict(models)
    for mode, B in S.PLAN_CASES:
        if mode not in ms:
            ms[mode] = FtcModel(sd, mode)
        want = [[k, a, gold["labels"][li]] for k, a, li in gold["plans"][f"{mode}_b{B}"]]
        assert S.plan_entries(ms[mode], B) == want, (mode, B)


def test_an_explicit_hint_is_the_kernel_the_label_names():
    """The contract between tuning.candidates and the library: for every (op, hint) pair of the table and fuzz sweeps that ftc_plan_create accepts, the label names the
    family, tile, K step, ring depth and split-K that tuning.describe(hint) names.  The two kernels without variants (thin_conv3x3, conv3x3_c32) take their ops
    whatever the hint says."""
    import conv_choice_sweep as S
    bad, n = [], 0
    for part in ("table", "fuzz"):
        for f, aux0 in S.entries(part):
            if aux0 == 0:
                continue
            lab, err = S.verdict(S.make_op(dict(f, aux0=aux0)))
            if err is not None or lab.startswith(("thin_conv3x3<", "conv3x3_c32<")):
                continue
            n += 1
            d = dict(kv.split("=") for kv in tuning.describe(aux0).split(",") if "=" in kv)
            if tuning.describe(aux0).startswith("halo"):
                ok = lab.startswith("conv3x3_halo<") and f",tile={d['channels']}x16x16," in lab and (d.get("bk") != "32" or lab.endswith(",bk=32>"))
            elif tuning.describe(aux0).startswith("px144"):
                ok = lab.startswith("conv1x1_px144<") and f",tile={d['tile']}," in lab
            else:
                ring = {"reg": 1, "dma2": 2, "dma3": 3}[d["stage"]]
                ok = (lab.startswith("conv_igemm_glds<" if ring > 1 else "conv_igemm<") and f",tile={d['tile']},bk={d['bk']},nbuf={ring}" in lab and
                      (f",splitk={d['splitk']}>" in lab if "splitk" in d else "splitk" not in lab))
            if not ok:
                bad.append((tuning.describe(aux0), lab))
    assert n > 4000 and not bad, (n, len(bad), bad[:5])


def test_conv_choice_header_is_host_only_and_clean_under_sanitizers(tmp_path):
    """csrc/conv_choice.h needs no HIP header: tests/c_abi/conv_choice_host.cc (plain C++, its own main) resolves and labels every aux0 on five ops under
    AddressSanitizer + UBSan and prints what the library answered for the same entries."""
    import subprocess
    import conv_choice_sweep as S
    exe = str(tmp_path / "conv_choice_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c_abi", "conv_choice_host.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    gold = S.load_golden()
    lines = r.stdout.splitlines()
    want = gold["parts"]["every_aux0"]
    assert len(lines) == len(want)
    for line, (li, ei) in zip(lines, want):
        why, lab = line.split("\t")
        assert lab == gold["labels"][li] and (why == "" if ei < 0 else gold["errors"][ei].endswith(why) and why != ""), (line, gold["labels"][li], ei)


# ---- the kernel choice of FTC_OP_WGRAD (csrc/wgrad_choice.h) ----------------------------------------------------------------------

def test_wgrad_splits_match_the_recorded_ones():
    """ftc_wgrad_splits over the shape grid of tests/wgrad_choice_sweep.py against tests/golden/wgrad_choices.json.gz (part "splits", written from the commit
    before the rule moved next to wgrad_resolve)."""
    import wgrad_choice_sweep as S
    want = S.load_golden()["splits"]
    got = S.replay_splits()
    assert len(got) == len(want) == len(S.SPLIT_GRID)
    bad = [(g, a, b) for g, a, b in zip(S.SPLIT_GRID, got, want) if a != b]
    assert not bad, (len(bad), bad[:5])


def test_wgrad_ops_of_the_train_plans_match_the_recorded_ones():
    """Every field (aux0 = the split count and the buffer references included) of every FTC_OP_WGRAD op of the six train plans."""
    import wgrad_choice_sweep as S
    want = S.load_golden()["train_ops"]
    got = S.train_ops()
    assert sorted(got) == sorted(want)
    for case in want:
        assert len(got[case]) == len(want[case]) == 251, case
        for i, (a, b) in enumerate(zip(got[case], want[case])):
            assert a == b, (case, i, dict(zip(S.INT_FIELDS, a)), dict(zip(S.INT_FIELDS, b)))


@pytest.mark.parametrize("part", ["cases", "train", "grid", "refused"])
def test_wgrad_choice_sweep_matches_the_recorded_one(part):
    """Which ops ftc_plan_create accepts, the full error text of the others and every kernel label, entry by entry against part "choices" of
    tests/golden/wgrad_choices.json.gz (written when the conditions of launch_wgrad had moved into wgrad_resolve verbatim and nothing else had changed)."""
    import wgrad_choice_sweep as S
    gold = S.load_golden()
    want = gold["choices"][part]
    ents = S.entries(part)
    got = S.replay_choices(part)
    assert len(got) == len(want) == len(ents)
    for i, ((lab, err), (li, ei)) in enumerate(zip(got, want)):
        assert err == (None if ei < 0 else gold["errors"][ei]), (part, i, ents[i])
        assert err is not None or lab == gold["labels"][li], (part, i, ents[i])          # (a refused op has no choice to label)
    assert sum(err is None for _, err in got) == (0 if part == "refused" else len(want))


def test_wgrad_cases_reach_every_kernel_family():
    """The ops test_wgrad and test_wgrad_exact run (WG_CASES x the seven storage configurations, the row's own flags) reach, by their labels: all five
    kernel families, both 16-bit types of the three 16-bit-only ones, the four tiles of the generic kernel, the thin kernel with 1 and 2 output channels at
    k = 1 and k = 3, an SE gate applied while staging and one applied to the partial tile (generic kernel and DMA ring)."""
    import wgrad_choice_sweep as S
    from test_gpu_bwd_ops import WG_CASES
    labels = set()
    for c in WG_CASES:
        for wd, io in S.STORAGE:
            lab, err = S.verdict(S.make_op(S.case_fields(c, wd, io, S.case_flags(c))))
            assert err is None, (c[0], wd, io, err)
            labels.add(lab)
    want = [f"{k}<{t}" for k in ("wgrad3t_kernel", "wgrad3_kernel", "wgrad1t_kernel") for t in ("bf16>", "f16>")]
    want += ["wgrad1t_kernel<bf16,gate=epi>", "wgrad1t_kernel<f16,gate=epi>", "wgrad_kernel<f32,", "wgrad_kernel<bf16,", "wgrad_kernel<f16,", ",gate=staged>", ",gate=epi>"]
    want += [f",tile={t}," for t in ("32x128", "64x64", "128x128", "192x256")]
    want += [f",co={co},k={k}>" for co in (1, 2) for k in (1, 3)] + ["wgrad_thin_kernel<x=f32,", "wgrad_thin_kernel<x=bf16,"]
    want += [f"wgrad_kernel<{w},x={x},dz={d}," for w, x, d in (("f32", "f32", "f32"), ("bf16", "f32", "f32"), ("bf16", "bf16", "f32"), ("bf16", "bf16", "bf16"), ("f16", "f32", "f16"))]
    missing = [w for w in want if not any(w in lab and lab.endswith(("+reduce", "+reduce_wide")) for lab in labels)]
    assert not missing, (missing, sorted(labels))


@pytest.fixture(scope="module")
def wgrad_choice_host(tmp_path_factory):
    """tests/c_abi/wgrad_choice_host.cc (plain C++ over csrc/wgrad_choice.h alone, its own main) built with AddressSanitizer + UBSan; returns a function
    that runs it on request lines and returns its output lines."""
    import subprocess
    exe = str(tmp_path_factory.mktemp("wgrad_choice") / "wgrad_choice_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c_abi", "wgrad_choice_host.cc"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split("\n")[:-1]
    return run


def test_wgrad_choice_header_is_host_only_and_clean_under_sanitizers(wgrad_choice_host):
    """csrc/wgrad_choice.h needs no HIP header: the stand-alone program resolves and labels every op of the recorded sweeps and answers the recorded
    split counts, what the library answered for the same entries."""
    import wgrad_choice_sweep as S
    gold = S.load_golden()
    assert [int(v) for v in wgrad_choice_host(["s " + " ".join(map(str, g)) for g in S.SPLIT_GRID])] == gold["splits"]
    for part in S.CHOICE_PARTS:
        ents = S.entries(part)
        lines = wgrad_choice_host(["o " + " ".join(str(int(f.get(n, 0))) for n in S.INT_FIELDS) for f in ents])
        want = gold["choices"][part]
        assert len(lines) == len(want)
        for f, line, (li, ei) in zip(ents, lines, want):
            why, lab = line.split("\t")[:2]
            assert (why == "" and lab == gold["labels"][li]) if ei < 0 else (why != "" and gold["errors"][ei].endswith(why)), (part, f, line)


def test_wgrad_labels_and_choices_correspond_one_to_one(wgrad_choice_host):
    """Over the recorded sweeps: two ops with one label run one instantiation (family, template arguments, form of the gate, reduction kernel), and two
    ops that run one instantiation have one label."""
    import wgrad_choice_sweep as S
    by_label, by_choice = {}, {}
    for part in ("cases", "train", "grid"):
        for line in wgrad_choice_host(["o " + " ".join(str(int(f.get(n, 0))) for n in S.INT_FIELDS) for f in S.entries(part)]):
            why, lab, choice, launch = line.split("\t")
            assert why == "" and choice.startswith("family=") and launch.startswith("chunk=")
            assert by_label.setdefault(lab, choice) == choice and by_choice.setdefault(choice, lab) == lab, (lab, choice, by_label.get(lab), by_choice.get(choice))
    assert len(by_label) == len(by_choice) >= 40


# ---- the kernel choice of FTC_OP_STEM, DWCONV, SE, MBHEAD, FMBCONV and UPCAT (csrc/backbone_choice.h) -------------------------------------------

@pytest.mark.parametrize("part", ["plans", "cases", "grid", "refused"])
def test_backbone_choice_sweep_matches_the_recorded_one(part):
    """Which ops ftc_plan_create accepts, the full error text of the others and every kernel label, entry by entry against part "choices" of
    tests/golden/backbone_choices.json.gz."""
    import backbone_choice_sweep as S
    gold = S.load_golden()
    want = gold["choices"][part]
    ents = S.entries(part)
    got = S.replay(part)
    assert len(got) == len(want) == len(ents) > 0
    for i, ((lab, err), (li, ei)) in enumerate(zip(got, want)):
        assert err == (None if ei < 0 else gold["errors"][ei]), (part, i, ents[i])
        assert err is not None or lab == gold["labels"][li], (part, i, ents[i])          # (a refused op has no choice to label)
    if part == "refused":
        assert not any(err is None for _, err in got)
        prefixes = {S.KIND_NAME[f["kind"]] + ": " for f in ents}
        assert all(any(p in err for p in prefixes) for _, err in got)                    # every reason keeps its kind prefix


def test_backbone_choices_equal_the_ones_before_the_resolvers():
    """Parts plans, cases and grid against "stage1", recorded from the commit before csrc/backbone_choice.h: the same ops accepted under the same labels,
    the same ops refused -- except the ops the rules of NEWLY_REFUSED name, which are refused now, each with (one of) the reason(s) its rule(s) give."""
    import backbone_choice_sweep as S
    gold = S.load_golden()
    hit = {name: 0 for name, _, _ in S.NEWLY_REFUSED}
    for part in ("plans", "cases", "grid"):
        ents = S.entries(part)
        assert len(ents) == len(gold["stage1"][part]) == len(gold["choices"][part])
        for i, (f, (li1, ok1), (li, ei)) in enumerate(zip(ents, gold["stage1"][part], gold["choices"][part])):
            if ok1 and ei >= 0:
                reasons = S.newly_refused(f)
                assert any(gold["errors"][ei].endswith(r) for r in reasons), (part, i, f, gold["errors"][ei], reasons)
                for name, rule, _ in S.NEWLY_REFUSED:
                    hit[name] += bool(rule(f))
            else:
                assert bool(ok1) == (ei < 0) and (not ok1 or gold["labels"][li1] == gold["labels"][li]), (part, i, f)
                assert not (ok1 and S.newly_refused(f)), (part, i, f)
    assert all(hit.values()), hit                                # every rule refuses something the library used to accept
    assert all(ei < 0 for _, ei in gold["choices"]["plans"])     # no op of a plan of ours is among them


@pytest.fixture(scope="module")
def backbone_choice_host(tmp_path_factory):
    """tests/c_abi/backbone_choice_host.cc (plain C++ over csrc/backbone_choice.h alone, its own main) built with AddressSanitizer + UBSan; returns a function
    that runs it on sweep entries and returns its output lines split at the tabs: [reason, label, instantiation, launch]."""
    import subprocess
    import backbone_choice_sweep as S
    exe = str(tmp_path_factory.mktemp("backbone_choice") / "backbone_choice_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c_abi", "backbone_choice_host.cc"), "-o", exe], check=True)

    def run(ents):
        r = subprocess.run([exe], input="".join(S.host_line(f) + "\n" for f in ents), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [line.split("\t") for line in r.stdout.split("\n")[:-1]]
        assert len(lines) == len(ents) and all(len(line) == 4 for line in lines)
        return lines
    return run


def test_backbone_choice_header_is_host_only_and_clean_under_sanitizers(backbone_choice_host):
    """csrc/backbone_choice.h needs no HIP header: the stand-alone program resolves and labels every op of the recorded sweeps, refuses what the library
    refused for the reason the library gave, and labels the others as the library did."""
    import backbone_choice_sweep as S
    gold = S.load_golden()
    for part in S.PARTS:
        ents = S.entries(part)
        want = gold["choices"][part]
        for f, (why, lab, _, _), (li, ei) in zip(ents, backbone_choice_host(ents), want):
            assert (why == "" and lab == gold["labels"][li]) if ei < 0 else (why != "" and gold["errors"][ei].endswith(why)), (part, f, why, lab)


def test_backbone_gpu_cases_reach_the_forms_their_names_say(backbone_choice_host):
    """The kernel form behind each named case of the GPU suites, which no label shows: the SE forms of test_gpu_se_bits.FORMS (and fc2_plain_hpart) and of
    test_se_saturated, and the band48 / band / fast / whole groups of test_gpu_mbhead_bits.py."""
    import backbone_choice_sweep as S
    import test_gpu_exact_mbconv as EM
    import test_gpu_mbhead_bits as MB
    import test_gpu_se_bits as SB
    want = {"fold64_bf16": "family=fold64 T=bf16 fc1=0", "fold64_f16": "family=fold64 T=f16 fc1=0", "foldx3": "family=foldx3 T=- fc1=0", "gates64": "family=gates64 T=- fc1=0",
            "fc2_plain": "family=fc1+fc2 T=- fc1=1", "fold_v1_bf16": "family=fc1+fc2_fold T=bf16 fc1=1", "fc2_plain_hpart": "family=fc2_hpart T=- fc1=0"}
    assert {n for n, *_ in SB.FORMS} | {"fc2_plain_hpart"} == set(want) == {c["form"] for c in SB.CASES}
    for c, (why, _, inst, _) in zip(SB.CASES, backbone_choice_host([S.se_bits_fields(c) for c in SB.CASES])):
        assert why == "" and inst == want[c["form"]], (c["id"], why, inst)
    sat = {("gates", False): ["family=fc1+fc2 T=- fc1=1"], ("gates", True): ["family=gates64 T=- fc1=0", "family=fc2_hpart T=- fc1=0"],
           ("fold_v1_bf16", False): ["family=fc1+fc2_fold T=bf16 fc1=1"], ("fold_v1_f16", False): ["family=fc1+fc2_fold T=f16 fc1=1"]}
    sat.update({(f"fold_{t}", hp): [f"family=fold64 T={t} fc1={int(not hp)}"] for t in ("bf16", "f16") for hp in (False, True)})
    sat.update({("fold_f16x3", hp): [f"family=foldx3 T=- fc1={int(not hp)}"] for hp in (False, True)})
    seen = set()
    for p in S.params(EM.test_se_saturated):
        named = S.se_sat_fields(p["case"], p["hpart"])
        for (name, _), (why, _, inst, _) in zip(named, backbone_choice_host([f for _, f in named])):
            assert why == "" and inst in sat[(name, p["hpart"])], (p, name, why, inst)
            seen.add(inst)
    assert seen == {i for v in sat.values() for i in v}          # (both kernels behind "gates" on partial products included)
    group = {"band48": "family=band48", "band": "family=general", "fast": "family=map24", "whole": "family=general"}
    for c, (why, _, inst, launch) in zip(MB.CASES, backbone_choice_host([S.mbhead_bits_fields(c) for c in MB.CASES])):
        assert why == "" and inst == f"{group[c['path']]} slice={c['slice']} T={'bf16' if c['dt'] == L.BF16 else 'f16'}", (c["id"], why, inst)
        assert f" nb={c['nb']} " in launch and f"hpart={int(c['hp'])} " in launch, (c["id"], launch)
        assert (c["nb"] > 1) == (c["path"] in ("band48", "band")), c["id"]


def test_backbone_gpu_cases_reach_every_kernel_instantiation(backbone_choice_host):
    """Every family of every kind, with every template argument it has, is what at least one case of the GPU suites (part "cases") runs."""
    import backbone_choice_sweep as S
    cases = S.case_entries()
    got = {}
    for (test, cid, f), (why, _, inst, _) in zip(cases, backbone_choice_host([f for _, _, f in cases])):
        if why == "":
            got.setdefault((S.KIND_NAME[f["kind"]], inst), f"{test} {cid}")
    want = [("stem", f"family={fam} out={o} copy={c} nq={nq} fast={int(fam > 0)}") for fam, o, c in ((0, "f32", "bf16"), (1, "f32", "bf16"), (1, "f32", "f16"), (2, "bf16", "bf16"), (2, "f16", "f16"))
            for nq in (1, 4)]
    want += [("dwconv", f"family=strip T={t} stride=1") for t in ("f32", "bf16", "f16")] + [("dwconv", f"family=general T={t} stride={s}") for t in ("f32", "bf16", "f16") for s in (1, 2)]
    want += [("se", "family=fc1+fc2 T=- fc1=1"), ("se", "family=fc2_hpart T=- fc1=0"), ("se", "family=gates64 T=- fc1=0"), ("se", "family=foldx3 T=- fc1=0"), ("se", "family=foldx3 T=- fc1=1")]
    want += [("se", f"family=fold64 T={t} fc1={fc1}") for t in ("bf16", "f16") for fc1 in (0, 1)] + [("se", f"family=fc1+fc2_fold T={t} fc1=1") for t in ("bf16", "f16")]
    want += [("mbhead", f"family={fam} slice={sl} T={t}") for fam in ("map24", "band48", "general") for sl in (128, 96) for t in ("bf16", "f16")]
    want += [("mbhead", f"family={fam} slice=64 T=f16x3") for fam in ("map24", "general")]
    want += [("fmbconv", f"T={t} E={E} bk={bk} sn={2 if E == 256 else 3}") for t in ("bf16", "f16") for E in (256, 384) for bk in (32, 64)] + [("fmbconv", "T=f16x3 E=256 bk=32 sn=0")]
    want += [("upcat", f"T={t} TT={tt} V={4 if t == 'f32' else 8}") for t, tt in (("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"), ("f16", "f32"), ("f16", "f16"))]
    assert sorted(got) == sorted(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))


# ---- the kernel forms of FTC_OP_BNSTAT, BNACT, BNBWD, DWBWD and SEBWD and the labels of the remaining kinds (csrc/train_choice.h) ---------------

@pytest.fixture(scope="module")
def train_choice_host(tmp_path_factory):
    """tests/c_abi/train_choice_host.cc (plain C++ over csrc/train_choice.h alone, its own main) built with AddressSanitizer + UBSan; returns a function that
    runs it on ops (tests/train_choice_host.py) and returns per op (reason, label, instantiation, launch)."""
    import train_choice_host as H
    return H.build(tmp_path_factory.mktemp("train_choice"))


def test_train_choice_header_is_host_only_and_clean_under_sanitizers(train_choice_host):
    """csrc/train_choice.h needs no HIP header: the stand-alone program resolves accepted and refused ops of the five kinds -- every refusal the header has --
    and answers as the library does: accepted exactly where ftc_plan_create accepts, refused for the reason it gives, labelled as ftc_op_kernel_label labels.
    The launch arithmetic behind the accepted ones is held to its Python restatements in test_bn_operands_host.py, test_se_operands_host.py and
    test_exact_operands_host.py; verdicts and messages of thousands more ops are tests/golden/op_extents.json.gz's."""
    import backbone_choice_sweep as S
    import train_choice_host as H
    sh = (2, 5, 13, 24)
    ok = [H.bnstat(sh), H.bnstat(sh[:3] + (9,), L.F16), H.bnact(sh, L.F32, L.F32, L.BF16, 3, L.BF16, True), H.bnact(sh[:3] + (9,), L.F16, L.F16, L.F16, 0),
          H.bnbwd(sh, L.F32, L.F32), H.bnbwd(sh, L.BF16, L.BF16, "both", True), H.bnbwd(sh, L.F16, L.F32, "out2"), H.dwbwd(sh, 1), H.dwbwd(sh, 2, "data"),
          H.dwbwd(sh, 2, "weight"), H.sebwd(sh, 6, 3)]
    bad = [dict(H.bnstat(sh), B=0), dict(H.bnstat(sh), Cin=0), H.bnstat(sh, 5),
           dict(H.bnact(sh, L.F32, L.F32, L.BF16), aux0=65536), H.bnact(sh, 5, L.F32, L.BF16), H.bnact(sh, L.F16, L.F32, L.BF16), H.bnact(sh, L.F32, L.F32, L.BF16, 1, L.F16),
           dict(H.bnact(sh, L.F32, L.F32, L.BF16), act=9), H.bnact(sh, L.F32, L.BF16, L.BF16, 1, None, True),
           H.bnbwd(sh[:3] + (6,), L.F32, L.F32), dict(H.bnbwd(sh, L.F32, L.F32), Cin_total=16), dict(H.bnbwd(sh, L.F32, L.F32), act=9), dict(H.bnbwd(sh, L.F32, L.F32), _refs=("in_", "in2", "scale", "aux")),
           H.bnbwd(sh, L.F32, L.F32, "both"), H.bnbwd(sh, L.BF16, L.BF16, "out2", True), H.bnbwd(sh, L.BF16, L.F16),
           dict(H.dwbwd(sh, 1), stride=3), dict(H.dwbwd(sh, 2), Ho=5), dict(H.dwbwd(sh, 1), _refs=("in2",)),
           H.sebwd(sh, 0), H.sebwd(sh[:3] + (8000,), 6)]
    got = train_choice_host(ok + bad)
    reasons = set()
    for f, (why, lab, _, _) in zip(ok + bad, got):
        label, err = S.verdict(S.make_op(f))
        assert lab == label and (why == "" and err is None if f in ok else why != "" and err is not None and err.endswith(why)), (f, why, lab, label, err)
        reasons.add(why)
    assert len(reasons) == 1 + len(bad) == 22                    # each refused op for another reason: the 21 the header holds
    # the kinds that choose nothing: their labels moved with the five; CONV, WGRAD and the backbone kinds are not this header's
    others = [dict(kind=k, w_dtype=dt, stride=2) for k in (L.OP_NMS, L.OP_TAPSUM, L.OP_GATHER_ROWS, L.OP_LOSSES, L.OP_LOSS_BWD, L.OP_SCATTER_ROWS, L.OP_UPCATBWD, L.OP_DILATE,
                                                            L.OP_TOPDGRAD, L.OP_COLSUM, L.OP_STEMWGRAD, L.OP_FILL, L.OP_JOIN) for dt in (L.F32, L.BF16, L.F16)]
    for f, (why, lab, _, _) in zip(others, train_choice_host(others, letter="l")):
        assert why == "" and lab == S.label(S.make_op(f)), (f, why, lab)
    theirs = [dict(kind=k) for k in (L.OP_CONV, L.OP_WGRAD, L.OP_STEM, L.OP_DWCONV, L.OP_SE, L.OP_MBHEAD, L.OP_FMBCONV, L.OP_UPCAT, 0, 99)]
    assert all(why == "no label" and lab == "" for why, lab, _, _ in train_choice_host(theirs, letter="l"))


# ---- plan construction and weight packing against the recorded ones (tests/plan_sweep.py) ----------------------------------------

@pytest.fixture(scope="module")
def plan_replay():
    """(recorded, replayed): tests/golden/model_plans.json.gz, written by `tests/plan_sweep.py --write` from the library of the commit before the
    plan builder was split up, and the same cases from the library in the tree.  The sweep builds its own models -- the xl ones from the checkpoint
    WITH the decoder, which the `models` fixture above does not carry.  The plan cache is keyed by the switches, so every switch case of a mode
    runs on the one xl model of that mode."""
    import plan_sweep as S
    return S.load_golden(), S.replay()


@pytest.mark.parametrize("part", ["plans", "weights", "decoder"])
def test_plans_weights_and_decoder_workspaces_equal_the_recorded_ones(plan_replay, part):
    """plans: every field of every ftc_op (refs and tuned aux0 included), every op's name, kind, flops and bytes and the plan totals, for xl at
    768 x 768 in four modes and four batch sizes, the other sizes, and every plan switch alone; weights: the sha256 of every MiB of the packed blob
    of 13 models; decoder: the workspace sizes of the two decoder paths.  Equal plans on equal weights are the same launches on the same data."""
    import plan_sweep as S
    want, got = plan_replay
    assert sorted(got[part]) == sorted(want[part])
    assert len(want["plans"]) == 94 and len(want["weights"]) == 13 and len(want["decoder"]) == 4
    assert S.decoder_sizes_missing(want) == [] and S.decoder_sizes_missing(got) == []          # (-1: a model without the decoder compares nothing)
    diff = S.first_difference(want, got, part)
    assert diff is None, diff


def test_a_plan_difference_is_named_by_case_op_and_field(plan_replay):
    import copy
    import plan_sweep as S
    want, got = plan_replay
    name = S.case_name("xl", "bf16", 8, 768, 768)
    bad = {"plans": {name: copy.deepcopy(got["plans"][name])}}
    bad["plans"][name]["ops"][5][S.RECORD_FIELDS.index("out2.offset")] += 256
    diff = S.first_difference({"plans": {name: want["plans"][name]}}, bad, "plans")
    assert diff.startswith(f"plan {name}: op 5 (backbone.features.") and "out2.offset = " in diff, diff


def test_every_plan_switch_changes_a_plan_and_an_off_value_does_not(plan_replay):
    """Each switch differs from the default plan of the same mode and batch in at least one of fp32, bf16 and fp16x3 (in the recorded plans and in
    the replayed ones: a case that changed nothing would prove nothing), and FTC_NO_MBSLICE=0 / FTC_NO_MBSLICE= (empty) are the default plan."""
    import plan_sweep as S
    for doc in plan_replay:
        assert S.idle_switches(doc) == []
        base = doc["plans"][S.case_name("xl", "bf16", 8, 768, 768)]
        for k, v in S.SAME_AS_DEFAULT:
            assert doc["plans"][S.case_name("xl", "bf16", 8, 768, 768, False, {k: v})] == base, (k, v)
    minwg1 = plan_replay[1]["plans"][S.case_name("xl", "bf16", 2, 768, 768, False, {"FTC_MBSLICE_MINWG": "1"})]
    assert minwg1 != plan_replay[1]["plans"][S.case_name("xl", "bf16", 2, 768, 768)]


def test_plan_cache_is_keyed_by_the_switches(models, monkeypatch):
    """A switch set between two requests for the same shape gives the plan of the new setting, and taking it away gives the first plan back."""
    m = models["bf16"]
    n_fmb = lambda pl: sum(pl.ops[i].kind == L.OP_FMBCONV for i in range(len(pl.ops)))       # noqa: E731
    first = m.plan(3, 768, 768)
    assert n_fmb(first) == 7
    monkeypatch.setenv("FTC_NO_FMBFUSE", "1")
    assert n_fmb(m.plan(3, 768, 768)) == 0
    monkeypatch.delenv("FTC_NO_FMBFUSE")
    assert m.plan(3, 768, 768).handle == first.handle
