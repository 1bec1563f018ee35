"""The training-mode graph of ``TextDetectorModel`` -- batch-statistics BatchNorm and StochasticDepth -- as an op list over the library's
plan interface (``include/ftc.h``), written once for the two paths that run it: ``TrainForward`` (the reference's BN-refresh forward,
no gradients) and ``TrainStep`` (the same forward, then the backward).

``emit_detector_forward`` and ``emit_decoder_forward`` walk the module's ``state_dict`` shapes (the graph knowledge the reference keeps in
Python as well) and emit through a ``Builder``.  The two callers differ only in data: the builder's settings (16-bit activation copies,
16-bit conv outputs, the side stream), the buffers each pins, and what each does with the resolved op array.  Weight names are those of
the packed weight tables: ``<conv or Linear>.weight#f`` K-major in the compute type (Linear K padded to 128), ``#d`` the data-gradient
layout, ``#dw`` depthwise [9][C] fp32, ``#t`` SE fc2 transposed [S][C] fp32, ``#stem`` [(r*3+s)*3+c][C0] fp32, ``<bn>.running`` the
[mean | var] pair of a BatchNorm; every other weight under its ``state_dict`` name.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from typing import Dict, List, Optional, Tuple

from . import _lib as L

BACKBONE_EPS, HEAD_EPS = 1e-3, 1e-5          # models/detector.py:27; nn.BatchNorm2d default (:161-184)
HEAD_NAMES = ["keyheatmap", "sizes", "textline", "sepatator", "code1", "code2", "code4", "code8"]
_STAGE_STRIDE = {1: 1, 2: 2, 3: 2, 4: 2, 5: 1, 6: 2, 7: 1}    # first-block stride per stage (models/detector.py:14-20, tv s/m/l tables)
F32ONLY = dict(want32=True, want16=False)
GEMM_ONLY = dict(want32=False, want16=True)          # read by convolutions only: the 16-bit copy suffices (fp32 mode: fp32)


def _fbits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


class _Buf:
    def __init__(self, nbytes: int):
        self.nbytes, self.first, self.last, self.offset = _align(nbytes), 1 << 30, -1, -1


def stochastic_depth_probs(sd_shapes) -> Dict[str, float]:
    """torchvision EfficientNet.__init__: sd_prob = 0.2 * block_id / total_blocks over ALL blocks of the backbone."""
    blocks = []
    i = 1
    while f"detector.backbone.features.{i}.0.block.0.0.weight" in sd_shapes:
        j = 0
        while f"detector.backbone.features.{i}.{j}.block.0.0.weight" in sd_shapes:
            blocks.append(f"backbone.features.{i}.{j}")
            j += 1
        i += 1
    return {p: 0.2 * k / len(blocks) for k, p in enumerate(blocks)}


class Builder:
    """Op-list builder.  An activation is a pair (fp32 tensor | None, 16-bit copy | None): with ``h16`` the BatchNorm passes write a copy in
    the compute type next to (or instead of) the fp32 tensor, the GEMMs (forward conv, data gradient, weight gradient) read the copies --
    half the operand bytes, DMA-staged kernels -- and fp32 stays where something other than a GEMM reads it (residual trunk, FPN taps,
    depthwise input, SE).  Without ``h16`` every activation is (fp32, None).

    table: weight name -> byte offset in the weight blob; ptable: parameter name -> byte offset in the gradient buffer (backward ops
    only); cdt: dtype of the GEMM weights; z16: convolution outputs stored in ``cdt``; side: weight gradients on the side stream."""

    def __init__(self, table: Dict[str, int], B: int, cdt: int, ptable: Optional[Dict[str, int]] = None, h16: bool = False,
                 z16: bool = False, side: bool = False):
        self.table, self.ptable, self.B, self.cdt, self.h16, self.z16 = table, ptable, B, cdt, h16, z16
        self.ops, self.bufs, self.names = [], [], []
        self.lib = L.load()
        # weight gradients on the side stream (ftc_plan_run_streams): nothing on the backward chain reads them, so they overlap its
        # HBM-bound BatchNorm / depthwise passes.  An op's buffers stay allocated until the FTC_OP_JOIN after it (join()).
        self.side = side
        self.side_pending: List[int] = []

    def buf(self, nbytes: int) -> tuple:
        b = _Buf(nbytes)
        self.bufs.append(b)
        return ("ws", b, 0)

    def scratch(self) -> tuple:
        """A scratch operand of the op it is given to: emit() reserves what ftc_op_extents says that op touches through it."""
        return ("scratch",)

    def w(self, name: str):
        return ("w", self.table[name])

    def g(self, name: str):
        return ("g", self.ptable[name])

    @staticmethod
    def _fill(op, f: dict) -> None:
        """The int fields of an emitted op into the ftc_op; every operand it carries marked as given."""
        for k, v in f.items():
            if k not in L.REFS:
                setattr(op, k, int(v))
            elif v is not None:
                getattr(op, k).base = L.BASE_WORKSPACE

    def emit(self, _name: str = "", **f) -> dict:
        """Appends the op; returns its fields with every scratch() placeholder replaced by the buffer reserved for it."""
        idx = len(self.ops)
        if ("scratch",) in f.values():
            op = L.Op()
            self._fill(op, f)
            nbytes, _ = L.op_extents(op)
            f = {k: self.buf(nbytes[L.REFS.index(k)]) if v == ("scratch",) else v for k, v in f.items()}
        for v in f.values():
            if isinstance(v, tuple) and v[0] == "ws":
                v[1].first, v[1].last = min(v[1].first, idx), max(v[1].last, idx)
        self.ops.append(f)
        self.names.append(_name)
        return f

    def join(self) -> None:
        """FTC_OP_JOIN: the main stream waits for the side stream; every buffer a pending side op touches lives until here."""
        if not self.side_pending:
            return
        j = len(self.ops)
        self.ops.append(dict(kind=L.OP_JOIN, B=1, H=1, W=1, Ho=1, Wo=1))
        self.names.append("join")
        for i in self.side_pending:
            for v in self.ops[i].values():
                if isinstance(v, tuple) and v[0] == "ws":
                    v[1].last = max(v[1].last, j)
        self.side_pending = []

    def side_op(self) -> None:
        """The op emitted next goes to the side stream: registered for the next join (emitted first when the oldest pending op is far behind)."""
        if self.side_pending and len(self.ops) - self.side_pending[0] >= int(os.environ.get("FTC_TRAIN_JOIN_EVERY", "32")):      # bounds how long operands outlive their last main-stream use
            self.join()
        self.side_pending.append(len(self.ops))

    def pin(self, ref) -> None:
        ref[1].first, ref[1].last = 0, 1 << 29

    def pick(self, act):
        """(operand, dtype) a GEMM reads for activation `act` = (fp32, copy16)."""
        return (act[1], self.cdt) if act[1] is not None else (act[0], L.F32)

    # ---- forward pieces
    def conv(self, x, h, w, cin, wname, cout, k, stride=1, se=None, bias=None, out=None, cout_total=None, cout_off=0, B=None):
        B = B or self.B
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        zdt = self.cdt if (self.z16 and out is None and cout_total is None) else L.F32
        z = out if out is not None else self.buf(B * ho * wo * cout * (2 if zdt != L.F32 else 4))
        if out is None:
            z[1].dt = zdt                                     # the dtype travels with the buffer: BNSTAT / BNACT / BNBWD read it
        xin, xdt = self.pick(x)
        self.emit(wname, kind=L.OP_CONV, flags=L.FLAG_SE_SCALE if se is not None else 0, act=L.ACT_NONE, in_dtype=xdt, out_dtype=zdt,
                  w_dtype=self.cdt, B=B, H=h, W=w, Ho=ho, Wo=wo, Cin=cin, Cin_total=cin, Cout=cout, Cout_total=cout_total or cout,
                  cout_off=cout_off, ksize=k, stride=stride, res_dtype=L.F32, in_=xin, out=z, w=self.w(wname + "#f"), bias=bias or self.w("zeros"), scale=se)
        return z, ho, wo

    def bnstat(self, z, h, w, c, bn_name, eps, B=None):
        B = B or self.B
        ss = self.buf(4 * c * 4)                              # scale | shift | mean | 1/std (FTC_OP_BNSTAT)
        self.emit(bn_name, kind=L.OP_BNSTAT, in_dtype=getattr(z[1], "dt", L.F32), B=B, H=h, W=w, Cin=c, aux0=_fbits(eps), aux1=_fbits(0.1), in_=z, w=self.w(bn_name + ".weight"),
                  bias=self.w(bn_name + ".bias"), aux=self.w(bn_name + ".running"), out=ss, in2=self.scratch())
        return ss

    def bn(self, z, h, w, c, bn_name, eps, act, residual=None, keep=None, sums_p=0, B=None, want32=True, want16=True):
        """BatchNorm with batch statistics (+ activation, keep-scale * branch + residual, SE sums) on z [B,h,w,c]
        -> ((y fp32 | None, y 16-bit | None), SE partial sums, statistics block)"""
        B = B or self.B
        ss = self.bnstat(z, h, w, c, bn_name, eps, B)
        want16 = want16 and self.h16
        want32 = want32 or not want16
        M = B * h * w
        y32 = self.buf(M * c * 4) if want32 else None
        y16 = self.buf(M * c * 2) if want16 else None
        sums = self.buf(B * sums_p * c * 4) if sums_p else None
        # row chunks per image: few when the SE op has to read the partial sums, else enough workgroups to fill the GPU
        rows_p = sums_p if sums_p else max(1, min(2048, (h * w) // 64))
        self.emit(bn_name, kind=L.OP_BNACT, flags=L.FLAG_RESIDUAL if residual is not None else 0, act=act, in_dtype=getattr(z[1], "dt", L.F32),
                  out_dtype=L.F32 if want32 else self.cdt, w_dtype=L.F16 if self.cdt == L.F16 else L.BF16, res_dtype=L.F32, B=B, H=h, W=w, Cin=c,
                  aux0=rows_p, in_=z, scale=ss, shift=("ws", ss[1], c * 4), in2=residual, w2=keep, out=y32 if want32 else y16,
                  out2=y16 if (want32 and want16) else None, aux=sums)
        return (y32, y16), sums, ss

    # ---- backward pieces
    def bn_bwd(self, gy, z, ss, h, w, c, bn_name, act, keep=None, ga=None, gb=None, gy_total=0, gy_off=0, out=None, accum=False, B=None,
               want32=False, want16=True):
        """-> (dz fp32 | None, dz 16-bit | None): dz of a convolution's BatchNorm is read by that convolution's two GEMMs only."""
        B = B or self.B
        M = B * h * w
        want16 = want16 and self.h16 and out is None
        want32 = want32 or not want16 or out is not None
        d32 = out if out is not None else (self.buf(M * c * 4) if want32 else None)
        d16 = self.buf(M * c * 2) if want16 else None
        self.emit("bwd:" + bn_name, kind=L.OP_BNBWD, flags=L.FLAG_ACCUM if accum else 0, act=act, w_dtype=self.cdt, in_dtype=getattr(z[1], "dt", L.F32), B=B, H=h, W=w, Cin=c,
                  Cin_total=gy_total, cin_off=gy_off, in_=gy, in2=z, scale=ss, w2=keep, bias=ga, bias2=gb, out=d32, out2=d16,
                  w=self.g(bn_name + ".weight"), shift=self.g(bn_name + ".bias"), aux=self.scratch())
        return (d32, d16)

    def wgrad(self, x, dz, h, w, cin, cout, k, stride, wname, se=None, cin_total=0, cin_off=0, cout_total=0, cout_off=0, B=None):
        B = B or self.B
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        S = int(self.lib.ftc_wgrad_splits(B, ho, wo, cout, cin, k))
        if se is not None and k == 1 and stride == 1:
            # SE-gated input (the project convolution): splits that each lie inside ONE image let the kernel apply the gate to the
            # columns of the partial tile instead of to every staged element (FTC_OP_WGRAD does so when Ho*Wo % chunk == 0)
            kk = max(1, round(S / B))
            while kk > 1 and (ho * wo) % (kk * 64):
                kk -= 1
            if (ho * wo) % (kk * 64) == 0:
                S = B * kk
        xin, xdt = self.pick(x)
        din, ddt = self.pick(dz)
        if self.side:
            self.side_op()
        self.emit("wgrad:" + wname, kind=L.OP_WGRAD, flags=(L.FLAG_SE_SCALE if se is not None else 0) | (L.FLAG_SIDE_STREAM if self.side else 0), w_dtype=self.cdt, in_dtype=xdt, res_dtype=ddt, B=B, H=h,
                  W=w, Ho=ho, Wo=wo, Cin=cin, Cin_total=cin_total, cin_off=cin_off, Cout=cout, Cout_total=cout_total, cout_off=cout_off, ksize=k,
                  stride=stride, aux0=S, in_=xin, in2=din, scale=se, out=self.g(wname), aux=self.scratch())

    def dgrad(self, dz, ho, wo, cout, wname, cin, k, stride, h, w, add=None, cout_pad=None, B=None):
        """d input fp32 [B,h,w,cin] of a convolution whose d output is dz = (fp32, 16-bit) [B,ho,wo,cout] (+ add)."""
        B = B or self.B
        src, sdt = self.pick(dz)
        if stride == 2:                                            # (the two stride-2 dense convs: fp32 through the dilation)
            assert dz[0] is not None
            src, sdt = self.buf(B * h * w * cout * 4), L.F32
            self.emit("dilate:" + wname, kind=L.OP_DILATE, B=B, H=ho, W=wo, Ho=h, Wo=w, Cin=cout, in_=dz[0], out=src)
        dx = self.buf(B * h * w * cin * 4)
        cp = cout_pad or cout
        self.emit("dgrad:" + wname, kind=L.OP_CONV, flags=L.FLAG_RESIDUAL if add is not None else 0, act=L.ACT_NONE, in_dtype=sdt, out_dtype=L.F32,
                  w_dtype=self.cdt, B=B, H=h, W=w, Ho=h, Wo=w, Cin=cp, Cin_total=cp, Cout=cin, Cout_total=cin, ksize=k, stride=1, res_dtype=L.F32,
                  in_=src, out=dx, w=self.w(wname + "#d"), bias=self.w("zeros"), in2=add)
        return dx

    # ---- the plan
    def resolve(self) -> Tuple[C.Array, int]:
        """Liveness-based first-fit arena (as csrc/model.hip does for the inference plan; buffers in order of first use, ties in order of
        creation), then every operand as (base, byte offset) -> (ctypes op array, workspace bytes)."""
        n_ops = len(self.ops)
        order = sorted((b for b in self.bufs if b.last >= 0), key=lambda b: b.first)
        live: List[_Buf] = []
        top = 0
        for b in order:
            b.last = min(b.last, n_ops)
            live = [x for x in live if x.last >= b.first]
            off = 0
            for x in sorted(live, key=lambda x: x.offset):
                if off + b.nbytes <= x.offset:
                    break
                off = max(off, x.offset + x.nbytes)
            b.offset = off
            live.append(b)
            top = max(top, off + b.nbytes)
        ops = (L.Op * n_ops)()
        for i, f in enumerate(self.ops):
            self._fill(ops[i], f)
            nbytes, _ = L.op_extents(ops[i])
            for k, v in f.items():
                if k not in L.REFS or v is None:
                    continue
                r = getattr(ops[i], k)
                if v[0] == "ws":
                    r.base, r.offset = L.BASE_WORKSPACE, v[1].offset + v[2]
                    # the arena places buffers side by side: an operand that runs past the buffer reserved for it would run into a live neighbour
                    if v[2] + nbytes[L.REFS.index(k)] > v[1].nbytes:
                        raise RuntimeError(f"train plan: op {i} ({self.names[i]}): operand {k.rstrip('_')} spans {nbytes[L.REFS.index(k)]} bytes from offset "
                                           f"{v[2]} of a buffer of {v[1].nbytes}")
                elif v[0] == "w":
                    r.base, r.offset = L.BASE_WEIGHTS, v[1]
                elif v[0] == "g":
                    r.base, r.offset = L.BASE_GRADS, v[1]
                else:
                    r.base, r.offset = L.BASE_INPUT, 0
        return ops, top + 256


def emit_detector_forward(g: Builder, sh, B: int, H: int, W: int) -> dict:
    """Stem, backbone, head conv and the nine FPN heads of the image [B,H,W,3] fp32 (FTC_BASE_INPUT) -> maps [B,mh,mw,9] and feats
    [B,mh,mw,100] (fp32), the keep-scale table ``keep`` (rows = ``res_names``) and, for the backward, ``tape`` (one record per backbone
    layer), ``taps`` (the FPN inputs) and ``heads``.  The keep-scales and the maps stay allocated over the whole plan."""
    pre = "detector."
    P = pre + "backbone.features"
    res_names: List[str] = []
    keep_buf = g.buf(4096 * 4)                                   # [n residual blocks][B] fp32 keep-scales, filled before every run
    g.pin(keep_buf)
    adt = g.cdt if g.h16 else L.F32                              # dtype of the FPN level tensors (read by convolutions / the upsampler only)
    aes = 2 if g.h16 else 4
    tape: List[dict] = []
    taps = []
    heads = []
    c0 = sh[P + ".0.0.weight"][0]
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    z = g.buf(B * h * w * c0 * 4)
    g.emit("stem", kind=L.OP_STEM, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, B=B, H=H, W=W, Ho=h, Wo=w, Cin=3, Cout=c0, ksize=3, stride=2,
           in_=("in",), out=z, w=g.w(P + ".0.0.weight#stem"), bias=g.w("zeros"))
    x, _, ss = g.bn(z, h, w, c0, P + ".0.1", BACKBONE_EPS, L.ACT_SILU)
    tape.append(dict(kind="stem", z=z, ss=ss, h=h, w=w, c=c0, out=x))
    c = c0
    pending_tap = None
    i = 1
    while f"{P}.{i}.0.block.0.0.weight" in sh:
        j = 0
        while f"{P}.{i}.{j}.block.0.0.weight" in sh:
            p = f"{P}.{i}.{j}"
            b = p + ".block"
            stride = _STAGE_STRIDE[i] if j == 0 else 1
            mb = f"{b}.2.fc1.weight" in sh
            fused4 = (not mb) and f"{b}.1.0.weight" in sh
            last = ".3" if mb else (".1" if fused4 else ".0")
            cout = sh[b + last + ".0.weight"][0]
            residual = x[0] if (stride == 1 and c == cout) else None
            keep = None
            if residual is not None:
                keep = ("ws", keep_buf[1], len(res_names) * _align(B, 4) * 4)       # rows padded to 16 bytes (operand alignment)
                res_names.append(p[len(pre):])
            rec = dict(b=b, xin=x, h=h, w=w, c=c, cout=cout, stride=stride, residual=residual is not None, keep=keep)
            if pending_tap is not None:                              # this block reads a tap: the heads' gradient of the tap joins its data gradient
                rec["xin_tap"], pending_tap = pending_tap, None
            if mb:
                e = sh[b + ".0.0.weight"][0]
                z0, _, _ = g.conv(x, h, w, c, b + ".0.0.weight", e, 1)
                y0, _, ss0 = g.bn(z0, h, w, e, b + ".0.1", BACKBONE_EPS, L.ACT_SILU, **F32ONLY)       # read by the fp32 depthwise kernels
                ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
                th = 8 if stride == 1 else 4
                pdw = -(-ho // th) * -(-wo // 8)
                zd = g.buf(B * ho * wo * e * 4)
                g.emit(b + ".1.0", kind=L.OP_DWCONV, act=L.ACT_NONE, in_dtype=L.F32, out_dtype=L.F32, B=B, H=h, W=w, Ho=ho, Wo=wo, Cin=e, Cout=e, ksize=3,
                       stride=stride, aux0=pdw, in_=y0[0], out=zd, w=g.w(b + ".1.0.weight#dw"), bias=g.w("zeros"), aux=g.scratch())
                pse = max(1, min(16, (ho * wo) // 64))
                y1, sums, ss1 = g.bn(zd, ho, wo, e, b + ".1.1", BACKBONE_EPS, L.ACT_SILU, sums_p=pse)                 # fp32 for the SE backward + copy
                s = sh[b + ".2.fc1.weight"][0]
                sc = g.buf(B * e * 4)
                g.emit(b + ".2", kind=L.OP_SE, B=B, H=ho, W=wo, Cin=e, Cout=e, aux0=s, aux1=pse, aux=sums, out=sc, in2=g.scratch(),
                       w=g.w(b + ".2.fc1.weight"), w2=g.w(b + ".2.fc2.weight#t"), bias=g.w(b + ".2.fc1.bias"), bias2=g.w(b + ".2.fc2.bias"))
                z3, _, _ = g.conv(y1, ho, wo, e, b + ".3.0.weight", cout, 1, se=sc)
                x, _, ss3 = g.bn(z3, ho, wo, cout, b + ".3.1", BACKBONE_EPS, L.ACT_NONE, residual=residual, keep=keep)
                rec.update(kind="mb", e=e, z0=z0, y0=y0, ss0=ss0, zd=zd, y1=y1, ss1=ss1, sums=sums, pse=pse, s=s, sc=sc, z3=z3, ss3=ss3, ho=ho, wo=wo)
                h, w = ho, wo
            elif fused4:
                e = sh[b + ".0.0.weight"][0]
                z0, ho, wo = g.conv(x, h, w, c, b + ".0.0.weight", e, 3, stride)
                y0, _, ss0 = g.bn(z0, ho, wo, e, b + ".0.1", BACKBONE_EPS, L.ACT_SILU, **GEMM_ONLY)
                z1, _, _ = g.conv(y0, ho, wo, e, b + ".1.0.weight", cout, 1)
                x, _, ss1 = g.bn(z1, ho, wo, cout, b + ".1.1", BACKBONE_EPS, L.ACT_NONE, residual=residual, keep=keep)
                rec.update(kind="f4", e=e, z0=z0, y0=y0, ss0=ss0, z1=z1, ss1=ss1, ho=ho, wo=wo)
                h, w = ho, wo
            else:
                z0, ho, wo = g.conv(x, h, w, c, b + ".0.0.weight", cout, 3, stride)
                x, _, ss0 = g.bn(z0, ho, wo, cout, b + ".0.1", BACKBONE_EPS, L.ACT_SILU, residual=residual, keep=keep)
                rec.update(kind="f1", z0=z0, ss0=ss0, ho=ho, wo=wo)
                h, w = ho, wo
            rec["out"] = x
            tape.append(rec)
            c = cout
            j += 1
        if i in (2, 3, 5):
            taps.append((x[0], c, h, w))
            pending_tap = len(taps) - 1
        i += 1
    cl = sh[f"{P}.{i}.0.weight"][0]
    zl, _, _ = g.conv(x, h, w, c, f"{P}.{i}.0.weight", cl, 1)
    xl, _, ssl = g.bn(zl, h, w, cl, f"{P}.{i}.1", BACKBONE_EPS, L.ACT_SILU, **F32ONLY)               # the last tap: read by the heads' fp32 tap path only
    hc = dict(kind="headconv", name=f"{P}.{i}", xin=x, z=zl, ss=ssl, h=h, w=w, c=c, cout=cl, out=xl, tap=len(taps))
    if pending_tap is not None:
        hc["xin_tap"], pending_tap = pending_tap, None
    tape.append(hc)
    taps.append((xl[0], cl, h, w))
    mh, mw = taps[0][2], taps[0][3]
    maps = g.buf(B * mh * mw * 9 * 4)
    feats = g.buf(B * mh * mw * 100 * 4)
    g.pin(maps)
    ch = 0
    n = len(taps)
    for name in HEAD_NAMES + ["feature"]:
        hp = pre + name
        y, cy, yh, yw = None, 0, 0, 0
        levels = []
        for lvl, (tx, tc, th_, tw_) in enumerate(reversed(taps)):
            ti = n - 1 - lvl
            # the head's input BatchNorm of the tap: statistics here, the affine applied by the upsample+concat kernel
            ssi = g.bnstat(tx, th_, tw_, tc, f"{hp}.in_bn.{ti}", HEAD_EPS)
            catb = g.buf(B * th_ * tw_ * (cy + tc) * aes)
            cat = (None, catb) if g.h16 else (catb, None)
            g.emit(f"{hp}.upcat.{lvl}", kind=L.OP_UPCAT, in_dtype=adt, out_dtype=adt, res_dtype=L.F32, B=B, H=yh if y is not None else th_,
                   W=yw if y is not None else tw_, Ho=th_, Wo=tw_, Cin=cy + tc, Cout=cy + tc, aux0=cy, aux1=tc, in_=g.pick(y)[0] if y is not None else None,
                   in2=tx, out=catb, scale=ssi, shift=("ws", ssi[1], tc * 4))
            cm = sh[f"{hp}.upsamplers.{lvl}.0.weight"][0]
            zc, _, _ = g.conv(cat, th_, tw_, cy + tc, f"{hp}.upsamplers.{lvl}.0.weight", cm, 3)
            yn, _, ssc = g.bn(zc, th_, tw_, cm, f"{hp}.upsamplers.{lvl}.1", HEAD_EPS, L.ACT_GELU, **GEMM_ONLY)
            levels.append(dict(lvl=lvl, ti=ti, tx=tx, tc=tc, h=th_, w=tw_, cy=cy, yh=yh, yw=yw, ssi=ssi, cat=cat, cm=cm, z=zc, ss=ssc, y=yn))
            y, cy, yh, yw = yn, cm, th_, tw_
        co = sh[f"{hp}.top_conv.0.weight"][0]
        if name == "feature":
            g.conv(y, yh, yw, cy, f"{hp}.top_conv.0.weight", co, 3, bias=g.w(f"{hp}.top_conv.0.bias"), out=feats)
            heads.append(dict(hp=hp, levels=levels, co=co, ch=None, y=y, cy=cy))
        else:
            g.conv(y, yh, yw, cy, f"{hp}.top_conv.0.weight", co, 3, bias=g.w(f"{hp}.top_conv.0.bias"), out=maps, cout_total=9, cout_off=ch)
            heads.append(dict(hp=hp, levels=levels, co=co, ch=ch, y=y, cy=cy))
            ch += co
    return dict(tape=tape, taps=taps, heads=heads, maps=maps, feats=feats, keep=keep_buf, res_names=res_names, mh=mh, mw=mw)


def emit_decoder_forward(g: Builder, sh, rows, n: int) -> List[dict]:
    """The SimpleDecoder on the activation `rows` [n,128] (the gathered feature rows, zero-padded from 100): per block Linear, BatchNorm1d,
    GELU twice, then the Linear to the logits -> one record per block, ``out`` = its logits [n, cout] fp32."""
    dec = []
    jb = 0
    while f"decoder.blocks.{jb}.0.weight" in sh:
        bq = f"decoder.blocks.{jb}"
        yq, cq = rows, 128
        lay = []
        for li, bi in ((0, 1), (3, 4)):
            coq = sh[f"{bq}.{li}.weight"][0]
            zq, _, _ = g.conv(yq, n, 1, cq, f"{bq}.{li}.weight", coq, 1, B=1)
            yn, _, ssq = g.bn(zq, n, 1, coq, f"{bq}.{bi}", HEAD_EPS, L.ACT_GELU, B=1, **GEMM_ONLY)
            lay.append(dict(x=yq, cin=cq, z=zq, ss=ssq, y=yn, cout=coq, wname=f"{bq}.{li}.weight", bn=f"{bq}.{bi}"))
            yq, cq = yn, coq
        coq = sh[f"{bq}.6.weight"][0]
        oq = g.buf(n * coq * 4)
        g.conv(yq, n, 1, cq, f"{bq}.6.weight", coq, 1, bias=g.w(f"{bq}.6.bias"), out=oq, B=1)
        dec.append(dict(b=bq, lay=lay, x=yq, cin=cq, out=oq, cout=coq))
        jb += 1
    return dec
