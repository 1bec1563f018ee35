"""Runs tests/c_abi/train_choice_host.cc -- plain C++ over csrc/train_choice.h alone, its own main, built with AddressSanitizer + UBSan -- on ops given as
field dicts and returns what the resolvers of FTC_OP_BNSTAT, BNACT, BNBWD, DWBWD and SEBWD answer.  No GPU and no library needed.  This module holds no
tests: tests/test_abi_and_plan.py, test_bn_operands_host.py, test_se_operands_host.py and test_exact_operands_host.py use it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_FIELDS = [n for n, t in L.Op._fields_ if t is C.c_int32]
REF_FIELDS = [n for n, t in L.Op._fields_ if t is L.Ref]
LETTER = {L.OP_BNSTAT: "n", L.OP_BNACT: "a", L.OP_BNBWD: "b", L.OP_DWBWD: "d", L.OP_SEBWD: "e"}


_EXE = []


def build(dirpath):
    """The program, built into `dirpath` by the first caller of the process (a module fixture hands in a pytest temporary directory)."""
    if not _EXE:
        out = os.path.join(str(dirpath), "train_choice_host")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "c_abi", "train_choice_host.cc"), "-o", out], check=True)
        _EXE.append(out)
    return run


def host_line(f, letter=None):
    """The request line of an op: `f` maps int field names to values; "_refs" names the operands that are given (Op field names: in_, in2, out, ...)."""
    mask = sum(1 << REF_FIELDS.index(r) for r in f.get("_refs", ()))
    return f"{letter or LETTER[f['kind']]} " + " ".join(str(int(f.get(n, 0))) for n in INT_FIELDS) + f" {mask}"


def _parse(part):
    out = {}
    for kv in part.split():
        k, v = kv.split("=")
        if k in out:                                        # (DWBWD prints a Q per half)
            k = "w" + k
        out[k] = tuple(int(x) for x in v.split(",")) if "," in v else int(v) if v.lstrip("-").isdigit() else v
    return out


def run(ops, letter=None, env=None):
    """One answer per op: (refusal or "", label, what selects the instantiation as a dict, what sizes the launch as a dict)."""
    e = {k: v for k, v in os.environ.items() if k not in ("FTC_BNACT_SCALAR", "FTC_DWBWD_DATA_OLD")}
    e.update(env or {})
    r = subprocess.run([_EXE[0]], input="".join(host_line(f, letter) + "\n" for f in ops), capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line.split("\t") for line in r.stdout.split("\n")[:-1]]
    assert len(lines) == len(ops) and all(len(line) == 4 for line in lines)
    return [(why, lab, _parse(inst), _parse(launch)) for why, lab, inst, launch in lines]


# ---- ops as the GPU modules build them ---------------------------------------------------------------------------------------------------------

def bnstat(shape, idt=L.F32):
    B, H, W, Cc = shape
    return dict(kind=L.OP_BNSTAT, in_dtype=idt, B=B, H=H, W=W, Cin=Cc, _refs=("in_", "out", "w", "bias", "in2"))


def bnact(shape, idt, odt, tc, P=1, res=None, out2=False):
    B, H, W, Cc = shape
    return dict(kind=L.OP_BNACT, in_dtype=idt, out_dtype=odt, w_dtype=tc, res_dtype=L.F32 if res is None else res, flags=0 if res is None else L.FLAG_RESIDUAL, B=B, H=H, W=W,
                Cin=Cc, aux0=P, _refs=("in_", "out", "scale", "shift", "aux") + (("in2",) if res is not None else ()) + (("out2",) if out2 else ()))


def bnbwd(shape, wd, zdt, outputs="out", accum=False):
    B, H, W, Cc = shape
    return dict(kind=L.OP_BNBWD, in_dtype=zdt, w_dtype=wd, flags=L.FLAG_ACCUM if accum else 0, B=B, H=H, W=W, Cin=Cc,
                _refs=("in_", "in2", "scale", "aux") + {"out": ("out",), "out2": ("out2",), "both": ("out", "out2")}[outputs])


def dwbwd(shape, stride, halves="both"):
    B, H, W, Cc = shape
    return dict(kind=L.OP_DWBWD, B=B, H=H, W=W, Ho=(H - 1) // stride + 1, Wo=(W - 1) // stride + 1, Cin=Cc, stride=stride,
                _refs=("in2",) + (("out", "w") if halves in ("both", "data") else ()) + (("out2", "in_", "aux") if halves in ("both", "weight") else ()))


def sebwd(shape, S, P=1):
    B, H, W, Cc = shape
    return dict(kind=L.OP_SEBWD, B=B, H=H, W=W, Cin=Cc, aux0=S, aux1=P, _refs=("in_", "in2", "scale", "aux", "w", "w2", "bias", "out", "out2"))
