"""The recorded output of plan construction and weight packing (csrc/plan.hip, csrc/pack.hip): every ftc_op of every plan the library builds for a
set of (model size, numeric mode, batch, plan switch) cases, the packed weight blob as chunk hashes, and the decoder workspace sizes -- all
host-side, no GPU needed.  If these are equal, the GPU executes the same launches on the same data.

    python tests/plan_sweep.py --write        # rewrites tests/golden/model_plans.json.gz from the library in the tree

The file is a gzip of JSON:
  {"ops": [record, ...],                                      every distinct op record once
   "plans": {case: {"ops": [index into "ops", ...], "info": [workspace, weights, peak live, total buffer bytes, map_h, map_w]}},
   "weights": {case: {"bytes": n, "chunks": [sha256 of each 1 MiB chunk of ftc_weights_host, ...]}},
   "decoder": {mode: {"decoder": {rows: bytes}, "glyph": {rows: bytes}}}}
An op record is the 24 int fields of ftc_op, then (base, reserved, offset) of its eleven refs, then name, kind, flops and bytes (the doubles as
float.hex()): RECORD_FIELDS names the positions.  tests/test_abi_and_plan.py replays every case and compares field by field.
"""
import gzip
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from findtextcenternet_amd import _lib as L            # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "model_plans.json.gz")
INTS = [n for n, _ in L.Op._fields_[:24]]
REFS = [n for n, _ in L.Op._fields_[24:]]
RECORD_FIELDS = INTS + [f"{r}.{p}" for r in REFS for p in ("base", "reserved", "offset")] + ["name", "kind", "flops", "bytes"]
INFO_FIELDS = ("workspace_bytes", "weights_bytes", "peak_live_bytes", "total_buffer_bytes", "map_h", "map_w")
MODES = ("fp32", "bf16", "fp16", "fp16x3")
MODES3 = ("fp32", "bf16", "fp16x3")
# every switch of plan construction ("Where a plan is decided, and its switches") with the value that turns it away from its default
SWITCHES = [("FTC_NO_MBSLICE", "1"), ("FTC_NO_MBSLICE_X3", "1"), ("FTC_NO_MBBAND", "1"), ("FTC_MBSLICE_96", "0"), ("FTC_MBSLICE_MINWG", "1000000"),
            ("FTC_NO_FMBFUSE", "1"), ("FTC_NO_FMBFUSE_X3", "1"), ("FTC_FMBFUSE_ALL", "1"), ("FTC_NO_KBLOCK", "1"), ("FTC_NO_X3FOLD", "1"),
            ("FTC_NO_PRESPLIT", "1"), ("FTC_NO_TOPFUSE", "1"), ("FTC_NO_TOPFUSE32", "1"), ("FTC_NO_UPFUSE", "1"), ("FTC_NO_UPFUSE32", "1"),
            ("FTC_NO_UPFUSE32_L2", "1"), ("FTC_NO_BNFOLD", "1"), ("FTC_NO_BNFOLD32", "1"), ("FTC_NO_WL1", "1"), ("FTC_NO_TUNING", "1")]
SAME_AS_DEFAULT = [("FTC_NO_MBSLICE", "0"), ("FTC_NO_MBSLICE", "")]          # env_on: "0" and the empty string are off
SWITCH_B = 8
DECODER_ROWS = (1, 100, 2048, 8192)
GLYPH_ROWS = (1, 64, 65, 97, 5000)


def case_name(size, mode, B, H, W, nchw=False, env=None):
    return f"{size}_{mode}_b{B}_{H}x{W}" + ("_nchw" if nchw else "") + "".join(f"_{k}={v}" for k, v in (env or {}).items())


def plan_cases():
    """[(name, size, mode, B, H, W, nchw, env)]"""
    out = [("xl", mode, B, 768, 768, False, {}) for mode in MODES for B in (1, 2, 8, 32)]
    out.append(("xl", "bf16", 8, 768, 768, True, {}))
    out += [(size, mode, 2, 128, 160, False, {}) for size in ("s", "m", "l", "xl") for mode in MODES3]
    out += [("xl", mode, SWITCH_B, 768, 768, False, {k: v}) for k, v in SWITCHES for mode in MODES3]
    out += [("xl", mode, 2, 768, 768, False, {"FTC_MBSLICE_MINWG": "1"}) for mode in MODES3]
    out += [("xl", "bf16", 8, 768, 768, False, {k: v}) for k, v in SAME_AS_DEFAULT]
    return [(case_name(*c), *c) for c in out]


def weight_cases():
    """[(name, size, mode, with_decoder)]"""
    return [(f"xl_{mode}", "xl", mode, True) for mode in MODES] + [(f"{size}_{mode}", size, mode, False) for size in ("s", "m", "l") for mode in MODES3]


class Models:
    """The seeded models by (size, mode): xl with the decoder, the others without.  fresh=True: never reuse one for two plan cases (a library whose
    plan cache ignores the switches)."""

    def __init__(self, given=None):
        self.sd, self.m = {}, dict(given or {})

    def state_dict(self, size):
        from findtextcenternet_amd.weights import deterministic_state_dict
        if size not in self.sd:
            # (only the prefixed form of the seeded checkpoint carries the decoder.* tensors; ftc_create strips "detector.")
            self.sd[size] = deterministic_state_dict(0, model_size=size, with_decoder=True) if size == "xl" else \
                deterministic_state_dict(0, model_size=size, prefix_detector=False)
        return self.sd[size]

    def get(self, size, mode, fresh=False):
        from findtextcenternet_amd.model import FtcModel
        if fresh:
            return FtcModel(self.state_dict(size), mode, size)
        if (size, mode) not in self.m:
            self.m[(size, mode)] = FtcModel(self.state_dict(size), mode, size)
        return self.m[(size, mode)]


def plan_record(model, B, H, W, nchw, env):
    """{"ops": [record], "info": [...]} of one plan built with `env` set."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pl = model.plan(B, H, W, nchw=nchw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    ops = []
    for o, me in zip(pl.ops, pl.meta):
        rec = [int(getattr(o, n)) for n in INTS]
        for r in REFS:
            ref = getattr(o, r)
            rec += [int(ref.base), int(ref.reserved), int(ref.offset)]
        ops.append(rec + [me.name, me.kind, me.flops.hex(), me.bytes.hex()])
    return {"ops": ops, "info": [int(getattr(pl.info, n)) for n in INFO_FIELDS]}


def weight_record(model):
    blob = memoryview(model.weights_host())
    step = 1 << 20
    return {"bytes": model.weights_bytes, "chunks": [hashlib.sha256(blob[i:i + step]).hexdigest() for i in range(0, len(blob), step)]}


def decoder_record(model):
    lib = L.load()
    return {"decoder": {str(n): int(lib.ftc_decoder_workspace_bytes(model.handle, n)) for n in DECODER_ROWS},
            "glyph": {str(n): int(lib.ftc_glyph_decode_workspace_bytes(model.handle, n)) for n in GLYPH_ROWS}}


def replay(models=None, fresh=False, verbose=False):
    """Everything the golden holds, from the library in the tree, with the op records written out (not indexed)."""
    ms = models if isinstance(models, Models) else Models(models)
    doc = {"plans": {}, "weights": {}, "decoder": {}}
    t0 = time.time()
    for name, size, mode, B, H, W, nchw, env in plan_cases():
        doc["plans"][name] = plan_record(ms.get(size, mode, fresh=fresh and bool(env)), B, H, W, nchw, env)
        if verbose:
            print(f"[{time.time() - t0:6.1f} s] {name}: {len(doc['plans'][name]['ops'])} ops", flush=True)
    for name, size, mode, _ in weight_cases():
        doc["weights"][name] = weight_record(ms.get(size, mode))
    for mode in MODES:
        doc["decoder"][mode] = decoder_record(ms.get("xl", mode))
    return doc


def decoder_sizes_missing(doc):
    """Decoder cases without a positive workspace size: a model without the decoder answers -1, which would compare nothing."""
    return [f"{mode}/{which}/{rows}" for mode, d in doc["decoder"].items() for which in ("decoder", "glyph") for rows, n in d[which].items() if n <= 0]


def idle_switches(doc):
    """Switches whose plan equals the default plan of the same mode and batch in all three modes: such a case would prove nothing."""
    return [f"{k}={v}" for k, v in SWITCHES
            if all(doc["plans"][case_name("xl", mode, SWITCH_B, 768, 768, False, {k: v})] == doc["plans"][case_name("xl", mode, SWITCH_B, 768, 768)] for mode in MODES3)]


def load_golden():
    """The golden with the op indices of every plan replaced by the records: the same structure replay() returns."""
    with gzip.open(GOLDEN, "rt") as f:
        doc = json.load(f)
    ops = doc.pop("ops")
    for p in doc["plans"].values():
        p["ops"] = [ops[i] for i in p["ops"]]
    return doc


def first_difference(want, got, part):
    """None, or a text that names the case and, in a plan, the op index and the field of the first difference between two replay() documents
    in part "plans", "weights" or "decoder"."""
    for name, w in want[part].items():
        g = got[part].get(name)
        if g is None:
            return f"{part} {name}: missing"
        if part == "plans":
            if len(w["ops"]) != len(g["ops"]):
                return f"plan {name}: {len(g['ops'])} ops, recorded {len(w['ops'])}"
            for i, (a, b) in enumerate(zip(w["ops"], g["ops"])):
                for field, x, y in zip(RECORD_FIELDS, a, b):
                    if x != y:
                        return f"plan {name}: op {i} ({a[-4]}): {field} = {y!r}, recorded {x!r}"
            for field, x, y in zip(INFO_FIELDS, w["info"], g["info"]):
                if x != y:
                    return f"plan {name}: {field} = {y}, recorded {x}"
        elif part == "weights":
            if w["bytes"] != g["bytes"]:
                return f"weights {name}: {g['bytes']} bytes, recorded {w['bytes']}"
            for i, (x, y) in enumerate(zip(w["chunks"], g["chunks"])):
                if x != y:
                    return f"weights {name}: the MiB chunk {i} differs (find the tensor by the ops' weight offsets)"
        else:
            for which in ("decoder", "glyph"):
                for rows, x in w[which].items():
                    if g[which][rows] != x:
                        return f"decoder {name}: {which} workspace for {rows} rows = {g[which][rows]}, recorded {x}"
    return None


def write_golden():
    doc = replay(fresh=True, verbose=True)
    idle = idle_switches(doc)
    if idle:
        raise SystemExit(f"refusing to write: {idle} change no plan at batch {SWITCH_B} in any of {MODES3}")
    if decoder_sizes_missing(doc):
        raise SystemExit(f"refusing to write: no decoder workspace size for {decoder_sizes_missing(doc)}")
    for k, v in SAME_AS_DEFAULT:
        assert doc["plans"][case_name("xl", "bf16", 8, 768, 768, False, {k: v})] == doc["plans"][case_name("xl", "bf16", 8, 768, 768)], (k, v)
    index, n = {}, 0
    for p in doc["plans"].values():
        n += len(p["ops"])
        p["ops"] = [index.setdefault(json.dumps(r), len(index)) for r in p["ops"]]
    doc["ops"] = [json.loads(r) for r in index]
    with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(doc['plans'])} plans, {n} ops ({len(index)} distinct), "
          f"{sum(len(w['chunks']) for w in doc['weights'].values())} weight chunks")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write_golden()
    else:
        print(__doc__)
