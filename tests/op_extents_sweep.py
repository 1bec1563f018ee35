"""What plan creation enforces about an op's eleven operands, and what the train-graph builder makes of it -- recorded on the CPU, no GPU needed,
from the commit BEFORE csrc/op_extents.h (when validate_op, the Python builder and TrainStep._grad_write_extents each stated the extents on their own).  Parts:

  verdicts  (a) whether ftc_plan_create accepts the one-op plan, or the exact message, for every distinct op (its 24 int fields and which operands are
            given) of three sets: "inference" the recorded inference plans (tests/golden/model_plans.json.gz), "train" the six train plans of
            tests/train_plan_choices.py, "cases" the ops of the GPU suites' case tables as the three choice sweeps enumerate them (backbone_choice_sweep
            part "cases", conv_choice_sweep parts "table", "fuzz" and "special", wgrad_choice_sweep part "cases")
  mutants   (b) single-fault mutants of every accepted op of (a) (FTC_OP_CONV ops that differ in the hint aux0 alone count once).  Per operand, in the order
            of REF_FIELDS: a GIVEN operand set to null; at offset 8 (misaligned); alone in the weights base at offset 256 with weights_bytes one byte short
            of its end (refused) and exactly at its end (accepted) -- the end is found by bisection over ftc_plan_create, so `flip` is the number of bytes
            the validator holds the operand to (1 = only the start is checked; 0 = given, but the op's form does not examine it).  An operand that is NOT given gets the base id 99: accepted = the op's
            form does not use it.
  plans     (c) every int field, base and offset of every op of the six train plans, workspace_bytes and n_fwd
  segments  (d) TrainStep._bucket_segments of each train plan for synthetic bucket ranges (BUCKETS: the flat gradient buffer cut into k equal ranges,
            first to last and last to first)

    python tests/op_extents_sweep.py --write        # rewrites tests/golden/op_extents.json.gz from the library in the tree

The file is a gzip of JSON: {"errors": [...], "verdicts": {set: {"n": count, "sha256": of the op keys, "err": [-1 | error index, ...]}},
"mutants": {"n": ..., "sha256": ..., "rows": [[per operand: [null, misaligned, flip, one short] | [base id 99]], ...]},
"records": [distinct op record, ...], "plans": {case: {"ops": [record index, ...], "workspace_bytes": n, "n_fwd": n}}, "segments": {case: {name: [[first, last,
bucket | null], ...]}}}.  tests/test_op_extents_host.py replays all of it.
"""
import ctypes as C
import gzip
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from findtextcenternet_amd import _lib as L            # noqa: E402
import plan_sweep as P                                 # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "op_extents.json.gz")
INT_FIELDS, REF_FIELDS = P.INTS, P.REFS
REF_NAMES = [r.rstrip("_") for r in REF_FIELDS]            # as the messages name them
SETS = ("inference", "train", "cases")
BIG = 1 << 44
PROBE_OFFSET = 256
BAD_BASE = 99
BUCKETS = (1, 3, 7, 16)


# ---- ops --------------------------------------------------------------------------------------------------------------------------------

def key_of(o):
    """(24 int fields, operand mask) of an ftc_op."""
    return tuple([int(getattr(o, n)) for n in INT_FIELDS] + [sum(1 << j for j, r in enumerate(REF_FIELDS) if getattr(o, r).base != L.BASE_NULL)])


def make_op(key):
    """ftc_op from a key; every operand it carries sits at offset 0 of a workspace taken to be large enough."""
    op = (L.Op * 1)()
    for n, v in zip(INT_FIELDS, key):
        setattr(op[0], n, v)
    for j, r in enumerate(REF_FIELDS):
        if key[-1] >> j & 1:
            getattr(op[0], r).base = L.BASE_WORKSPACE
    return op


def verdict(op, weights_bytes=BIG):
    """None when ftc_plan_create accepts the one-op plan, else the full error text."""
    lib = L.load()
    h = C.c_void_p()
    if lib.ftc_plan_create(op, 1, BIG, weights_bytes, C.byref(h)) == 0:
        lib.ftc_plan_destroy(h)
        return None
    return lib.ftc_last_error().decode()


def distinct(keys):
    return list(dict.fromkeys(keys))


def digest(keys):
    return hashlib.sha256(json.dumps([list(k) for k in keys], separators=(",", ":")).encode()).hexdigest()


def inference_keys():
    with gzip.open(P.GOLDEN, "rt") as fh:
        recs = json.load(fh)["ops"]
    n = len(INT_FIELDS)
    return distinct(tuple(r[:n] + [sum(1 << j for j in range(len(REF_FIELDS)) if r[n + 3 * j] != L.BASE_NULL)]) for r in recs)


def case_keys():
    import backbone_choice_sweep as BS
    import conv_choice_sweep as CS
    import wgrad_choice_sweep as WS
    keys = [key_of(BS.make_op(f)[0]) for _, _, f in BS.case_entries()]
    keys += [key_of(CS.make_op(dict(f, aux0=a))[0]) for part in ("table", "fuzz", "special") for f, a in CS.entries(part)]
    keys += [key_of(WS.make_op(f)[0]) for f in WS.entries("cases")]
    return distinct(keys)


# ---- the six train plans ------------------------------------------------------------------------------------------------------------------

class _Ranges:
    def __init__(self, ranges):
        self.ranges = ranges


def bucket_ranges(n_elems):
    """{name: [(first element, one past the last), ...]} -- the flat gradient buffer in k equal ranges, in both orders."""
    out = {}
    for k in BUCKETS:
        cuts = [n_elems * i // k for i in range(k + 1)]
        out[f"{k}_up"] = [(cuts[i], cuts[i + 1]) for i in range(k)]
        out[f"{k}_down"] = out[f"{k}_up"][::-1]
    return out


def train_plans():
    """{case: (TrainStep, plan)} of train_plan_choices.CASES."""
    import train_plan_choices as T
    from findtextcenternet_amd import TextDetectorModel, TrainStep
    model = TextDetectorModel(pre_weights=False, precision="fp32").train()
    out = {}
    for c in T.CASES:
        ts = TrainStep(model, c[0])
        out[T.case_name(*c)] = (ts, ts.plan_for(*c[1:]))
    return out


def plan_record(plan):
    ops = []
    for i in range(plan["n_ops"]):
        o = plan["ops"][i]
        ops.append([int(getattr(o, n)) for n in INT_FIELDS] + [int(v) for r in REF_FIELDS for v in (getattr(o, r).base, getattr(o, r).offset)])
    return {"ops": ops, "workspace_bytes": int(plan["workspace_bytes"]), "n_fwd": int(plan["n_fwd"])}


def segments(ts, plan):
    out = {}
    for name, ranges in bucket_ranges(ts.n_param_bytes // 4).items():
        ts.ddp = _Ranges(ranges)
        out[name] = [[a, b, bi] for a, b, bi in ts._bucket_segments(plan)]
    del ts.ddp
    return out


def train_keys(plans):
    return distinct(key_of(plan["ops"][i]) for _, plan in plans.values() for i in range(plan["n_ops"]))


# ---- (a), (b) ------------------------------------------------------------------------------------------------------------------------------------

def mutant_keys(accepted):
    """The accepted ops the mutants are made of: distinct, FTC_OP_CONV ops that differ in aux0 alone once (the first accepted one)."""
    a0 = INT_FIELDS.index("aux0")
    seen = {}
    for k in accepted:
        seen.setdefault(k[:a0] + (0,) + k[a0 + 1:] if k[0] == L.OP_CONV else k, k)
    return list(seen.values())


def flip_point(op, ref):
    """Smallest weights_bytes at which the plan is accepted with `ref` alone in the weights base at PROBE_OFFSET, less PROBE_OFFSET."""
    ref.base, ref.offset = L.BASE_WEIGHTS, PROBE_OFFSET
    assert verdict(op, BIG) is None
    if verdict(op, PROBE_OFFSET) is None:                    # given, but the op's form does not use it: not examined at all
        return 0
    lo, hi = PROBE_OFFSET, BIG                               # refused at lo, accepted at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if verdict(op, mid) is None:
            hi = mid
        else:
            lo = mid
    return hi - PROBE_OFFSET


def mutants(key):
    """Per operand [null, misaligned, flip, one byte short] (given) or [base id 99] (not given); a verdict is None or the error text."""
    rows = []
    for j, r in enumerate(REF_FIELDS):
        op = make_op(key)
        ref = getattr(op[0], r)
        if key[-1] >> j & 1:
            ref.base = L.BASE_NULL
            null = verdict(op)
            ref.base, ref.offset = L.BASE_WORKSPACE, 8
            mis = verdict(op)
            flip = flip_point(op, ref)
            short = verdict(op, PROBE_OFFSET + flip - 1) if flip else None
            assert (short is not None or not flip) and verdict(op, PROBE_OFFSET + flip) is None
            rows.append([null, mis, flip, short])
        else:
            ref.base = BAD_BASE
            rows.append([verdict(op)])
    return rows


def replay_verdicts(keys):
    return [verdict(make_op(k)) for k in keys]


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def write_golden():
    errors = {}
    enc = lambda e: -1 if e is None else errors.setdefault(e, len(errors))      # noqa: E731
    plans = train_plans()
    keys = {"inference": inference_keys(), "train": train_keys(plans), "cases": case_keys()}
    doc = {"verdicts": {}, "plans": {}, "segments": {}}
    accepted = []
    for s in SETS:
        got = replay_verdicts(keys[s])
        doc["verdicts"][s] = {"n": len(keys[s]), "sha256": digest(keys[s]), "err": [enc(e) for e in got]}
        accepted += [k for k, e in zip(keys[s], got) if e is None]
        print(f"verdicts/{s}: {len(got)} ops, {sum(e is None for e in got)} accepted", flush=True)
    mk = mutant_keys(distinct(accepted))
    rows = []
    for k in mk:
        rows.append([[enc(v) if i != 2 else v for i, v in enumerate(row)] for row in mutants(k)])
    doc["mutants"] = {"n": len(mk), "sha256": digest(mk), "rows": rows}
    print(f"mutants: {len(mk)} ops, {sum(len(r) == 4 for row in rows for r in row)} given operands", flush=True)
    index = {}
    for case, (ts, plan) in plans.items():
        rec = plan_record(plan)
        rec["ops"] = [index.setdefault(json.dumps(r), len(index)) for r in rec["ops"]]
        doc["plans"][case] = rec
        doc["segments"][case] = segments(ts, plan)
    doc["records"] = [json.loads(r) for r in index]
    doc["errors"] = list(errors)
    with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes, {len(errors)} error texts, {len(index)} distinct train-plan op records")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write_golden()
    else:
        print(__doc__)
