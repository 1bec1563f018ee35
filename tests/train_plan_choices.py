"""The recorded kernel choices of the train step's plans: [signature, aux0] of every FTC_OP_CONV, in plan order, of
TrainStep(model, precision).plan_for(B, H, W) for the cases below -- host-side, no GPU needed.  If these are equal, the train step launches
the same convolution kernels.

    python tests/train_plan_choices.py --write        # rewrites tests/golden/train_plan_choices.json.gz from the library in the tree

The file is a gzip of JSON: {case: [[signature, aux0], ...]}.  tests/test_tuning_host.py replays every case.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from findtextcenternet_amd import _lib as L            # noqa: E402
from findtextcenternet_amd import tuning               # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "train_plan_choices.json.gz")
CASES = [(p, B, H, W) for B, H, W in ((8, 768, 768), (2, 128, 128)) for p in ("bf16", "fp16", "fp32")]
TUNED = {(8, 768, 768): {"bf16": 480, "fp16": 480, "fp32": 7}, (2, 128, 128): {"bf16": 0, "fp16": 0, "fp32": 0}}     # convolutions with aux0 != 0


def case_name(p, B, H, W):
    return f"{p}_b{B}_{H}x{W}"


def conv_ops(plan):
    return [plan["ops"][i] for i in range(plan["n_ops"]) if plan["ops"][i].kind == L.OP_CONV]


def choices(model, p, B, H, W):
    from findtextcenternet_amd import TrainStep
    return [[tuning.signature(o), int(o.aux0)] for o in conv_ops(TrainStep(model, p).plan_for(B, H, W))]       # (plan_for raises unless ftc_plan_create accepts)


def replay(cases=CASES):
    from findtextcenternet_amd import TextDetectorModel
    model = TextDetectorModel(pre_weights=False, precision="fp32").train()
    return {case_name(*c): choices(model, *c) for c in cases}


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


if __name__ == "__main__":
    if "--print" in sys.argv:                 # --print precision B H W: one case as JSON, for a test that needs it from a process of its own
        p, B, H, W = sys.argv[sys.argv.index("--print") + 1:][:4]
        print(json.dumps(replay([(p, int(B), int(H), int(W))])))
    elif "--write" in sys.argv:
        doc = replay()
        with gzip.GzipFile(GOLDEN, "wb", mtime=0) as f:
            f.write(json.dumps(doc, separators=(",", ":")).encode())
        print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes; " + ", ".join(f"{k}: {sum(1 for _, a in v if a)} of {len(v)} tuned" for k, v in doc.items()))
    else:
        print(__doc__)
