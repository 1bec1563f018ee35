"""csrc/op_extents.h on the CPU: what plan creation enforces about an op's operands, what ftc_op_extents exports, what the train-graph builder sizes
from it and what both plan builders check with it -- against tests/golden/op_extents.json.gz (tests/op_extents_sweep.py), recorded from the commit before
the header, when validate_op, the Python builder and TrainStep._grad_write_extents each stated the extents on their own."""
import os
import re
import subprocess

import pytest

import op_extents_sweep as S
from findtextcenternet_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# A not-given operand with base id 99 is GIVEN to the resolvers, so on these forms the mutant carries two faults at once -- the base id, and an out2 the
# op's form has no place for.  The form is reported first now, as the six backbone kinds and WGRAD always did; the recorded text was "out2: bad base id".
FORM_FIRST = ("conv: out2 (bf16 copy) needs an fp32 primary output and Cout % 4 == 0",
              "conv: an fp32 convolution writes out2 only as the pre-split copy of an fp16x3 plan (FTC_FLAG_SPLIT16; whole rows, one group)",
              "bnact: out2 (16-bit copy) needs an fp32 primary output")


@pytest.fixture(scope="module")
def gold():
    return S.load_golden()


@pytest.fixture(scope="module")
def plans():
    """{case: (TrainStep, plan)}: the six train plans, built once (Builder.resolve has run its fit check on each)."""
    return S.train_plans()


@pytest.fixture(scope="module")
def keys(plans):
    return {"inference": S.inference_keys(), "train": S.train_keys(plans), "cases": S.case_keys()}


@pytest.fixture(scope="module")
def verdicts(keys):
    return {s: S.replay_verdicts(keys[s]) for s in S.SETS}


@pytest.fixture(scope="module")
def mutant_ops(keys, verdicts):
    return S.mutant_keys(S.distinct([k for s in S.SETS for k, e in zip(keys[s], verdicts[s]) if e is None]))


@pytest.mark.parametrize("part", S.SETS)
def test_verdicts_equal_the_recorded_ones(gold, keys, verdicts, part):
    """(a) the same ops, each accepted or refused with the exact message recorded before the header."""
    want = gold["verdicts"][part]
    assert len(keys[part]) == want["n"] > 0 and S.digest(keys[part]) == want["sha256"]
    for k, got, ei in zip(keys[part], verdicts[part], want["err"]):
        assert got == (None if ei < 0 else gold["errors"][ei]), k


def test_single_fault_mutants_equal_the_recorded_ones(gold, mutant_ops):
    """(b) every operand of every accepted op: null, misaligned, one byte short of its end and exactly at it, and a bad base id on the operands that are
    not given -- byte for byte, but for the two-fault entries of FORM_FIRST."""
    want = gold["mutants"]
    assert len(mutant_ops) == want["n"] > 4000 and S.digest(mutant_ops) == want["sha256"]
    txt = lambda i: None if i < 0 else gold["errors"][i]      # noqa: E731
    form_first = {t: 0 for t in FORM_FIRST}
    for k, rows in zip(mutant_ops, want["rows"]):
        for name, got, rec in zip(S.REF_NAMES, S.mutants(k), rows):
            if len(rec) == 4:
                assert got == [txt(rec[0]), txt(rec[1]), rec[2], txt(rec[3])], (k, name)
            elif got != [txt(rec[0])]:
                reason = got[0].split("): ", 1)[1]
                assert name == "out2" and txt(rec[0]).endswith("): out2: bad base id") and reason in form_first, (k, name, got, txt(rec[0]))
                form_first[reason] += 1
    assert all(form_first.values()), form_first


def test_exported_extents_are_what_plan_creation_enforces(gold, mutant_ops):
    """ftc_op_extents of every accepted op: bytes = the recorded number at which the one-op plan flips from refused to accepted (0, unknown: the start
    alone, one byte), and a state that agrees with the recorded verdicts of the null and bad-base mutants."""
    seen = {L.OPERAND_UNUSED: 0, L.OPERAND_OPTIONAL: 0, L.OPERAND_REQUIRED: 0}
    for k, rows in zip(mutant_ops, gold["mutants"]["rows"]):
        nbytes, state = L.op_extents(S.make_op(k)[0])
        for name, b, st, rec in zip(S.REF_NAMES, nbytes, state, rows):
            seen[st] += 1
            if len(rec) == 4:                                # given
                null, flip = (None if rec[0] < 0 else gold["errors"][rec[0]]), rec[2]
                assert (flip == 0) == (st == L.OPERAND_UNUSED) and (flip == 0 or max(b, 1) == flip), (k, name, b, st, flip)
                if null is not None and null.endswith(f"): {name}: missing required operand"):
                    assert st == L.OPERAND_REQUIRED, (k, name)
                assert not (st == L.OPERAND_REQUIRED and null is None), (k, name)
            else:                                            # not given: base id 99 was accepted (unused), refused as a bad operand (optional), or GIVING
                bad_operand = rec[0] >= 0 and gold["errors"][rec[0]].endswith(f"): {name}: bad base id")      # the operand changed what the form asks
                assert st != L.OPERAND_REQUIRED and (rec[0] >= 0 or st == L.OPERAND_UNUSED) and (not bad_operand or st == L.OPERAND_OPTIONAL), (k, name, st)
    assert all(seen.values()), seen


def test_a_malformed_op_has_no_extents():
    op = S.make_op(S.inference_keys()[0])
    op[0].B = 0
    with pytest.raises(L.FtcError, match="ftc_op_extents: B/H/W must be positive"):
        L.op_extents(op[0])


def test_train_plans_and_bucket_segments_equal_the_recorded_ones(gold, plans):
    """(c) every field of every op of the six train plans, workspace_bytes and n_fwd; (d) the bucket segments of synthetic ranges."""
    for case, (ts, plan) in plans.items():
        want, got = gold["plans"][case], S.plan_record(plan)
        assert got["workspace_bytes"] == want["workspace_bytes"] and got["n_fwd"] == want["n_fwd"] and len(got["ops"]) == len(want["ops"]), case
        for i, (g, wi) in enumerate(zip(got["ops"], want["ops"])):
            assert g == gold["records"][wi], (case, i, plan["names"][i])
        assert S.segments(ts, plan) == gold["segments"][case], case
    assert len(gold["plans"]) == 6


def test_the_builders_size_no_scratch_of_their_own():
    """The chunk formulas live in csrc/op_extents.h alone: the only clamp left in the Python package is rows_p, a launch parameter."""
    pkg = os.path.join(ROOT, "findtextcenternet_amd")
    hits = [(f, line.strip()) for f in sorted(os.listdir(pkg)) if f.endswith(".py") for line in open(os.path.join(pkg, f)) if "min(512" in line or "min(2048" in line]
    assert len(hits) == 1 and hits[0][0] == "train_graph.py" and hits[0][1].startswith("rows_p ="), hits


def test_train_builder_names_an_operand_that_does_not_fit_its_buffer(monkeypatch):
    """A scratch buffer reserved 256 bytes short: Builder.resolve names the op index, the op and the operand."""
    from findtextcenternet_amd import TextDetectorModel, TrainStep
    from findtextcenternet_amd import train_graph as G
    resolve = G.Builder.resolve

    def short(self):
        i = next(i for i, f in enumerate(self.ops) if f["kind"] == L.OP_WGRAD)
        self.ops[i]["aux"][1].nbytes -= 256
        return resolve(self)
    monkeypatch.setattr(G.Builder, "resolve", short)
    model = TextDetectorModel(pre_weights=False, precision="fp32").train()
    with pytest.raises(RuntimeError, match=r"train plan: op \d+ \(wgrad:decoder\.blocks\.\d\.6\.weight\): operand aux spans \d+ bytes from offset 0 of a buffer of \d+"):
        TrainStep(model, "bf16").plan_for(2, 128, 128)


def test_inference_builder_names_an_operand_that_does_not_fit_its_buffer(monkeypatch):
    """FTC_PLAN_SHRINK_BUF reserves one buffer of csrc/plan.hip's builder 256 bytes short: Builder::finish names the op index, the op and the operand.
    (The fit check itself ran on every plan the recorded sweep of tests/plan_sweep.py builds: test_abi_and_plan.py replays them.)"""
    import plan_sweep as P
    model = P.Models().get("s", "bf16")
    model.plan(2, 128, 160)
    monkeypatch.setenv("FTC_PLAN_SHRINK_BUF", "0")
    with pytest.raises(L.FtcError, match=r"ftc model plan: op 0 \(backbone\.features\.0\): operand out spans \d+ bytes from offset 0 of a buffer of \d+"):
        model.plan(2, 128, 160)


@pytest.fixture(scope="module")
def op_extents_host(tmp_path_factory):
    """tests/c_abi/op_extents_host.cc (plain C++ over csrc/op_extents.h and the choice headers alone, its own main) built with AddressSanitizer + UBSan;
    returns a function that runs it on op keys and returns [(reason, [(state, bytes)] * 11)]."""
    exe = str(tmp_path_factory.mktemp("op_extents") / "op_extents_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "c_abi", "op_extents_host.cc"), "-o", exe], check=True)

    def run(ks):
        r = subprocess.run([exe], input="".join(" ".join(map(str, k)) + "\n" for k in ks), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [line.split("\t") for line in r.stdout.split("\n")[:-1]]
        assert len(lines) == len(ks) and all(len(line) == 2 for line in lines)
        return [(why, [tuple(int(v) for v in f.split(":")) for f in fields.split(" ")]) for why, fields in lines]
    return run


def test_op_extents_header_is_host_only_and_clean_under_sanitizers(gold, keys, verdicts, op_extents_host):
    """The stand-alone program over every recorded op: it refuses what the library refused for its form with the reason the library gave, and prints the
    table ftc_op_extents returns for the others (an op at offset 0 of a workspace of 2^44 bytes is refused for its form or not at all, but for a
    required operand it does not carry)."""
    for part in S.SETS:
        for k, err, (why, table) in zip(keys[part], verdicts[part], op_extents_host(keys[part])):
            if err is None:
                nbytes, state = L.op_extents(S.make_op(k)[0])
                assert why == "" and table == list(zip(state, nbytes)), (part, k)
            elif why:
                assert err.endswith("): " + why), (part, k, why)
            else:
                assert re.search(r"\): \w+: missing required operand$", err), (part, k, err)
