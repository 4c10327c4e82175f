"""The premise of smx_compose_train on the CPU: a merge train is a loop over one compose with a
re-log rule between two steps, and that rule is include/smx.h's -- the accumulator's columns are
its source ops' own, a move's v0 / v1 replaced by the addr / file it has gathered, and addr /
file / ctx accumulate per field as the last value that is not -1.  The golden trains
(tests/golden/train_cases.json: the reference's compose_oplogs in the host loop with eviction,
tools/make_train_golden.py) are marshalled once per case, run through the column-level oracle
(tests/_train.py) and materialised once per train; final ops, per-step conflicts and which steps
landed equal the reference's.  Ops and conflicts are compared as dicts: materialising once sets
a move's newAddress before its newFile, step after step may add them in the other order.

The golden set holds every situation the rule is there for, asserted below."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import marshal as M
from semantic_merge_amd.ops import KIND_MOVE

import _train
from _util import load, to_ops


@pytest.fixture(scope="module")
def cases():
    return [_train.golden_case(c) for c in load("train_cases.json")]


@pytest.fixture(scope="module")
def runs(cases):
    """Per case (logs as ops, LogsSoA, all ops in column order, the oracle's result, its trace)."""
    out = []
    for case in cases:
        logs = [to_ops(x) for x in case["logs"]]
        lsoa = M.marshal_logs(logs)
        trace = []
        ops = [o for log in logs for o in log]
        alt, empty = M.move_file_alt(ops, lsoa.kind, lsoa.strings)
        out.append((logs, lsoa, ops, _train.run_train(lsoa, case["train"], trace=trace, v1_alt=alt, empty_str=empty),
                    trace))
    return out


def test_golden_trains_through_the_column_oracle(cases, runs):
    assert len(cases) >= 100
    for c, (case, (logs, lsoa, ops, res, _)) in enumerate(zip(cases, runs)):
        before = [o.to_dict() for o in ops]
        out, conf = _train.materialize(lsoa, ops, res)
        assert [o.to_dict() for o in ops] == before, f"case {c}: inputs mutated"
        assert [bool(s) for s in case["steps"]] == [oc != 0 for _, oc, _ in res[5]], f"case {c}: which steps landed"
        assert res[4] == sum(1 for s in case["steps"] if not s)
        assert [o.to_dict() for o in out] == case["out"], f"case {c}: the train's ops differ from the reference's"
        assert [[x.to_dict() for x in s] for s in conf] == case["steps"], f"case {c}: conflicts differ"
        assert len(res[0]) == len(case["out"]) and all(n <= len(case["out"]) for n, _, _ in res[5])


def test_golden_set_holds_every_situation(cases, runs):
    seen = dict.fromkeys(("evicted then lands", "conflicts with an earlier landed log only",
                          "lands though it conflicts with an evicted log", "a None-valued move inherits across a step",
                          "opA differs from the original op"), 0)
    for case, (logs, lsoa, ops, res, trace) in zip(cases, runs):
        train, steps = case["train"], res[5]
        off = np.asarray(lsoa.log_off)
        log_of = lambda col: int(np.searchsorted(off, col, "right")) - 1  # noqa: E731
        outcome = [oc for _, oc, _ in steps]
        landed_logs = []
        for s, oc in enumerate(outcome):
            if oc > 0 and any(o == 0 for o in outcome[s + 1:]):
                seen["evicted then lands"] += 1
            if oc > 0 and len(landed_logs) >= 2:
                a_steps = set()
                for col in steps[s][2][:, 0].tolist():   # the landed steps the conflicting A ops came in with
                    a_steps |= {q for q in landed_logs if train[q] == log_of(col)}
                if landed_logs[0] not in a_steps:
                    seen["conflicts with an earlier landed log only"] += 1
            if oc == 0:
                for e in range(s):
                    if outcome[e] > 0 and len(oracle.compose(lsoa.pair(train[e], train[s]))[4]):
                        seen["lands though it conflicts with an evicted log"] += 1
                        break
                landed_logs.append(s)
        for tr in trace:
            if len(tr["pairs"]):
                continue
            o = tr["order"]
            old = o < tr["n_acc"]
            mv = tr["kind"][o] == KIND_MOVE
            v0 = np.asarray(lsoa.v0)[tr["idx"][o]]
            v1 = np.asarray(lsoa.v1)[tr["idx"][o]]
            if (old & mv & (v0 == -1) & (tr["addr"][o] == -1) & (tr["r_addr"] != -1)).any() or \
                    (old & mv & (v1 == -1) & (tr["file"][o] == -1) & (tr["r_file"] != -1)).any():
                seen["a None-valued move inherits across a step"] += 1
        _, conf = _train.materialize(lsoa, ops, res)
        for (_, _, recs), cs in zip(steps, conf):
            for rec, cf in zip(recs.tolist(), cs):
                if cf.opA != ops[rec[0]].to_dict():
                    assert rec[2] != -1 or rec[3] != -1
                    seen["opA differs from the original op"] += 1
    assert all(seen.values()), seen
