"""GPU parity of smx_train_stage and smx_train_land (csrc/smx_train_step.h), through
DeviceTrainLoop: a train of any size as a host loop of stage, smx_compose and land, against the
column-level train oracle without its size limit (tests/_train_loop.py), step by step -- the
length after each step, its outcome and records, the final accumulator, the steps that landed.
Every output word starts as a canary, so the words a call must not write are checked.  Shapes: the
first step over 2048 ops (2200, then 3300) and the smallest one (2048, then 2049); golden trains
behind a filler log that puts every step over the limit; a conflict, then a landing; truncated
records; empty logs; a log twice; invalid logs; a bad src in a hand-made accumulator; two trains
one after another on one set of buffers."""
import numpy as np
import pytest

from semantic_merge_amd import marshal as M
from semantic_merge_amd.ops import KIND_MOVE

import _train
import _train_loop as TL
from _batch import ADV, branch, none_moves
from _pairs import logs_soa
from _util import load, to_ops

pytestmark = pytest.mark.gpu

N_SYM = 64
RENAME = 1
GOLDEN_EVERY = 3  # every third golden train: the file runs in a few seconds


def clean(n, seed, **kw):
    """A log of n ops without renames: it conflicts with nothing, so every step with it lands."""
    soa = branch(n, N_SYM, seed, seed & 1, **kw)
    soa.kind[soa.kind == RENAME] = 2
    return soa


def spoiled(soa, **cols):
    """A copy of a log with its middle op's columns set (an invalid kind or symbol)."""
    out = M.SoA(soa.n_a, soa.n_b, *[np.array(getattr(soa, c)) for c in _train.COLS], soa.n_sym)
    for c, v in cols.items():
        getattr(out, c)[out.n // 2] = v
    return out


NAMES = ("empty", "c1100a", "c1100b", "c1100c", "c1024a", "c1024b", "one", "m1100", "advA", "advB", "c9", "badkind",
         "badsym")
IX = {name: i for i, name in enumerate(NAMES)}


def T(*names):
    return [IX[n] for n in names]


def make_pool():
    c = [clean(1100, 21), none_moves(clean(1100, 22), 5), clean(1100, 23), clean(1024, 24), clean(1024, 25)]
    empty = M.SoA(0, 0, *[np.asarray(getattr(c[0], col))[:0] for col in _train.COLS], N_SYM)
    # moves first, then two logs whose renames diverge: the second conflicts with what the first left
    logs = [empty] + c + [branch(1, N_SYM, 3, 1), none_moves(clean(1100, 31, **ADV), 7),
                          branch(1100, N_SYM, 32, 0, **ADV), branch(1100, N_SYM, 32, 1, **ADV), clean(9, 26),
                          spoiled(clean(40, 27), kind=18), spoiled(clean(40, 28), sym=N_SYM)]
    assert len(logs) == len(NAMES)
    return logs_soa(logs, N_SYM)


@pytest.fixture(scope="module")
def pool():
    return make_pool()


def test_just_past_2048_ops(pool):
    """Three logs of 1100 ops: step 0 has an empty accumulator, step 1 is the first over 2048 ops
    (2200), step 2 is 3300; and the smallest large step: 1024 + 1024 = 2048, then one op more."""
    for label, train, lens in (("3 x 1100", T("c1100a", "c1100b", "c1100c"), [1100, 2200, 3300]),
                               ("1024, 1024, 1", T("c1024a", "c1024b", "one"), [1024, 2048, 2049]),
                               ("moves, then renames", T("m1100", "advA", "c1100b"), [1100, 2200, 3300])):
        db, raw = TL.run(pool, train)
        res = TL.check(db, raw, label)
        assert [s[0] for s in res[5]] == lens and res[4] == 3, label
        assert [s[2][0] for s in db.steps] == [0, 0, 0], label


def golden_runs():
    """Every GOLDEN_EVERY-th golden train behind a filler log: (logs as ops, LogsSoA, train, v1_alt,
    empty_str, the oracle's result and its trace)."""
    out = []
    for c, case in enumerate(load("train_cases.json")):
        if c % GOLDEN_EVERY:
            continue
        dicts, train = TL.fronted(_train.golden_case(case), c)
        logs = [to_ops(x) for x in dicts]
        lsoa = M.marshal_logs(logs)
        alt, empty = M.move_file_alt([o for log in logs for o in log], lsoa.kind, lsoa.strings)
        trace = []
        want = TL.run_train(lsoa, train, trace=trace, v1_alt=alt, empty_str=empty)
        out.append((logs, lsoa, train, alt, empty, want, trace))
    return out


def golden_situations(runs):
    """What the chosen trains hold: evicted steps; a None-valued move that inherited a value a
    step earlier, behind the filler, with an op of the next log's landing between the two (the
    staged rewrite of v0 / v1); steps that stage a move whose gathered file is the empty string,
    so that its v1 falls through to v1_alt, and trains whose last step does."""
    seen = {"evicted": 0, "inherited": 0, "empty file": 0, "empty file, last step": 0}
    for _, lsoa, _, alt, empty, want, trace in runs:
        seen["evicted"] += sum(1 for _, oc, _ in want[5] if oc > 0)
        fell = [bool(TL.staged_values(lsoa, tr, alt, empty)[2].any()) for tr in trace]
        seen["empty file"] += sum(fell)
        seen["empty file, last step"] += fell[-1]
        for tr in trace:
            if len(tr["pairs"]) or tr["n_acc"] < TL.FILLER_OPS:
                continue
            o = tr["order"]
            old, mv = o < tr["n_acc"], tr["kind"][o] == KIND_MOVE
            v0, v1 = np.asarray(lsoa.v0)[tr["idx"][o]], np.asarray(lsoa.v1)[tr["idx"][o]]
            seen["inherited"] += bool((old & mv & (v0 == -1) & (tr["addr"][o] == -1) & (tr["r_addr"] != -1)).any() or
                                      (old & mv & (v1 == -1) & (tr["file"][o] == -1) & (tr["r_file"] != -1)).any())
    return seen


def test_golden_trains_pushed_over_the_limit():
    runs = golden_runs()
    seen = golden_situations(runs)
    assert seen["evicted"] >= 10 and seen["inherited"] >= 1 and seen["empty file"] >= 1 and \
        seen["empty file, last step"] >= 1, seen
    for c, (_, lsoa, train, alt, empty, want, trace) in enumerate(runs):
        label = f"golden train {c * GOLDEN_EVERY}"
        assert all(n >= TL.FILLER_OPS for n, _, _ in want[5]), "every step is over the limit"
        db, raw = TL.run(lsoa, train, v1_alt=alt, empty_str=empty)
        TL.check(db, raw, label, want=want)
        # the last step's staged columns are still there: the moves' rewritten v0 / v1, the fall-through included
        v0, v1, _ = TL.staged_values(lsoa, trace[-1], alt, empty)
        assert np.array_equal(raw["st_v0"][: len(v0)], v0), f"{label}: the last step's staged v0"
        assert np.array_equal(raw["st_v1"][: len(v1)], v1), f"{label}: the last step's staged v1"


def test_a_conflict_then_a_landing(pool):
    """advB conflicts with what advA left, then c1100b lands: the state buffers did not flip at the
    conflict, the accumulator out was not written, and the records carry the A ops' accumulated
    addr and file."""
    snaps = []
    train = T("m1100", "advA", "advB", "c1100b")

    def hook(g, s):
        snaps.append((s, db_box[0].state0.cpu().numpy().copy(), db_box[0].state1.cpu().numpy().copy()))

    from semantic_merge_amd._rigs import DeviceTrainLoop
    db = DeviceTrainLoop(pool, train, fill=TL.FILL)
    db_box = [db]
    db.run(hook=hook)
    res = TL.check(db, db.raw(), "conflict, then landing")
    assert [oc for _, oc, _ in res[5]] == [0, 0, res[5][2][1], 0] and res[5][2][1] > 0
    assert snaps[2][0] == (0, res[5][2][1], 2200)
    assert snaps[1][1].tobytes() == snaps[2][1].tobytes() and snaps[1][2].tobytes() == snaps[2][2].tobytes()
    recs = res[5][2][2]
    assert (recs[:, 2] != -1).any() or (recs[:, 3] != -1).any(), "no record carries an accumulated value"
    assert [n for n, _, _ in res[5]] == [1100, 2200, 2200, 3300] and res[4] == 3


@pytest.mark.parametrize("cap", [0, 1])
def test_truncated_records(pool, cap):
    train = T("m1100", "advA", "advB", "c9")
    want = TL.ref(pool, train)
    assert want[5][2][1] > 1
    db, raw = TL.run(pool, train, record_caps=[1100, 1100, cap, 9])
    res = TL.check(db, raw, f"record_cap {cap}", truncated=[2])
    assert res[5][2][1] == want[5][2][1] and len(res[5][2][2]) == cap


def test_empty_logs_and_a_log_twice(pool):
    for label, train in (("an empty log in the middle", T("c1100a", "empty", "c1100b", "empty", "c9")),
                         ("an empty log first", T("empty", "c1100a", "c1100b")),
                         ("a log twice", T("m1100", "m1100", "c9", "c9")),
                         ("a log twice, with renames", T("c1100a", "advA", "advA"))):
        db, raw = TL.run(pool, train)
        res = TL.check(db, raw, label)
        assert res[4] >= 2, label


def test_invalid_logs(pool):
    """A log with an op of kind 18 and one with sym = n_sym: stage reports -1, the step's outcome is
    -1, nothing else is written, and the train goes on.  Log indices outside the logs give -1 on
    the host."""
    train = T("c1100a", "badkind", "c1100b", "badsym", "c9") + [-1, len(NAMES)] + T("one")
    db, raw = TL.run(pool, train)
    res = TL.check(db, raw, "invalid logs")
    assert [oc for _, oc, _ in res[5]] == [0, -1, 0, -1, 0, -1, -1, 0]
    assert db.steps[1][2][:2] == (-1, -1) and db.steps[3][2][:2] == (-1, -1)
    assert db.steps[5][2] is None and db.steps[6][2] is None
    # a log whose offsets decrease: invalid on the host, as smx_compose_train has it on the device
    off = np.array(pool.log_off)
    off[IX["c1100b"]] = off[IX["c1100a"]] - 1
    db, raw = TL.run(pool, T("c1100a", "c1100b", "c9"), log_off=off)
    res = TL.check(db, raw, "a log with a decreasing offset", log_off=off)
    assert res[5][1][1] == -1


@pytest.mark.parametrize("bad", ["n_total", "-1"])
def test_a_bad_src_is_not_read_through(pool, bad):
    """A hand-made accumulator with a src entry outside the columns: the device's own check gives
    -1, the entry is not dereferenced, and the accumulator stays."""
    src = np.arange(2100, dtype=np.int32) + int(pool.log_off[IX["c1100a"]])
    src[1234] = pool.n_total if bad == "n_total" else -1
    none = np.full(len(src), -1, np.int32)
    acc = (src, none, none, none)
    steps = [(len(src), -1, np.zeros((0, 4), np.int32))]
    db, raw = TL.run(pool, T("c9"), acc=acc)
    TL.check(db, raw, "a bad src", want=acc + (0, steps))
    assert db.steps[0][2] == (-1, -1, TL.FILL)
    assert raw["st_kind"][1234] == 0xFF and raw["st_sym"][1234] == -1
    # the same accumulator without the bad entry lands
    src[1234] = src[1233]
    db, raw = TL.run(pool, T("c9"), acc=(src, none, none, none))
    assert db.steps[0][2][:2] == (0, 0) and db.n_acc == len(src) + 9


def test_two_trains_on_one_set_of_buffers(pool):
    from semantic_merge_amd._rigs import DeviceTrainLoop
    t1, t2 = T("m1100", "advA", "advB", "c1100b"), T("c1024a", "c1024b", "one", "badkind", "advB")
    alone = []
    for tr in (t1, t2):
        db, raw = TL.run(pool, tr)
        alone.append(TL.check(db, raw, "own buffers"))
    a = DeviceTrainLoop(pool, t1, fill=TL.FILL)
    b = DeviceTrainLoop(pool, t2, share=a)
    for _ in range(2):
        for db, want in ((a, alone[0]), (b, alone[1])):
            db.run()
            got = db.results()
            for g, w in zip(got[:4], want[:4]):
                assert np.array_equal(g, w)
            assert got[4] == want[4] and len(got[5]) == len(want[5])
            for gs, ws in zip(got[5], want[5]):
                assert gs[:2] == ws[:2] and np.array_equal(gs[2], ws[2])
