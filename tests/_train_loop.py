"""What the tests of smx_train_stage / smx_train_land share (trains of any size, one step at a
time: DeviceTrainLoop, compose_train(large=True)): the column-level train oracle of tests/_train.py
without its size limit, the golden trains with a filler log in front that pushes every step over
2048 ops, and the check of a DeviceTrainLoop run against the oracle, canaries included."""
import numpy as np

import _train
from _train import FILL, NONE, RES

BIG = 1 << 62
FILLER_OPS = 2100


def run_train(lsoa, train, **kw):
    """_train.run_train with no limit on a step's size: its only limit is the module's
    BATCH_MAX_OPS, lifted for the call."""
    old = _train.BATCH_MAX_OPS
    _train.BATCH_MAX_OPS = BIG
    try:
        return _train.run_train(lsoa, train, **kw)
    finally:
        _train.BATCH_MAX_OPS = old


_ref = {}


def ref(lsoa, train, **kw):
    """run_train(lsoa, train), computed once per (LogsSoA, train, arguments)."""
    key = (id(lsoa), tuple(train), tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else repr(v))
                                                  for k, v in kw.items())))
    got = _ref.get(key)
    if got is None:
        got = _ref[key] = ((lsoa, kw), run_train(lsoa, train, **kw))
    return got[1]


def fronted(case, c, n=FILLER_OPS):
    """A golden case (the dicts of _train.golden_case) with a filler log behind its logs and in
    front of its train: n editStmtBlock ops on fresh symbols, their provenance taken in turn from
    the case's own ops, so their timestamps spread over the case's range.  The filler holds no
    rename and no move: it lands first, every later step is over 2048 ops, and the golden
    conflicts and the golden ops (behind the filler's) stay as they are.  Returns (logs, train)."""
    own = [o for log in case["logs"] for o in log]
    prov = [dict(o["provenance"]) for o in own] or [{"rev": "base"}]
    filler = [{"id": f"{i:08x}-{c:04x}-4000-8000-00000000f111", "schemaVersion": 1, "type": "editStmtBlock",
               "target": {"symbolId": f"filler{c}_{i}", "addressId": None}, "params": {"file": "filler.ts"},
               "guards": {}, "effects": {}, "provenance": dict(prov[i % len(prov)])} for i in range(n)]
    return case["logs"] + [filler], [len(case["logs"])] + list(case["train"])


def staged_values(lsoa, tr, v1_alt=None, empty_str=NONE):
    """(v0, v1, fell) that smx_train_stage gives the step of trace entry `tr` (run_train's trace):
    a move's v0 / v1 from the addr / file it has gathered, v1_alt's entry where that file is the
    empty string; fell: the entries that took v1_alt."""
    idx, a, f = tr["idx"], tr["addr"], tr["file"]
    move = tr["kind"] == _train.KIND_MOVE
    v0 = np.where(move & (a != NONE), a, np.asarray(lsoa.v0)[idx]).astype(np.int32)
    v1 = np.where(move & (f != NONE), f, np.asarray(lsoa.v1)[idx]).astype(np.int32)
    fell = move & (f == empty_str) if empty_str != NONE else np.zeros(len(idx), bool)
    if fell.any():
        v1 = np.where(fell, np.asarray(v1_alt, np.int32)[idx], v1).astype(np.int32)
    return v0, v1, fell


def run(lsoa, train, hook=None, **kw):
    from semantic_merge_amd._rigs import DeviceTrainLoop
    db = DeviceTrainLoop(lsoa, train, fill=FILL, **kw)
    db.run(hook=hook)
    return db, db.raw()


def check(db, raw, label, want=None, truncated=(), **kw):
    """The run equals the oracle (`want`: the expected result instead) step by step -- the length
    after each step, its outcome and records (steps of `truncated`: the oracle's first records,
    the full count) --, in the final src / addr / file / ctx and in the steps that landed; and no
    word was written outside what the contract names: past the staged columns' capacity, past the
    longest accumulator a state buffer ever took, past a step's records, past status."""
    w = ref(db.lsoa, db.train, **kw) if want is None else want
    res = db.results(raw)
    for name, g, r in zip(RES, res[:4], w[:4]):
        assert np.array_equal(g, r), f"{label}: {name} differs: {g[:8]} vs {r[:8]} ({len(g)}, {len(r)})"
    assert res[4] == w[4], f"{label}: {res[4]} steps landed, not {w[4]}"
    assert len(res[5]) == len(w[5]), f"{label}: steps"
    wrote = np.zeros(len(raw["records"]), bool)
    top, cur = [0, 0], 0  # the longest accumulator each state buffer took
    if db._acc is not None:
        top[0] = len(db._acc[0])
    for g, (got, exp) in enumerate(zip(res[5], w[5])):
        c, cap = int(db.rec_off[g]), int(db.rec_off[g + 1] - db.rec_off[g])
        assert got[:2] == exp[:2], f"{label}: step {g}: (length, outcome) {got[:2]}, not {exp[:2]}"
        recs = exp[2]
        if g in truncated:
            assert exp[1] > cap, f"{label}: step {g} is not truncated"
            recs = recs[:cap]
        assert np.array_equal(got[2], recs), f"{label}: step {g}: conflict records differ"
        wrote[4 * c: 4 * (c + len(recs))] = True
        if got[1] == 0 and db.steps[g][2] is not None:
            cur ^= 1
            top[cur] = max(top[cur], got[0])
    assert cur == db.cur, f"{label}: the state buffers flipped {db.cur}, not {cur}"
    fill32 = np.int32(FILL)
    bad = np.flatnonzero(~wrote & (raw["records"] != fill32))
    assert not len(bad), f"{label}: records written outside the steps' records, at {bad[:5].tolist()}"
    q = db.cap + db.CONF_GUARD
    for b in (0, 1):
        st = raw["state%d" % b]
        for f in range(4):
            bad = np.flatnonzero(st[f * q + top[b]: (f + 1) * q] != fill32)
            assert not len(bad), f"{label}: state buffer {b}, {RES[f]}: written past {top[b]} entries, at {bad[:5].tolist()}"
        assert (st[4 * q:] == fill32).all(), f"{label}: state buffer {b} written past its end"
    for name in raw:
        if name.startswith("st_"):
            guard = raw[name][db.cap:]  # (a byte column holds the fill's low byte)
            assert (guard == (FILL & 0xFF if guard.dtype == np.uint8 else FILL)).all(), \
                f"{label}: {name} written past its capacity"
    assert (raw["status"][3:] == np.int64(FILL)).all(), f"{label}: status written past its three words"
    return res
