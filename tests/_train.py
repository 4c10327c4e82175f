"""What the smx_compose_train tests share: the column-level train oracle -- a Python loop over
oracle.compose with the re-log rule of include/smx.h (the accumulator's columns are its source
ops' own, a move's v0 / v1 replaced by the addr / file it has gathered; a step lands on zero
conflicts and folds its addr / file / ctx in, per field the last value that is not -1) --, the
materialiser of its results into Op and Conflict objects, and the check of a DeviceTrains run
against it, canaries included."""
import numpy as np

from oracle import oracle
from semantic_merge_amd._abi import BATCH_MAX_OPS
from semantic_merge_amd.marshal import SoA
from semantic_merge_amd.materialize import conflict_factory, materialize_ops
from semantic_merge_amd.ops import KIND_MOVE

FILL = 0x5A5A5A5A  # what every output word holds before a run
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")
RES = ("src", "addr", "file", "ctx")
N_KINDS = 18
NONE = -1


def golden_case(case):
    """A case of tests/golden/train_cases.json as plain dicts: {"logs": op dicts per log, "train",
    "out": the op dicts the train leaves, "steps": per step its conflict dicts}.  The file holds
    an input op as [id, type, symbolId, addressId, params, [timestamp]] (then guards and effects,
    where it has any), an output op as [log, index] of the input op it is a clone of (then params
    and addressId where the reference changed them), and a conflict as its A and B ops in that
    form; tools/make_train_golden.py checks that every case reads back to the reference's dicts."""
    from semantic_merge_amd.conflict import divergent_rename
    from semantic_merge_amd.ops import Op

    def op(s):
        prov = {"rev": "base", **({"timestamp": s[5][0]} if s[5] else {})}
        return {"id": s[0], "schemaVersion": 1, "type": s[1], "target": {"symbolId": s[2], "addressId": s[3]},
                "params": s[4], "guards": s[6] if len(s) > 6 else {}, "effects": s[7] if len(s) > 6 else {},
                "provenance": prov}

    logs = [[op(s) for s in log] for log in case["logs"]]

    def clone(c):
        d = logs[c[0]][c[1]]
        return d if len(c) == 2 else {**d, "target": {"symbolId": d["target"]["symbolId"], "addressId": c[3]},
                                      "params": c[2]}

    steps = [[divergent_rename(Op.from_dict(clone(a)), Op.from_dict(clone(b))).to_dict() for a, b in step]
             for step in case["steps"]]
    return {"logs": logs, "train": case["train"], "out": [clone(c) for c in case["out"]], "steps": steps}


def logs_ok(log_off, n_total):
    """smx_screen's log_off rules: log l is invalid when its offset is negative or below an
    earlier offset, or its end before its start or past n_total."""
    off = np.asarray(log_off, np.int64)
    before = np.maximum.accumulate(np.concatenate([[0], off[:-1]]))[:-1] if len(off) > 1 else np.zeros(0, np.int64)
    return (off[:-1] >= before) & (off[1:] >= off[:-1]) & (off[1:] <= n_total)


def run_train(lsoa, train, log_off=None, n_sym=None, n_total=None, trace=None, v1_alt=None, empty_str=NONE):
    """(src, addr, file, ctx, landed, steps) of one train over a LogsSoA; steps: per step
    (accumulator length after it, outcome, conflict records (n, 4)).  trace: a list that gets,
    per step that composed, what went in and came out (for tests that look inside a step)."""
    cols = {c: np.asarray(getattr(lsoa, c)) for c in COLS}
    off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64)
    n_sym = int(lsoa.n_sym) if n_sym is None else n_sym
    ok = logs_ok(off, int(lsoa.n_total) if n_total is None else n_total)
    src = np.zeros(0, np.int32)
    addr, file, ctx = src.copy(), src.copy(), src.copy()
    none = np.zeros((0, 4), np.int32)
    landed, steps = 0, []
    for l in train:
        if not (0 <= l < len(ok)) or not ok[l]:
            steps.append((len(src), -1, none))
            continue
        lo, nb = int(off[l]), int(off[l + 1] - off[l])
        if len(src) + nb > BATCH_MAX_OPS:
            steps.append((len(src), -2, none))
            continue
        idx = np.concatenate([src, np.arange(lo, lo + nb, dtype=np.int32)]).astype(np.int32)
        fresh = np.full(nb, NONE, np.int32)
        a, f, x = np.concatenate([addr, fresh]), np.concatenate([file, fresh]), np.concatenate([ctx, fresh])
        kind, sym = cols["kind"][idx], cols["sym"][idx]
        if (kind >= N_KINDS).any() or (sym.astype(np.int64) >= n_sym).any():
            steps.append((len(src), -1, none))
            continue
        move = kind == KIND_MOVE
        v0 = np.where(move & (a != NONE), a, cols["v0"][idx]).astype(np.int32)
        v1 = np.where(move & (f != NONE), f, cols["v1"][idx]).astype(np.int32)
        if empty_str != NONE:  # an empty newFile: marshalling falls through to the op's own `file`
            v1 = np.where(move & (f == empty_str), np.asarray(v1_alt, np.int32)[idx], v1).astype(np.int32)
        soa = SoA(len(src), nb, kind, cols["ts"][idx], cols["oid_hi"][idx], cols["oid_lo"][idx], sym, v0, v1, n_sym)
        order, ra, rf, rx, pairs = oracle.compose(soa)
        if trace is not None:
            trace.append({"step": len(steps), "n_acc": len(src), "idx": idx, "kind": kind, "addr": a, "file": f,
                          "order": order, "r_addr": ra, "r_file": rf, "pairs": pairs})
        if len(pairs):
            ea, eb = pairs[:, 0], pairs[:, 1]
            steps.append((len(src), len(pairs), np.stack([idx[ea], idx[eb], a[ea], f[ea]], axis=1).astype(np.int32)))
            continue
        src = idx[order]
        addr = np.where(ra != NONE, ra, a[order]).astype(np.int32)
        file = np.where(rf != NONE, rf, f[order]).astype(np.int32)
        ctx = np.where(rx != NONE, rx, x[order]).astype(np.int32)
        landed += 1
        steps.append((len(src), 0, none))
    return src, addr, file, ctx, landed, steps


_ref = {}


def ref(lsoa, train, **kw):
    """run_train(lsoa, train), computed once per (LogsSoA, train)."""
    key = (id(lsoa), tuple(train), tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else repr(v))
                                                  for k, v in kw.items())))
    got = _ref.get(key)
    if got is None:
        got = _ref[key] = ((lsoa, kw), run_train(lsoa, train, **kw))
    return got[1]


def materialize(lsoa, ops, result):
    """(ops the train leaves, per step its Conflict objects) of a train's result, in the oracle's
    or the device's form, over `ops`, all the logs' ops in column order: one materialise with
    order = src, and per conflict A built from the source op with the record's addr / file."""
    src, addr, file, ctx, _, steps = result
    kind = np.asarray(lsoa.kind)
    out = materialize_ops(ops, kind, lsoa.strings, np.asarray(src), np.asarray(addr), np.asarray(file), np.asarray(ctx))
    make = conflict_factory()
    conf = []
    for _, _, recs in steps:
        recs = np.asarray(recs).reshape(-1, 4)
        a = materialize_ops(ops, kind, lsoa.strings, recs[:, 0], recs[:, 2], recs[:, 3], np.full(len(recs), NONE))
        conf.append([make(x, ops[b]) for x, b in zip(a, recs[:, 1].tolist())])
    return out, conf


def run(lsoa, trains, **kw):
    from semantic_merge_amd._lib import DeviceTrains
    db = DeviceTrains(lsoa, trains, fill=FILL, **kw)
    db.run()
    raw = db.raw()
    return db, raw


def check(db, raw, label, failed=(), truncated=(), want=None, **kw):
    """Trains of `failed` report -1, -1 and wrote nothing; every other train equals the oracle
    (`want`: per train its expected result instead), step by step (steps of `truncated`, by
    global step index: the oracle's first records, the full count); no word outside the valid
    trains' counts-long regions, the steps' records and counts was written."""
    res = db.results(raw)
    fill32, fill64 = np.int32(FILL), np.int64(FILL)
    wrote = {name: np.zeros(len(raw[name]), bool) for name in RES + ("conf", "counts", "step_counts")}
    for t, train in enumerate(db.trains):
        k, landed = (int(x) for x in raw["counts"][2 * t: 2 * t + 2])
        wrote["counts"][2 * t: 2 * t + 2] = True
        if t in failed:
            assert (k, landed) == (-1, -1), f"{label}: train {t} reports {(k, landed)}, not -1"
            continue
        assert not isinstance(res[t], int), f"{label}: train {t} failed with counts {res[t]}"
        w = want[t] if want is not None else ref(db.lsoa, train, **kw)
        for name, g, r in zip(RES, res[t][:4], w[:4]):
            assert np.array_equal(g, r), f"{label}: train {t}: {name} differs: {g[:8]} vs {r[:8]} ({len(g)}, {len(r)})"
        assert landed == w[4], f"{label}: train {t}: {landed} steps landed, not {w[4]}"
        g0 = int(db.train_off[t])
        assert len(res[t][5]) == len(w[5]), f"{label}: train {t}: steps"
        for s, (got, exp) in enumerate(zip(res[t][5], w[5])):
            g = g0 + s
            c, cap = int(db.conf_off[g]), int(db.conf_off[g + 1] - db.conf_off[g])
            assert got[:2] == exp[:2], f"{label}: train {t} step {s}: (length, outcome) {got[:2]}, not {exp[:2]}"
            recs = exp[2]
            if g in truncated:
                assert exp[1] > cap, f"{label}: train {t} step {s} is not truncated"
                recs = recs[:cap]
            assert np.array_equal(got[2], recs), f"{label}: train {t} step {s}: conflict records differ"
            wrote["conf"][4 * c: 4 * (c + len(recs))] = True
            wrote["step_counts"][2 * g: 2 * g + 2] = True
        o = int(db.res_off[t])
        for name in RES:
            wrote[name][o: o + k] = True
    for name in wrote:
        fill = fill64 if raw[name].dtype == np.int64 else fill32
        bad = np.flatnonzero(~wrote[name] & (raw[name] != fill))
        assert not len(bad), f"{label}: {name} written outside the valid regions, at {bad[:5].tolist()}"
    return res
