"""What the smx_screen_train tests share: the two oracles of a train's conflicts and the check of a
DeviceScreenTrains run against them, canaries included.

full_train    the loop over oracle.compose with the re-log rule of include/smx.h (tests/_train.py's
              run_train) without the limit of 2048 ops: per step (the renames in the accumulator
              after it, outcome, the conflicts as (A column index, B column index))
rename_train  the premise of smx_screen_train in numpy: the accumulator is a list of renames
              sorted by (ts, oid_hi, oid_lo), a step is the reference's two-head walk of it
              against the log's renames, stably sorted, and a step that lands is a stable merge
              of the two, A first on equal keys
Both return (n_renames, landed, steps)."""
import numpy as np

from oracle import oracle
from semantic_merge_amd.marshal import SoA
from semantic_merge_amd.ops import KIND_MOVE, KIND_RENAME

from _train import COLS, N_KINDS, NONE, logs_ok

FILL = 0x5A5A5A5A  # what every output word holds before a run
NO_PAIRS = np.zeros((0, 2), np.int32)


def full_train(lsoa, train, log_off=None, n_total=None):
    cols = {c: np.asarray(getattr(lsoa, c)) for c in COLS}
    off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64)
    n_sym = int(lsoa.n_sym)
    ok = logs_ok(off, int(lsoa.n_total) if n_total is None else n_total)
    src = np.zeros(0, np.int32)
    addr, file, ctx = src.copy(), src.copy(), src.copy()
    landed, steps = 0, []

    def n_ren():
        return int((cols["kind"][src] == KIND_RENAME).sum())

    for l in train:
        if not (0 <= l < len(ok)) or not ok[l]:
            steps.append((n_ren(), -1, NO_PAIRS))
            continue
        lo, nb = int(off[l]), int(off[l + 1] - off[l])
        idx = np.concatenate([src, np.arange(lo, lo + nb, dtype=np.int32)]).astype(np.int32)
        fresh = np.full(nb, NONE, np.int32)
        a, f, x = np.concatenate([addr, fresh]), np.concatenate([file, fresh]), np.concatenate([ctx, fresh])
        kind, sym = cols["kind"][idx], cols["sym"][idx]
        if (kind >= N_KINDS).any():
            steps.append((n_ren(), -1, NO_PAIRS))
            continue
        move = kind == KIND_MOVE
        v0 = np.where(move & (a != NONE), a, cols["v0"][idx]).astype(np.int32)
        v1 = np.where(move & (f != NONE), f, cols["v1"][idx]).astype(np.int32)
        soa = SoA(len(src), nb, kind, cols["ts"][idx], cols["oid_hi"][idx], cols["oid_lo"][idx], sym, v0, v1, n_sym)
        order, ra, rf, rx, pairs = oracle.compose(soa)
        if len(pairs):
            steps.append((n_ren(), len(pairs), idx[np.asarray(pairs)].astype(np.int32).reshape(-1, 2)))
            continue
        src = idx[order]
        addr = np.where(ra != NONE, ra, a[order]).astype(np.int32)
        file = np.where(rf != NONE, rf, f[order]).astype(np.int32)
        ctx = np.where(rx != NONE, rx, x[order]).astype(np.int32)
        landed += 1
        steps.append((n_ren(), 0, NO_PAIRS))
    return n_ren(), landed, steps


def sorted_renames(lsoa, lo, hi):
    """The column indices of the renames of ops [lo, hi), stably sorted by (ts, oid_hi, oid_lo)."""
    j = lo + np.flatnonzero(np.asarray(lsoa.kind[lo:hi]) == KIND_RENAME)
    order = np.lexsort((np.asarray(lsoa.oid_lo)[j], np.asarray(lsoa.oid_hi)[j], np.asarray(lsoa.ts)[j]))  # (stable)
    return j[order].astype(np.int64)


def rename_train(lsoa, train, log_off=None, n_total=None):
    off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64)
    ok = logs_ok(off, int(lsoa.n_total) if n_total is None else n_total)
    kind = np.asarray(lsoa.kind)
    ts, hi, lo = (np.asarray(getattr(lsoa, c)).tolist() for c in ("ts", "oid_hi", "oid_lo"))
    sym, v0 = np.asarray(lsoa.sym).tolist(), np.asarray(lsoa.v0).astype(np.int32).tolist()
    acc, landed, steps = [], 0, []
    for l in train:
        if not (0 <= l < len(ok)) or not ok[l] or (kind[int(off[l]): int(off[l + 1])] >= N_KINDS).any():
            steps.append((len(acc), -1, NO_PAIRS))
            continue
        b = sorted_renames(lsoa, int(off[l]), int(off[l + 1])).tolist()
        i = j = 0
        merged, conf = [], []
        while i < len(acc) and j < len(b):
            x, y = acc[i], b[j]
            if sym[x] == sym[y] and v0[x] != v0[y]:
                conf.append((x, y))
                i += 1
                j += 1
            elif (ts[x], hi[x], lo[x]) <= (ts[y], hi[y], lo[y]):   # A first on equal keys
                merged.append(x)
                i += 1
            else:
                merged.append(y)
                j += 1
        if conf:
            steps.append((len(acc), len(conf), np.asarray(conf, np.int32).reshape(-1, 2)))
            continue
        acc = merged + acc[i:] + b[j:]
        landed += 1
        steps.append((len(acc), 0, NO_PAIRS))
    return len(acc), landed, steps


def same(got, want, label):
    """Two oracles' (or an oracle's and the device's) results of one train are equal."""
    assert got[:2] == want[:2], f"{label}: (renames, landed) {got[:2]}, not {want[:2]}"
    assert len(got[2]) == len(want[2]), f"{label}: steps"
    for s, (g, w) in enumerate(zip(got[2], want[2])):
        assert g[:2] == w[:2], f"{label}: step {s}: (renames, outcome) {g[:2]}, not {w[:2]}"
        assert np.array_equal(g[2], w[2]), f"{label}: step {s}: conflicts differ: {g[2][:4].tolist()} vs {w[2][:4].tolist()}"


_ref = {}


def ref(lsoa, train, full=True, **kw):
    """full_train (or rename_train) of (lsoa, train), computed once."""
    key = (id(lsoa), tuple(train), full, tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else repr(v))
                                                        for k, v in kw.items())))
    got = _ref.get(key)
    if got is None:
        got = _ref[key] = ((lsoa, kw), (full_train if full else rename_train)(lsoa, train, **kw))
    return got[1]


def run(lsoa, trains, **kw):
    from semantic_merge_amd._lib import DeviceScreenTrains
    db = DeviceScreenTrains(lsoa, trains, fill=FILL, **kw)
    db.run()
    return db, db.raw()


def check(db, raw, label, failed=(), truncated=(), full=True, **kw):
    """Trains of `failed` report -1, -1 and wrote nothing; every other train equals the oracle
    step by step (steps of `truncated`, by global step index: the oracle's first records, the
    full count); no word outside the counts and the steps' written records was touched."""
    res = db.results(raw)
    fill32, fill64 = np.int32(FILL), np.int64(FILL)
    wrote = {name: np.zeros(len(raw[name]), bool) for name in ("conf", "counts", "step_counts")}
    for t, train in enumerate(db.trains):
        k, landed = (int(x) for x in raw["counts"][2 * t: 2 * t + 2])
        wrote["counts"][2 * t: 2 * t + 2] = True
        if t in failed:
            assert (k, landed) == (-1, -1), f"{label}: train {t} reports {(k, landed)}, not -1"
            continue
        assert not isinstance(res[t], int), f"{label}: train {t} failed with counts {res[t]}"
        w = ref(db.lsoa, train, full=full, **kw)
        assert res[t][:2] == w[:2], f"{label}: train {t}: (renames, landed) {res[t][:2]}, not {w[:2]}"
        g0 = int(db.train_off[t])
        assert len(res[t][2]) == len(w[2]), f"{label}: train {t}: steps"
        for s, (got, exp) in enumerate(zip(res[t][2], w[2])):
            g = g0 + s
            c, cap = int(db.conf_off[g]), int(db.conf_off[g + 1] - db.conf_off[g])
            assert got[:2] == exp[:2], f"{label}: train {t} step {s}: (renames, outcome) {got[:2]}, not {exp[:2]}"
            recs = exp[2]
            if g in truncated:
                assert exp[1] > cap, f"{label}: train {t} step {s} is not truncated"
                recs = recs[:cap]
            assert np.array_equal(got[2], recs), f"{label}: train {t} step {s}: conflict records differ"
            wrote["conf"][2 * c: 2 * (c + len(recs))] = True
            wrote["step_counts"][2 * g: 2 * g + 2] = True
    for name in wrote:
        fill = fill64 if raw[name].dtype == np.int64 else fill32
        bad = np.flatnonzero(~wrote[name] & (raw[name] != fill))
        assert not len(bad), f"{label}: {name} written outside the valid regions, at {bad[:5].tolist()}"
    return res
