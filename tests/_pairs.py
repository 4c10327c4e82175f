"""What the smx_compose_pairs GPU tests share: a LogsSoA out of one-branch SoAs (the log
builders are test_gpu_shared.py's), the oracle's result per pair computed once, and the check
of a DevicePairs run: every valid pair equal to the oracle on that pair alone, every failed
pair reporting its code, and every output word outside the valid pairs' counts-long regions
still the canary the rig filled it with."""
import numpy as np

from oracle import oracle
from semantic_merge_amd._lib import DevicePairs
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, LogsSoA

from _util import _eq_soa as _eq

FILL = 0x5A5A5A5A  # what every output word holds before a run
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")
GAP = {"kind": 0xFF, "sym": 0xFFFFFFFF, "v0": -1, "v1": -1}  # invalid: a kernel that read a gap would report -1
RES = ("order", "addr", "file", "ctx")


def gap_log(n):
    """n entries that no pair holds, filled with invalid bytes: a 'log' for logs_soa."""
    return {"gap": n}


def logs_soa(logs, n_sym):
    """The LogsSoA of one-branch SoAs stored one after another (a gap_log(n) among them: n
    invalid entries that are a log of their own, which no pair may hold)."""
    lens = [x["gap"] if isinstance(x, dict) else x.n for x in logs]
    cols = []
    for c in COLS:
        dt = next(np.asarray(getattr(x, c)).dtype for x in logs if not isinstance(x, dict))
        cols.append(np.concatenate([np.full(x["gap"], GAP.get(c, 0), dt) if isinstance(x, dict)
                                    else np.asarray(getattr(x, c)) for x in logs]))
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    return LogsSoA(off, *cols, n_sym, [], TS_ISO, ID_UUID)


_ref = {}


def ref(lsoa, i, j):
    """oracle.compose(lsoa.pair(i, j)), computed once."""
    key = (id(lsoa), int(i), int(j))
    got = _ref.get(key)
    if got is None:
        got = _ref[key] = (lsoa, oracle.compose(lsoa.pair(int(i), int(j))))
    return got[1]


def run(lsoa, pairs, **kw):
    db = DevicePairs(lsoa, pairs, fill=FILL, **kw)
    db.run()
    raw = db.raw()
    return db, raw, db.results(raw)


def check(db, raw, label, failed=(), sent_back=(), truncated=()):
    """Pairs of `failed` report -1 and those of `sent_back` -2, and neither wrote anything; every
    other pair equals the oracle (`truncated`: its conflict pairs are the oracle's first ones,
    its count the full one); no word outside the valid pairs' counts-long regions was written."""
    res = db.results(raw)
    wrote = {name: np.zeros(len(raw[name]), bool) for name in RES}
    wrote_conf = np.zeros(len(raw["conf"]), bool)
    for p, (i, j) in enumerate(db.pairs.tolist()):
        k, nc = (int(x) for x in raw["counts"][2 * p: 2 * p + 2])
        if p in failed or p in sent_back:
            want = -1 if p in failed else -2
            assert (k, nc) == (want, want), f"{label}: pair {p} ({i}, {j}) reports {(k, nc)}, not {want}"
            continue
        assert not isinstance(res[p], int), f"{label}: pair {p} ({i}, {j}) failed with counts {res[p]}"
        want = ref(db.lsoa, i, j)
        c, cap = int(db.conf_off[p]), int(db.conf_off[p + 1] - db.conf_off[p])
        if p in truncated:
            assert (k, nc) == (len(want[0]), len(want[4])) and nc > cap, f"{label}: pair {p}: counts {(k, nc)}"
            want = want[:4] + (want[4][:cap],)
        _eq(res[p], want, f"{label}: pair {p} ({i}, {j})")
        r = int(db.res_off[p])
        for name in RES:
            wrote[name][r: r + k] = True
        wrote_conf[2 * c: 2 * (c + min(nc, cap))] = True
    for name in RES:
        bad = np.flatnonzero(~wrote[name] & (raw[name] != np.int32(FILL)))
        assert not len(bad), f"{label}: {name} written outside the pairs' results, at {bad[:5].tolist()}"
    bad = np.flatnonzero(~wrote_conf & (raw["conf"] != np.int32(FILL)))
    assert not len(bad), f"{label}: conflicts written outside the pairs' regions, at {bad[:5].tolist()}"
    return res


def same_bytes(a, b, label):
    """Two lists of per-item results are bit-equal, array by array."""
    assert len(a) == len(b), label
    for m, (x, y) in enumerate(zip(a, b)):
        assert isinstance(x, int) == isinstance(y, int), f"{label}: item {m}"
        if isinstance(x, int):
            assert x == y, f"{label}: item {m}"
            continue
        for name, u, v in zip(RES + ("conflicts",), x, y):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), f"{label}: item {m}: {name} differs"
