"""What the GPU tests of the conflict screens share (test_gpu_screen*.py, test_gpu_cand.py,
test_cand_premise.py): logs given column by column or cut to a number of renames, the oracle's
conflicts computed once per pair, and the checks of a DeviceScreen run."""
import numpy as np

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd._lib import DeviceScreen
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, LogsSoA, SoA

from _shapes import pick

FILL = 0x5A5A5A5A  # what every output word holds before a run that checks the unwritten ones
RENAME = synth.KIND_RANK["renameSymbol"]
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")
DT = dict(kind=np.uint8, ts=np.uint64, oid_hi=np.uint64, oid_lo=np.uint64, sym=np.uint32, v0=np.int32, v1=np.int32)


def logs_soa(parts, n_sym):
    """The LogsSoA of one-branch SoAs, one log each, in order."""
    cols = [np.concatenate([np.asarray(getattr(p, c)).astype(DT[c]) for p in parts]) if parts else np.zeros(0, DT[c])
            for c in COLS]
    off = np.concatenate([[0], np.cumsum([p.n for p in parts], dtype=np.int64)]).astype(np.int64)
    return LogsSoA(off, *cols, n_sym, [], TS_ISO, ID_UUID)


def make_log(kind, ts, hi, lo, sym, v0, n_sym=4):
    """A log given column by column."""
    n = len(kind)
    a = [np.asarray(x, DT[c]) for x, c in zip((kind, ts, hi, lo, sym, v0, v0), COLS)]
    return SoA(n, 0, *a, n_sym, [], TS_ISO, ID_UUID)


def with_renames(soa, r, others=None):
    """soa (one branch) with only its first r renames, and its first `others` other ops
    (default: all of them)."""
    is_r = soa.kind == RENAME
    keep = np.where(is_r, np.cumsum(is_r) <= r, True if others is None else np.cumsum(~is_r) <= others)
    out = pick(soa, keep, np.zeros(0, bool)) if soa.n_b == 0 else pick(soa, np.zeros(0, bool), keep)
    assert int((out.kind == RENAME).sum()) == r, "the base log has too few renames"
    return out


def empty_log(n_sym=4):
    return make_log([], [], [], [], [], [], n_sym)


_ref = {}


def ref(lsoa, i, j):
    """oracle.compose(lsoa.pair(i, j))[4], computed once."""
    key = (id(lsoa), i, j)
    got = _ref.get(key)
    if got is None:
        got = _ref[key] = (lsoa, oracle.compose(lsoa.pair(i, j))[4])
    return got[1]


def check_all(got, lsoa, pairs, label, skip=()):
    assert len(got) == len(pairs)
    for p, ((i, j), g) in enumerate(zip(pairs, got)):
        if p in skip:
            continue
        assert not isinstance(g, int), f"{label}: pair {p} ({i}, {j}) failed with counts {g}"
        want = ref(lsoa, i, j)
        assert g.shape == want.shape and np.array_equal(g, want), f"{label}: pair {p} ({i}, {j})"


def run(lsoa, pairs, **kw):
    ds = DeviceScreen(lsoa, pairs, fill=FILL, **kw)
    ds.run()
    raw = ds.raw()
    return ds, raw, ds.results(raw)


def check_unwritten(ds, raw, label):
    """Nothing is written past a pair's conflicts (or at all, for a failed pair), and
    nothing after the last region."""
    for p in range(ds.n_pairs):
        c, cap = int(ds.conf_off[p]), int(ds.conf_off[p + 1] - ds.conf_off[p])
        nc = min(max(int(raw["counts"][p]), 0), cap)
        assert (raw["conf"][2 * (c + nc): 2 * (c + cap)] == FILL).all(), f"{label}: pair {p}: written past {nc} pairs"
    assert (raw["conf"][2 * int(ds.conf_off[-1]):] == FILL).all(), f"{label}: written after the last region"


def renames_ordered(soa):
    k = soa.kind == RENAME
    key = list(zip(soa.ts[k].tolist(), soa.oid_hi[k].tolist(), soa.oid_lo[k].tolist()))
    return key == sorted(key)
