"""The candidate rule of smx_screen_candidates (include/smx.h) restated in numpy over a LogsSoA,
and a generator of sparse logs: logs over a symbol space large enough that some pairs share a
renamed symbol and some do not."""
import numpy as np

from semantic_merge_amd import synth
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, LogsSoA

RENAME = synth.KIND_RANK["renameSymbol"]
N_KINDS = 18
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")
DT = dict(kind=np.uint8, ts=np.uint64, oid_hi=np.uint64, oid_lo=np.uint64, sym=np.uint32, v0=np.int32, v1=np.int32)


def logs_soa(parts, n_sym, head=0, tail=0):
    """The LogsSoA of one-branch SoAs, one log each, in order.  One offset array cannot leave
    room between two logs, so the entries that no log covers are `head` in front of the first
    log and `tail` after the last one: kind 255, symbol 0xFFFFFFFF, v0 -1."""
    gap = {"kind": 0xFF, "sym": 0xFFFFFFFF, "v0": -1, "v1": -1}
    cols = [np.concatenate([np.full(head, gap.get(c, 0), DT[c])]
                           + [np.asarray(getattr(p, c)).astype(DT[c]) for p in parts]
                           + [np.full(tail, gap.get(c, 0), DT[c])]) for c in COLS]
    off = head + np.concatenate([[0], np.cumsum([p.n for p in parts], dtype=np.int64)]).astype(np.int64)
    return LogsSoA(off, *cols, n_sym, [], TS_ISO, ID_UUID)


def valid_logs(log_off, n_total, kind):
    """smx_screen's rule: a log starts at or after every earlier offset (and at or after 0),
    does not end before it starts, ends inside n_total, and holds no kind >= 18."""
    off = np.asarray(log_off, np.int64)
    L = len(off) - 1
    ok = np.zeros(L, bool)
    pm = 0
    for l in range(L):
        o0, o1 = int(off[l]), int(off[l + 1])
        ok[l] = not (o0 < pm or o1 < o0 or o1 > n_total)
        if ok[l]:
            ok[l] = not (np.asarray(kind[o0:o1]) >= N_KINDS).any()
        pm = max(pm, o0)
    return ok


def rename_sets(lsoa, log_off=None, n_total=None):
    """Per log: None for an invalid log, else {sym: set of v0 (as u32)} over its renames, and
    log_info (-1, or the number of renames)."""
    off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64)
    n_total = lsoa.n_total if n_total is None else n_total
    ok = valid_logs(off, n_total, lsoa.kind)
    sets, info = [], np.full(len(off) - 1, -1, np.int32)
    for l in range(len(off) - 1):
        if not ok[l]:
            sets.append(None)
            continue
        s = slice(int(off[l]), int(off[l + 1]))
        r = np.asarray(lsoa.kind[s]) == RENAME
        info[l] = int(r.sum())
        d = {}
        for sym, v in zip(np.asarray(lsoa.sym[s])[r].astype(np.uint32).tolist(),
                          np.asarray(lsoa.v0[s])[r].astype(np.int32).view(np.uint32).tolist()):
            d.setdefault(sym, set()).add(v)
        sets.append(d)
    return sets, info


def candidates(lsoa, log_off=None, n_total=None):
    """(pairs, log_info): the (i, j), i < j, of valid logs with a symbol that both rename and
    whose v0 over the two logs are not all one class, in ascending order ((n, 2) int32)."""
    sets, info = rename_sets(lsoa, log_off, n_total)
    out = []
    for i in range(len(sets)):
        a = sets[i]
        if not a:
            continue
        for j in range(i + 1, len(sets)):
            b = sets[j]
            if b and any(len(a[s] | b[s]) > 1 for s in a.keys() & b.keys()):
                out.append((i, j))
    return np.asarray(out, np.int32).reshape(-1, 2), info


def spread(soa, space, rng):
    """soa (one branch) with its symbols mapped one to one into [0, space) at random."""
    n_loc = int(soa.n_sym)
    m = rng.choice(space, n_loc, replace=False).astype(np.uint32)
    soa.sym = m[np.asarray(soa.sym).astype(np.int64)]
    soa.n_sym = space
    return soa


def sparse_logs(n_logs, space, seed, lo=10, hi=401, n_loc=8):
    """n_logs logs of lo .. hi - 1 ops in test_gpu_shared's own_logs recipe, each over n_loc
    symbols of its own drawn from [0, space): two logs share a renamed symbol only by chance."""
    from test_gpu_shared import own_logs
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi, n_logs).tolist()
    return logs_soa([spread(s, space, rng) for s in own_logs(n_loc, seed + 1000, sizes)], space)
