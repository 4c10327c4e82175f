"""RGA batches for the replay's edges: lists of exact sizes whose key components come from
alphabets of 2 to 4 letters, so two events of one list tie at every level of the key --
anchor, t, author, opid_hi, opid_lo and the whole key (synth.rga_batch draws t from 2^40
values and uuid-like opids: its events never tie below the top half of t)."""
import numpy as np

from semantic_merge_amd.crdt import RgaBatch

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# every list size at which the replay takes another path: one event per lane up to 64,
# K = 2..4 events per lane up to 256 (k_rga_wave), 257..512 (k_rga_wave2), longer lists
# (k_rga_big, its block sort padded to powers of two), and a list far beyond
SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
OPS = (0.55, 0.25, 0.20)  # insert, move, delete

# regime -> (anchors, t values)
#  narrow   anchor and t ranges fit beside the event bits: the packed 32-bit sort; equal
#           top halves of t (-1 alone, 0 and 1 together, 2^32 alone) with different low halves
#  wide     the 64-bit sort; t compared as signed; (0xFFFFFFFF, INT64_MAX) makes key word 0
#           equal to the sorting network's padding value
#  one_key  every event has the same key: one tie run ordered by creation index alone
REGIMES = {
    "narrow": ((0, 1), (-1, 0, 1, 1 << 32)),
    "wide": ((0, 0xFFFFFFFF), (I64_MIN, -1, 0, I64_MAX)),
    "one_key": ((1,), (1,)),
}
AUTHORS = (0, 3)
OPID_HI = (5, 1 << 63)
OPID_LO = (0, (1 << 64) - 1)


def events(list_id, n_lists, seed, regime, ops=OPS, values_per_list=None):
    """An RgaBatch over the given list ids (stream order = index order) with tie-heavy
    keys.  Values: values_per_list per list, by default about size / 8 and at least 2;
    value ids interned in first-seen order, like synth.rga_batch."""
    rng = np.random.default_rng(seed)
    lid = np.asarray(list_id, np.int64)
    n = lid.size
    anchors, ts = REGIMES[regime]
    one = regime == "one_key"
    pick = lambda alphabet, dt: np.asarray(alphabet, dt)[rng.integers(0, len(alphabet), size=n)]
    op = rng.choice(3, size=n, p=np.asarray(ops, np.float64) / sum(ops)).astype(np.uint8)
    anchor = pick(anchors, np.uint32)
    t = pick(ts, np.int64)
    author = pick(AUTHORS[:1] if one else AUTHORS, np.uint32)
    hi = pick(OPID_HI[:1] if one else OPID_HI, np.uint64)
    lo = pick(OPID_LO[:1] if one else OPID_LO, np.uint64)
    if values_per_list is None:
        nv = np.maximum(np.bincount(lid, minlength=n_lists) // 8, 2)
    else:
        nv = np.full(n_lists, values_per_list, np.int64)
    val = lid * (1 << 20) + rng.integers(0, 1 << 20, size=n) % nv[lid] if n else np.zeros(0, np.int64)
    _, first, inv = np.unique(val, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return RgaBatch(int(n_lists), lid.astype(np.uint32), op, rank[inv].astype(np.uint32), anchor, t, author, hi, lo, [])


def tie_batch(sizes=SIZES, seed=7, regime="narrow", ops=OPS, values_per_list=None):
    """List l has exactly sizes[l] events; the lists' events are interleaved by one random
    permutation of the whole stream."""
    sizes = np.asarray(sizes, np.int64)
    lid = np.repeat(np.arange(sizes.size), sizes)
    lid = lid[np.random.default_rng(seed + 1000).permutation(lid.size)]
    b = events(lid, sizes.size, seed, regime, ops, values_per_list)
    assert np.array_equal(np.bincount(b.list_id, minlength=sizes.size), sizes)
    return b


def grouped(b):
    """The same lists with each list's events together, in stream order: a stable sort by
    list id, events re-indexed."""
    p = np.argsort(b.list_id, kind="stable")
    return RgaBatch(b.n_lists, b.list_id[p], b.op[p], b.value[p], b.anchor[p], b.t[p], b.author[p],
                    b.opid_hi[p], b.opid_lo[p], [])


def args(b):
    """oracle.rga's positional arguments."""
    return (b.n_lists, b.list_id, b.op, b.value, b.anchor, b.t, b.author, b.opid_hi, b.opid_lo)


def tie_counts(b, src, offsets, min_events=63):
    """{list: [c1, c2, c3, c4]} for every list of at least min_events events, counted over
    the adjacent elements of its state (src, offsets: a replay's output, any mode):
      c1 pairs equal through t, different in author
      c2 pairs equal through author, different in opid_hi
      c3 pairs equal through opid_hi, different in opid_lo
      c4 pairs with the whole key equal."""
    cols = [np.asarray(c)[src] for c in (b.anchor, b.t, b.author, b.opid_hi, b.opid_lo)]
    sizes = np.bincount(b.list_id, minlength=b.n_lists)
    out = {}
    for l in np.flatnonzero(sizes >= min_events):
        a, e = int(offsets[l]), int(offsets[l + 1])
        eq = [c[a:e][1:] == c[a:e][:-1] for c in cols]
        through = np.logical_and.accumulate(np.array(eq).reshape(5, -1), axis=0)
        out[int(l)] = [int((through[k + 1] & ~eq[k + 2]).sum()) for k in range(3)] + [int(through[4].sum())]
    return out


def assert_ties(b, src, offsets):
    """The coverage condition of the tie tests: every list of at least 63 events has all
    four kinds of adjacent tie in its state."""
    counts = tie_counts(b, src, offsets)
    assert counts, "no list of 63 events or more"
    for l, c in counts.items():
        assert min(c) >= 1, f"list {l}: adjacent ties by level {c}"
    return counts
