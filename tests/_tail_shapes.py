"""Shapes for the tail of a merge (walk, per-symbol tables, packed final-state table, emit)
at its geometry edges: symbol sets on the bucket boundaries of the tables, logs of an exact
op count on both sides of the skip-mode thresholds, value ids of exact bit widths, symbols
that collide in the small plan's hash table, and one-symbol rename chains.  Plain numpy, no
GPU import: tests/test_tail_premise.py proves on the CPU that each shape has the edge it is
named for, tests/test_gpu_tail_edges.py runs them."""
import numpy as np

from semantic_merge_amd import synth
from semantic_merge_amd.marshal import SoA

MOVE = synth.KIND_RANK["moveDecl"]
RENAME = synth.KIND_RANK["renameSymbol"]

# csrc/smx_tables.h and csrc/smx_compose.hip (tb_geometry, launch_tail)
TB_WIDTH, TB_MAXBK, TB_NBK_TGT, TB_TILE = 4096, 1024, 256, 16384
TB_OVERLAP_MIN, TB_UNSKIP_MAXN = 1 << 18, 1 << 22
HASH_MUL = 2654435761  # csrc/smx_small.h slot_of

# moves and renames in equal parts: 40 000 ops give more than 16 384 moves (a tile of moves
# alone), a tile that holds the last moves and the first renames, and a tile of renames alone
TAIL_MIX = (("renameSymbol", 0.45), ("moveDecl", 0.45), ("editStmtBlock", 0.06), ("addDecl", 0.02),
            ("deleteDecl", 0.01), ("modifyImport", 0.01))
BASE_SYMBOLS = 1024  # symbols of the synthetic log before remap (more than any edge set holds)

N_SERIAL = 40_000  # ops of the geometry and packing cases: serial tables, the scatter reads the skip bits
GEOMETRY_SYMS = (1, 255, 256, 257, 65_536, 65_537, 1_048_576, 1_048_577, 4_190_209, 4_194_304, 4_194_305,
                 16_777_217)
SKIP_CASES = ((262_143, 4_194_304), (262_144, 4_194_304), (262_143, 3000), (262_144, 3000),
              (4_194_304, 4_194_304), (4_194_305, 4_194_304))  # (n, n_sym)
PACK_SYMS = (3000, 1_048_577)
PACK_WIDTHS = ((16, 16, 16), (17, 16, 16), (31, 1, 16), (1, 31, 16), (22, 21, 21), (22, 22, 21), (32, 31, 1),
               (32, 32, 1))
PACK_ATOMIC = (4_194_305, (16, 16, 16))  # a packable shape on the atomic path: unpacked entries
CHAIN_LENGTHS = tuple(range(120, 136)) + tuple(range(250, 263))
WIN_TGT = 1792  # csrc/smx_window.h: the presorted windows' target size


def geometry(n_sym):
    """(width, nbk, bucketed) as tb_geometry computes them."""
    width = min(max(-(-n_sym // TB_NBK_TGT), 1), TB_WIDTH)
    nbk = -(-n_sym // width)
    return width, nbk, nbk <= TB_MAXBK


def skip_mode(n, n_sym):
    """launch_tail's keep_skip for n ops (0 on the atomic path, which has no scatter)."""
    if not geometry(n_sym)[2] or n < TB_OVERLAP_MIN:
        return 0
    return 2 if n <= TB_UNSKIP_MAXN else 1


def sort_passes(n_sym):
    """Digit passes of run_mvprefix's sort by symbol: one per byte of n_sym - 1 up to its
    highest non-zero byte (a zero byte below it is sorted too)."""
    return sum(((n_sym - 1) >> (8 * d)) != 0 for d in range(4))


def describe(n, n_sym):
    """One line of the geometry table: what a case of n ops over n_sym symbols is meant to hit."""
    width, nbk, bucketed = geometry(n_sym)
    last = n_sym - (nbk - 1) * width
    mode = ("0: the scatter reads the skip bits", "1: k_tb_unskip kills records",
            "2: the reduce reads the skip bits")[skip_mode(n, n_sym)] if bucketed else "-: k_tab_atomic reads the skip bits"
    return (f"TAIL n={n} n_sym={n_sym} width={width} nbk={nbk} last_bucket={last}{'' if last == width else ' (partial)'} "
            f"path={'bucketed' if bucketed else 'atomic'} keep_skip={mode} sort_passes={sort_passes(n_sym)}")


def byte_pairs(n_sym):
    """{d: (s, t)} for every digit d that run_mvprefix sorts: two symbols below n_sym that
    differ only in byte d."""
    out = {}
    for d in range(4):
        if ((n_sym - 1) >> (8 * d)) == 0:
            continue
        lo = 5 if d and ((n_sym - 1 - 5) >> (8 * d)) >= 1 else 0
        k = min(255, (n_sym - 1 - lo) >> (8 * d))
        out[d] = (lo, lo + (k << (8 * d)))
    return out


def edge_symbols(n_sym):
    """Sorted unique u32 symbols below n_sym: the first and last symbol of bucket 0, of the
    last bucket and of up to 300 buckets spread evenly between them; n_sym - 1 and n_sym - 2;
    symbols at both ends of a 21-entry line of the 6-byte final-state entries (s % 21 in
    {0, 20}) at the start, the middle and the end of the table; byte_pairs(n_sym)."""
    width, nbk, _ = geometry(n_sym)
    bks = np.unique(np.concatenate([[0, nbk - 1], np.linspace(0, nbk - 1, min(nbk, 300)).astype(np.int64)]))
    syms = [bks * width, np.minimum((bks + 1) * width, n_sym) - 1, [n_sym - 1, n_sym - 2]]
    for line in (0, n_sym // 42, (n_sym - 1) // 21 - 1, (n_sym - 1) // 21):
        syms.append([21 * line, 21 * line + 20, 21 * line + 21])
    syms.extend(byte_pairs(n_sym).values())
    s = np.unique(np.concatenate([np.asarray(x, np.int64) for x in syms]))
    return s[(s >= 0) & (s < n_sym)].astype(np.uint32)


def _shuffled_edge(n_sym, seed):
    edge = edge_symbols(n_sym)
    return edge[np.random.default_rng(seed).permutation(len(edge))]


def remap(soa, n_sym, seed):
    """soa's symbols mapped onto edge_symbols(n_sym) (old symbol mod the set's size, the set
    in an order shuffled by seed; not injective when soa has more symbols than the set) and
    soa.n_sym set; in place.  Every symbol keeps its ops, spread over the whole log."""
    edge = _shuffled_edge(n_sym, seed)
    soa.sym = edge[soa.sym.astype(np.int64) % len(edge)]
    soa.n_sym = int(n_sym)
    return soa


def tail_log(n, n_sym, seed, none_moves=True):
    """A log of exactly n ops with ordered timestamps (the presorted plan) over
    edge_symbols(n_sym): moves and renames in equal parts (TAIL_MIX); half of the rename pairs
    (A op k, B op k) retargeted to one symbol, two ops per millisecond and branch, so that most of
    them meet as heads and conflict; with none_moves a third of the moves without an address
    and, independently, a quarter without a file.

    Up to 64 symbols (half of them at most) get a pinned ending: the last renames of such a
    symbol are one pair (A op k, B op k) with no other rename in their millisecond, so that
    the pair conflicts and the symbol's last rename is a skipped one; with none_moves its last
    move has an address and no file, the one before it a file."""
    spec = synth.LiftSpec(n, BASE_SYMBOLS, seed, ops_per_ms=2, divergent=0.5, rename_overlap=1.0, mix=TAIL_MIX)
    soa = synth.lift_soa(synth.lift_logs(spec))
    edge = _shuffled_edge(n_sym, seed)
    used = np.sort(edge[np.bincount(soa.sym.astype(np.int64) % len(edge), minlength=len(edge)) > 0])
    soa = remap(soa, n_sym, seed)
    assert soa.n == n and abs(soa.n_a - soa.n_b) <= 1
    rng = np.random.default_rng(seed + 1)
    pinned = rng.choice(used, min(64, len(used) // 2), replace=False)
    if len(pinned):
        free = np.setdiff1d(used, pinned)
        ren = soa.kind == RENAME
        m = min(soa.n_a, soa.n_b) & ~1
        k = np.arange(max(m - (1 << 15), 0), m)   # (the last ops hold pairs enough)
        alone = ren[k] & ren[soa.n_a + k] & ~ren[k ^ 1] & ~ren[soa.n_a + (k ^ 1)]
        ks = k[alone][-len(pinned):]
        assert len(ks) == len(pinned)
        for lo, hi in ((ks[0] & ~1, soa.n_a), (soa.n_a + (ks[0] & ~1), soa.n)):   # no other rename of them from there on
            late = lo + np.flatnonzero(ren[lo:hi] & np.isin(soa.sym[lo:hi], pinned))
            soa.sym[late] = rng.choice(free, len(late))
        soa.sym[ks] = soa.sym[soa.n_a + ks] = pinned
    if none_moves:
        # the pinned symbols' last two moves in T order (they lie in the last 2^16 ops of a branch)
        z = np.concatenate([np.arange(max(soa.n_a - (1 << 16), 0), soa.n_a),
                            np.arange(soa.n_a + max(soa.n_b - (1 << 16), 0), soa.n)])
        z = z[(soa.kind[z] == MOVE) & np.isin(soa.sym[z], pinned)]
        z = z[np.lexsort((z, soa.oid_lo[z], soa.oid_hi[z], soa.ts[z]))]
        last2 = [z[soa.sym[z] == s][-2:] for s in pinned.tolist()]
        last2 = np.array([x for x in last2 if len(x) == 2], np.int64).reshape(-1, 2)
        keep_a, keep_f = soa.v0[last2[:, 1]].copy(), soa.v1[last2[:, 0]].copy()
        mv = np.flatnonzero(soa.kind == MOVE)
        soa.v0[mv[rng.random(len(mv)) < 1 / 3]] = -1
        soa.v1[mv[rng.random(len(mv)) < 1 / 4]] = -1
        soa.v0[last2[:, 1]], soa.v1[last2[:, 1]], soa.v1[last2[:, 0]] = keep_a, -1, keep_f
    return soa


def _narrow(vals, width, rng):
    """An injective map of the distinct non-negative ids `vals` into ids v with v + 1 of at
    most `width` bits, at least one of exactly `width` bits (width 32: 2^31 - 1 itself).
    Where there are more ids than such values (width 1 holds only id 0) the map wraps."""
    top = 1 << (width - 1)       # v + 1 in [1, 2 * top - 1]; v + 1 >= top has the top bit
    room = top if width == 32 else 2 * top - 1   # ids are i32: v <= 2^31 - 1
    k = len(vals)
    if k > room:
        new = np.arange(k, dtype=np.int64) % room
    elif room <= (1 << 22):
        new = rng.permutation(room)[:k].astype(np.int64)
    else:
        new = np.empty(0, np.int64)
        while len(new) < k:
            new = np.unique(np.concatenate([new, rng.integers(0, room, 2 * k, dtype=np.int64)]))
        new = rng.permutation(new)[:k]
    if k and new.max() + 1 < top:
        new[rng.integers(0, k)] = top - 1 + (0 if width == 32 else rng.integers(0, top))
        assert len(np.unique(new)) == min(k, room)
    return dict(zip(vals.tolist(), new.tolist()))


def with_value_widths(soa, wa, wf, wc, seed):
    """The non-negative table values rewritten (in place) so that the bit widths of the OR of
    value + 1 are exactly (wa, wf, wc): the moves' v0 (newAddress), the moves' v1 (newFile)
    and the renames' v1 (the name's string id), as marshal.py fills them and k_window_f
    accumulates them.  Each column goes through an injective map where its width leaves room.
    The renames' v0 (the equality class of the name, which alone decides a conflict and is
    no table value) stays: two classes may share a string id, as 1 and "1" do."""
    rng = np.random.default_rng(seed)
    for col, kind, width in ((soa.v0, MOVE, wa), (soa.v1, MOVE, wf), (soa.v1, RENAME, wc)):
        idx = np.flatnonzero((soa.kind == kind) & (col >= 0))
        assert len(idx) and 1 <= width <= 32
        vals, inv = np.unique(col[idx], return_inverse=True)
        m = _narrow(vals, width, rng)
        col[idx] = np.array([m[v] for v in vals.tolist()], np.int64)[inv].astype(np.int32)
    return soa


def value_widths(soa):
    """(wa, wf, wc) as k_window_f and fin_pack_of compute them: OR of value + 1 over the
    moves' v0, the moves' v1 and the renames' v1 (None adds nothing), then the bit width."""
    def w(col, kind):
        v = col[soa.kind == kind].astype(np.int64) + 1
        return int(np.bitwise_or.reduce(v)).bit_length() if len(v) else 0
    return w(soa.v0, MOVE), w(soa.v1, MOVE), w(soa.v1, RENAME)


def hash_prefix(sym, bits=12):
    """The top `bits` bits of the small plan's symbol hash."""
    return ((np.asarray(sym, np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def colliding_symbols(count, n_sym):
    """`count` distinct symbols below n_sym whose (s * 2654435761) mod 2^32 share their top 12
    bits: one home slot in the small plan's 4096-slot table, and in the smaller tables of the
    batch classes (a prefix of those bits)."""
    found, want = [], None
    for lo in range(0, n_sym, 1 << 22):
        s = np.arange(lo, min(lo + (1 << 22), n_sym), dtype=np.uint64)
        h = hash_prefix(s)
        if want is None:
            want = h[min(12345, len(h) - 1)]
        found.append(s[h == want])
        if sum(map(len, found)) >= count:
            break
    out = np.concatenate(found)[:count].astype(np.uint32)
    assert len(out) == count, f"only {len(out)} symbols below {n_sym} share a hash prefix"
    return out


def chain_case(n_ren, seed, interleave):
    """One DivergentRename region as long as the logs: every op renames symbol 0.  A's
    renames all take name class 0; B's class 1 (every head pair conflicts) or, with
    interleave, a random class per rename and interleaved timestamps (equal names do
    not conflict, so the pairing drifts along the chain)."""
    rng = np.random.default_rng(seed)
    na = nb = n_ren
    kind = np.full(na + nb, 1, np.uint8)
    if interleave:
        ts = np.concatenate([np.arange(na, dtype=np.uint64) * 2, np.arange(nb, dtype=np.uint64) * 2 + 1])
    else:
        ts = np.concatenate([np.arange(na, dtype=np.uint64), np.uint64(na) + np.arange(nb, dtype=np.uint64)])
    hi = rng.integers(0, 2**63, size=na + nb, dtype=np.int64).astype(np.uint64)
    lo = rng.integers(0, 2**63, size=na + nb, dtype=np.int64).astype(np.uint64)
    sym = np.zeros(na + nb, np.uint32)
    v0 = np.concatenate([np.zeros(na, np.int32),
                         rng.integers(0, 2, nb).astype(np.int32) if interleave else np.ones(nb, np.int32)])
    v1 = v0.copy()
    return SoA(na, nb, kind, ts, hi, lo, sym, v0, v1, 1, ["a", "b"])


_COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")


def embed(chain, lead, seed):
    """`chain` (chain_case) after `lead` unrelated ops: a presorted log of lead + chain.n ops
    over 41 symbols whose renames of symbol 40 are the chain's, later than every other op, so
    that the chain's region lies across the window boundaries behind the lead."""
    soa = synth.lift_soa(synth.lift_logs(synth.LiftSpec(lead, 40, seed, mix=synth.ADVERSARIAL_MIX)))
    t0 = soa.ts.max() + np.uint64(1000)
    parts = {c: [] for c in _COLS}
    for s_lo, s_n, c_lo, c_n in ((0, soa.n_a, 0, chain.n_a), (soa.n_a, soa.n_b, chain.n_a, chain.n_b)):
        for c in _COLS:
            tail = np.asarray(getattr(chain, c))[c_lo:c_lo + c_n]
            if c == "ts":
                tail = tail + t0
            elif c == "sym":
                tail = np.full(c_n, 40, np.uint32)
            elif c in ("v0", "v1"):
                tail = tail + np.int32(200_000)  # names of the chain alone
            parts[c].append(np.asarray(getattr(soa, c))[s_lo:s_lo + s_n])
            parts[c].append(tail.astype(getattr(soa, c).dtype))
    cols = [np.concatenate(parts[c]) for c in _COLS]
    return SoA(soa.n_a + chain.n_a, soa.n_b + chain.n_b, *cols, 41, [], soa.ts_mode, soa.id_mode)


def conflict_regions(k, n_regions=24, filler=40, seed=0):
    """Logs of renames whose DivergentRename regions have exactly k conflicts: per region one
    symbol, k renames by A and k by B with pairwise different names at timestamps that pair
    them off (A's i-th against B's i-th), then `filler` renames of symbols that only one
    branch renames."""
    rng = np.random.default_rng(seed)
    cols = {side: {c: [] for c in ("ts", "sym", "v0")} for side in (0, 1)}
    t = 1000
    for r in range(n_regions):
        for i in range(k):
            for side in (0, 1):
                cols[side]["ts"].append(t + i)
                cols[side]["sym"].append(r)
                cols[side]["v0"].append(2 * (r * k + i) + side)
        t += k
        for i in range(filler):
            side = (r + i) % 2
            cols[side]["ts"].append(t + i)
            cols[side]["sym"].append(n_regions + 2 * (i % 8) + side)
            cols[side]["v0"].append(100_000 + i)
        t += filler
    na, nb = len(cols[0]["ts"]), len(cols[1]["ts"])
    n = na + nb
    cat = lambda c, dt: np.concatenate([np.asarray(cols[0][c], dt), np.asarray(cols[1][c], dt)])  # noqa: E731
    v0 = cat("v0", np.int32)
    return SoA(na, nb, np.full(n, RENAME, np.uint8), cat("ts", np.uint64),
               rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64),
               rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64),
               cat("sym", np.uint32), v0, v0.copy(), n_regions + 16, [])
