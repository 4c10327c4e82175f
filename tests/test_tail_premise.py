"""What tests/test_gpu_tail_edges.py rests on, proved on the CPU from the inputs and the oracle
alone: every shape of tests/_tail_shapes.py has the edge it is named for.  The table geometry
is recomputed as tb_geometry does; the records (a move at its T position, a rename at
nMv + its position among the renames) and their 16 384-record tiles as smx_tables.h lays them
out; kept and skipped renames come from oracle.compose's order.

The floor of 32 symbols (a quarter of the symbols where there are fewer than 128) is a guard
against a vacuous test, not a measurement; it counts symbols that meet all three last-writer
premises at once.  With one symbol the premises cannot hold (see the case's comment).  The
sort passes are counted as run_mvprefix counts them: one per byte of n_sym - 1 up to its
highest non-zero byte, so 65 537 symbols (n_sym - 1 = 0x10000) sort three digits."""
import numpy as np
import pytest

from oracle import oracle

import _tail_shapes as ts

MOVE, RENAME = ts.MOVE, ts.RENAME
CASES = sorted({(ts.N_SERIAL, s) for s in ts.GEOMETRY_SYMS + ts.PACK_SYMS + (ts.PACK_ATOMIC[0],)} | set(ts.SKIP_CASES))


def intended(n_sym):
    """(width, nbk, bucketed, passes) each size is in the lists for."""
    return {1: (1, 1, True, 0), 255: (1, 255, True, 1), 256: (1, 256, True, 1), 257: (2, 129, True, 2),
            3000: (12, 250, True, 2), 65_536: (256, 256, True, 2), 65_537: (257, 256, True, 3),
            1_048_576: (4096, 256, True, 3), 1_048_577: (4096, 257, True, 3),
            4_190_209: (4096, 1024, True, 3), 4_194_304: (4096, 1024, True, 3),
            4_194_305: (4096, 1025, False, 3), 16_777_217: (4096, 4097, False, 4)}[n_sym]


def records(soa, ref):
    """The table records of soa in T order: (op index, symbol, record index r, kept), moves
    first (r = T), then the renames (r = nMv + position among the renames); kept: the op is
    in the oracle's order (a skipped rename is not)."""
    side = (np.arange(soa.n) >= soa.n_a).astype(np.int8)
    t = np.lexsort((np.arange(soa.n), side, soa.oid_lo, soa.oid_hi, soa.ts, soa.kind))
    t = t[(soa.kind[t] == MOVE) | (soa.kind[t] == RENAME)]
    assert (np.diff(soa.kind[t].astype(np.int8)) >= 0).all()
    kept = np.zeros(soa.n, bool)
    kept[ref[0]] = True
    assert kept[t[soa.kind[t] == MOVE]].all()
    return t, soa.sym[t].astype(np.int64), np.arange(len(t)), kept[t]


def last_of(sym_id, r, mask, n_ids):
    """Per symbol id: the largest record index among the masked records, or -1."""
    out = np.full(n_ids, -1, np.int64)
    np.maximum.at(out, sym_id[mask], r[mask])
    return out


@pytest.mark.parametrize("n,n_sym", CASES)
def test_tail_log_has_its_edges(n, n_sym):
    soa = ts.tail_log(n, n_sym, 1)
    ref = oracle.compose(soa)
    assert soa.n == n and soa.n_sym == n_sym and soa.sym.max() < n_sym
    assert (np.diff(soa.ts[:soa.n_a].astype(np.int64)) >= 0).all() and (np.diff(soa.ts[soa.n_a:].astype(np.int64)) >= 0).all()

    # geometry, skip mode and sort passes are the intended ones
    width, nbk, bucketed = ts.geometry(n_sym)
    assert (width, nbk, bucketed, ts.sort_passes(n_sym)) == intended(n_sym)
    assert ts.skip_mode(n, n_sym) == (0 if n < (1 << 18) or not bucketed else 2 if n <= (1 << 22) else 1)
    if n_sym == 4_190_209:
        assert n_sym - (nbk - 1) * width == 1     # 1023 full buckets and one symbol
    edge = ts.edge_symbols(n_sym)
    assert edge.dtype == np.uint32 and (np.diff(edge.astype(np.int64)) > 0).all() and edge[-1] == n_sym - 1
    assert {0, width - 1, (nbk - 1) * width, n_sym - 1, max(n_sym - 2, 0)} <= set(edge.tolist())
    if n_sym > 42:
        assert (edge % 21 == 0).sum() >= 3 and (edge % 21 == 20).sum() >= 3

    op, sym, r, kept = records(soa, ref)
    is_mv = soa.kind[op] == MOVE
    n_mv, n_rec = int(is_mv.sum()), len(op)
    has_a, has_f = is_mv & (soa.v0[op] >= 0), is_mv & (soa.v1[op] >= 0)
    carries = has_a | has_f | (~is_mv & kept)

    # tiles: one of moves alone, one with the last moves and the first renames, one of renames alone
    n_tiles = -(-n_rec // ts.TB_TILE)
    assert n_tiles >= 3 and n_mv >= ts.TB_TILE and n_mv % ts.TB_TILE != 0 and (n_tiles - 1) * ts.TB_TILE >= n_mv

    # buckets: the first and the last have records; beyond 256 buckets, more than 256 have
    bks = np.unique(sym[carries] // width)
    assert bks[0] == 0 and bks[-1] == nbk - 1
    if nbk > 256:
        assert len(bks) > 256
    top = sym == n_sym - 1
    assert (top & (has_a | has_f)).any() and (top & ~is_mv & kept).any()

    # last-writer ordering, per symbol
    ids, sid = np.unique(sym, return_inverse=True)
    k = len(ids)
    tile, loc = r // ts.TB_TILE, r % ts.TB_TILE
    ren_kept, ren_any = ~is_mv & kept, ~is_mv
    last_kept = last_of(sid, r, ren_kept, k)
    lk = last_kept[sid]
    earlier_higher = ren_kept & (lk >= 0) & (tile < lk // ts.TB_TILE) & (loc > lk % ts.TB_TILE)
    tiles_cross = np.zeros(k, bool)
    tiles_cross[sid[earlier_higher]] = True     # the last writer's in-tile index is below an earlier writer's
    last_a, last_f = last_of(sid, r, has_a, k), last_of(sid, r, has_f, k)
    split_moves = (last_a >= 0) & (last_f >= 0) & (last_a != last_f)
    last_ren = last_of(sid, r, ren_any, k)
    skipped_last = (last_kept >= 0) & (last_ren > last_kept)
    good = tiles_cross & split_moves & skipped_last
    floor = min(32, max(k // 4, 1))
    print(f"{ts.describe(n, n_sym)}: {k} symbols, {len(ref[4])} conflicts; last-writer premises "
          f"{tiles_cross.sum()} / {split_moves.sum()} / {skipped_last.sum()}, all three {good.sum()} (floor {floor})")
    if n_sym == 1:
        # one symbol: every head pair conflicts until a branch has no rename left, so the kept
        # renames are the longer side's last ones, all in the last tile; what is left of the
        # premises is that the tables have many writers and skipped renames to pass over
        n_ra, n_rb = int(ren_any[op < soa.n_a].sum()), int(ren_any[op >= soa.n_a].sum())
        assert len(ref[4]) == min(n_ra, n_rb) and 2 <= ren_kept.sum() == abs(n_ra - n_rb)
    else:
        assert good.sum() >= floor

    # several writers per symbol and table (what the atomic path's atomicMax has to order)
    assert (np.bincount(sid[ren_kept], minlength=k) >= 2).sum() >= floor
    assert (np.bincount(sid[has_a], minlength=k) >= 2).sum() >= floor
    assert (np.bincount(sid[has_f], minlength=k) >= 2).sum() >= floor

    # the prefix sort: for every digit it sorts, two symbols that differ in that byte alone,
    # both with None-valued moves
    pairs = ts.byte_pairs(n_sym)
    assert len(pairs) == ts.sort_passes(n_sym)
    none_mv = set(sym[is_mv & ((soa.v0[op] < 0) | (soa.v1[op] < 0))].tolist())
    for d, (s, t) in pairs.items():
        assert s != t and (s ^ t) & ~(0xFF << (8 * d)) == 0 and max(s, t) < n_sym
        assert s in none_mv and t in none_mv, f"digit {d}: symbols {s}, {t}"
    if n_sym > 1:
        assert ((soa.v0 < 0) & (soa.v1 >= 0) & (soa.kind == MOVE)).any() and ((soa.v1 < 0) & (soa.v0 >= 0) & (soa.kind == MOVE)).any()


@pytest.mark.parametrize("n_sym", ts.PACK_SYMS + (ts.PACK_ATOMIC[0],))
def test_value_widths_are_exact(n_sym):
    shapes = ts.PACK_WIDTHS if n_sym in ts.PACK_SYMS else (ts.PACK_ATOMIC[1],)
    base = ts.tail_log(ts.N_SERIAL, n_sym, 1)
    base_conf = oracle.compose(base)[4]
    for wa, wf, wc in shapes:
        soa = ts.tail_log(ts.N_SERIAL, n_sym, 1)
        ts.with_value_widths(soa, wa, wf, wc, 3)
        assert ts.value_widths(soa) == (wa, wf, wc)
        assert np.array_equal((soa.v0 < 0), (base.v0 < 0)) and np.array_equal((soa.v1 < 0), (base.v1 < 0))
        if 32 in (wa, wf):
            assert soa.v0[soa.kind == MOVE].max() == 2**31 - 1 if wa == 32 else True
            assert soa.v1[soa.kind == MOVE].max() == 2**31 - 1 if wf == 32 else True
        # the conflicts are the base log's: the names' equality classes did not move
        assert np.array_equal(oracle.compose(soa)[4], base_conf)
        # injective where the width leaves room: distinct ids stay distinct
        for col, kind, w in ((soa.v0, MOVE, wa), (soa.v1, MOVE, wf), (soa.v1, RENAME, wc)):
            m = (soa.kind == kind) & (col >= 0)
            before = (base.v0 if col is soa.v0 else base.v1)[m]
            room = 2**31 if w == 32 else 2**w - 1
            assert len(np.unique(col[m])) == min(len(np.unique(before)), room)
    sums = sorted({sum(s) for s in ts.PACK_WIDTHS})
    assert sums == [48, 49, 64, 65]


def test_colliding_symbols_share_one_slot():
    for count in (2048, 64):
        s = ts.colliding_symbols(count, 2**30)
        assert s.dtype == np.uint32 and len(np.unique(s)) == count and s.max() < 2**30
        for bits in (12, 11, 9, 7):   # the small plan's table and the batch classes' smaller ones
            assert len(np.unique(ts.hash_prefix(s, bits))) == 1


def test_chains_cross_the_walk_thresholds():
    """Chains of L conflicting renames per branch: lengths on both sides of 128 and 256 (a
    walk step consumes one rename of the region, or one of each branch), alone and across
    the window boundary at merged position 2 * WIN_TGT; regions of exactly 1, 2, 3 conflicts."""
    assert {127, 128, 129, 255, 256, 257} <= set(ts.CHAIN_LENGTHS)
    for L in ts.CHAIN_LENGTHS:
        for inter in (False, True):
            c = ts.chain_case(L, 3, inter)
            nc = len(oracle.compose(c)[4])
            assert (nc == L) if not inter else (0 < nc < L)
            lead = 2 * ts.WIN_TGT - L
            e = ts.embed(c, lead, 5)
            assert e.n == lead + 2 * L and lead < 2 * ts.WIN_TGT < e.n and lead >= 3000
            assert (np.diff(e.ts[:e.n_a].astype(np.int64)) >= 0).all() and (np.diff(e.ts[e.n_a:].astype(np.int64)) >= 0).all()
            ec = oracle.compose(e)[4]
            in_chain = (e.sym[ec[:, 0]] == 40).sum()
            assert in_chain == nc
    for k in (1, 2, 3):
        soa = ts.conflict_regions(k)
        conf = oracle.compose(soa)[4]
        per_region = np.bincount(soa.sym[conf[:, 0]], minlength=24)
        assert (per_region[:24] == k).all() and len(conf) == 24 * k
