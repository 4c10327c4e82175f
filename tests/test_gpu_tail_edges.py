"""GPU parity of the tail of a merge (walk, per-symbol tables, packed final-state table, emit)
at its geometry edges, against the CPU oracle: the bucket geometry of the tables up to the
full 4096-symbol width and 1024 buckets and over into the atomic path, the three ways the
tables pass over skipped renames on both sides of their op-count thresholds, the packing of
the final-state table at the sums of widths where its entry size changes, the digit passes
of the None-move prefix sort, symbols that collide in the small plan's hash table, and
regions on both sides of the walk's scan, replay and staging thresholds.
tests/test_tail_premise.py proves on the CPU that the shapes (tests/_tail_shapes.py) have
these edges."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd._lib import DeviceCompose, compose_soa, compose_soa_many, set_small_limit

import _tail_shapes as ts
from _shapes import pick
from _util import _eq_soa

pytestmark = pytest.mark.gpu

_large = {}
_LARGE_LAST = max(ts.SKIP_CASES)


def _case(n, n_sym):
    """(log, oracle result); the logs of 4M ops are built once (the premise of every case:
    tests/test_tail_premise.py on the same (n, n_sym, seed))."""
    if n < (1 << 22):
        soa = ts.tail_log(n, n_sym, 1)
        return soa, oracle.compose(soa)
    if (n, n_sym) not in _large:
        soa = ts.tail_log(n, n_sym, 1)
        _large[(n, n_sym)] = (soa, oracle.compose(soa))
    return _large[(n, n_sym)]


def _run(soa, ref, label, plan="presorted"):
    dc = DeviceCompose(soa)
    dc.run()
    _eq_soa(dc.results(), ref, label)
    assert dc.last_plan() == plan, label


@pytest.mark.parametrize("n_sym", ts.GEOMETRY_SYMS)
def test_table_geometry(n_sym):
    """40 000 ops (serial tables, the scatter reads the skip bits), None-valued moves, over the
    bucket edges of n_sym symbols: width 1 and one bucket; 255, 256 and 257 symbols around the
    target bucket count; 65 536 / 65 537 (two and three prefix-sort passes); width 4096 with
    256 and 257 buckets; 1023 full buckets and one of a single symbol; 1024 buckets, the last
    bucketed size; the first atomic size; and 2^24 + 1 symbols (atomic, four sort passes: its
    oracle and workspace take 0.2 s of host time)."""
    print(ts.describe(ts.N_SERIAL, n_sym))
    soa, ref = _case(ts.N_SERIAL, n_sym)
    _run(soa, ref, f"n_sym={n_sym}")


@pytest.mark.parametrize("n,n_sym", ts.SKIP_CASES)
def test_table_skip_modes(n, n_sym):
    """Both sides of 2^18 ops (the scatter reads the skip bits / the scatter runs beside the
    walk and the reduce reads them) and of 2^22 ops (... / k_tb_unskip kills the records), at
    1024 buckets of 4096 symbols and, for the first boundary, at 250 buckets of 12."""
    print(ts.describe(n, n_sym))
    soa, ref = _case(n, n_sym)
    _run(soa, ref, f"n={n} n_sym={n_sym}")
    if (n, n_sym) == _LARGE_LAST:
        _large.clear()


@pytest.mark.parametrize("n_sym", ts.PACK_SYMS)
@pytest.mark.parametrize("widths", ts.PACK_WIDTHS, ids=lambda w: "-".join(map(str, w)))
def test_fin_pack_widths(widths, n_sym):
    """Final-state entries of 6 bytes up to 48 bits, 8 bytes up to 64, int4 beyond, at the
    sums 48, 49, 64 and 65; unequal widths; 2^31 - 1 as a value.  The symbols include both
    ends of 21-entry lines of the 6-byte layout."""
    soa = ts.with_value_widths(ts.tail_log(ts.N_SERIAL, n_sym, 1), *widths, 3)
    print(f"{ts.describe(ts.N_SERIAL, n_sym)} widths={widths} sum={sum(widths)}")
    _run(soa, oracle.compose(soa), f"n_sym={n_sym} widths={widths}")


def test_fin_pack_atomic_path_unpacked():
    """Widths that would pack, beyond the bucketed sizes: k_finalize writes int4 entries and
    the emit has to read them as such."""
    n_sym, widths = ts.PACK_ATOMIC
    assert not ts.geometry(n_sym)[2] and sum(widths) <= 48
    soa = ts.with_value_widths(ts.tail_log(ts.N_SERIAL, n_sym, 1), *widths, 3)
    print(f"{ts.describe(ts.N_SERIAL, n_sym)} widths={widths} sum={sum(widths)}")
    _run(soa, oracle.compose(soa), f"atomic path, widths={widths}")


@pytest.fixture
def small_limit():
    old = set_small_limit(2048)
    yield set_small_limit
    set_small_limit(old)


def _collision_log(n_symbols):
    """2048 ops (renames, moves with None values, other ops) whose symbols all share one home
    slot of the small plan's hash table: one symbol per op, or 64 symbols of 32 ops each.  The
    symbol space ends at the largest symbol found (some 2^23 with 2048 symbols: the atomic
    tables in the window plans; some 2^18 with 64)."""
    soa = synth.lift_soa(synth.lift_logs(synth.LiftSpec(2048, n_symbols, 91, ops_per_ms=3, divergent=0.5,
                                                        rename_overlap=1.0, mix=ts.TAIL_MIX)))
    if n_symbols == 2048:
        soa.sym = np.random.default_rng(7).permutation(2048).astype(np.uint32)
    soa.sym = ts.colliding_symbols(n_symbols, 2**30)[soa.sym]
    soa.n_sym = int(soa.sym.max()) + 1   # (2^30 symbols would take a 28 GiB workspace in the window plans)
    mv = np.flatnonzero(soa.kind == ts.MOVE)
    soa.v0[mv[::3]] = -1
    soa.v1[mv[1::4]] = -1
    return soa


@pytest.mark.parametrize("n_symbols", [2048, 64])
def test_small_plan_hash_collisions(small_limit, n_symbols):
    """Every symbol probes from the same slot: chains of up to 2048 slots, in the small plan
    (one workgroup, linear probing), in the window plans on the same log, and cut to 150 and
    1000 ops in one batch (the batch classes' smaller tables)."""
    soa = _collision_log(n_symbols)
    assert len(np.unique(soa.sym)) == n_symbols and len(np.unique(ts.hash_prefix(soa.sym))) == 1
    ref = oracle.compose(soa)
    assert n_symbols == 2048 or len(ref[4]) > 0
    _run(soa, ref, f"{n_symbols} colliding symbols, small plan", plan="small")
    small_limit(0)
    _eq_soa(compose_soa(soa), ref, f"{n_symbols} colliding symbols, window plans")
    assert DeviceCompose.last_plan() != "small"
    small_limit(2048)
    cuts = []
    for m in (150, 1000):
        keep_a, keep_b = np.arange(soa.n_a) < m // 2, np.arange(soa.n_b) < m - m // 2
        cuts.append(pick(soa, keep_a, keep_b))
    for cut, got in zip(cuts, compose_soa_many(cuts)):
        assert not isinstance(got, int), f"merge of {cut.n} ops failed with counts {got}"
        _eq_soa(got, oracle.compose(cut), f"{n_symbols} colliding symbols, batch of {cut.n} ops")


@pytest.mark.parametrize("interleave", [False, True])
def test_walk_thresholds(small_limit, interleave):
    """One-symbol regions of 120..135 and 250..262 renames per branch (WALK_SCAN and
    REPLAY_CAP are 256 steps; a step consumes one rename of a branch, or one of each), through
    the window plans: alone, and behind unrelated ops so that the region lies across the
    window boundary at merged position 2 * 1792 (k_boundary).  The lead is 3584 - L ops, not
    a fixed 3000: behind 3000 ops no chain of these lengths reaches the boundary."""
    small_limit(0)
    for L in ts.CHAIN_LENGTHS:
        chain = ts.chain_case(L, 3, interleave)
        ref = oracle.compose(chain)
        got = compose_soa(chain)
        _eq_soa(got, ref, f"chain L={L} interleave={interleave}")
        assert DeviceCompose.last_plan() != "small"
        emb = ts.embed(chain, 2 * ts.WIN_TGT - L, 5)
        _run(emb, oracle.compose(emb), f"embedded chain L={L} interleave={interleave}")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_walk_staged_region_conflicts(small_limit, k):
    """Regions of exactly k conflicts (RS_CONF = 2: regions of up to two conflicts are staged
    beside their candidate, longer ones replayed): the conflict list and, through the emitted
    order, the skips."""
    small_limit(0)
    soa = ts.conflict_regions(k)
    ref = oracle.compose(soa)
    assert len(ref[4]) == 24 * k and len(ref[0]) == soa.n - 48 * k
    got = compose_soa(soa)
    assert DeviceCompose.last_plan() != "small"
    _eq_soa(got, ref, f"regions of {k} conflicts")
