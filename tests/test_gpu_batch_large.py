"""GPU parity of the batched compose with SMX_BATCH_LARGE (smx_compose_batch_ex /
smx_compose_batch_shared_ex, csrc/smx_batch_large.h): merges of more than 2048 ops run inside
the batch, one workgroup each, and every merge equals the CPU oracle on that merge alone.  The
sort's tile and level edges, every order of the logs, a walk of several rounds, the chains'
table at its edges, conflict capacities, failed merges between large ones, grid caps, workspace
reuse, the shared form and the Python layers.  Every output word starts as FILL, so the words a
call must not write are checked."""
import dataclasses

import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import (DeviceBatch, DeviceBatchShared, compose_soa_many, compose_soa_shared, lib,
                                     session)
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, SharedSoA

from _batch import check_all, check_unwritten, lift, none_moves, ref
from _shapes import pick
from _util import _eq_soa as _eq, jline, to_ops

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A  # what every output word holds before a run that checks the unwritten ones
MOVE = synth.KIND_RANK["moveDecl"]
RENAME = synth.KIND_RANK["renameSymbol"]
LARGE = _abi.BATCH_LARGE
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")


def split(base, n, n_a):
    """n ops of `base` (whose branches hold at least n ops each): the first n_a of A, the first n - n_a of B."""
    ka, kb = np.zeros(base.n_a, bool), np.zeros(base.n_b, bool)
    ka[:n_a] = True
    kb[:n - n_a] = True
    return pick(base, ka, kb)


def run(soas, **kw):
    db = DeviceBatch(soas, fill=FILL, flags=kw.pop("flags", LARGE), **kw)
    db.run()
    raw = db.raw()
    return db, raw, db.results(raw)


@pytest.fixture(scope="module")
def edges():
    """One op in the second tile, two full tiles, one op in the third, an odd number of runs;
    each with n_a at 0, 1, len - 1 and len."""
    out = []
    for n in (2049, 4096, 4097, 6145):
        base = lift(2 * n, max(n // 25, 2), 500 + n, mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
        out += [split(base, n, n_a) for n_a in (0, 1, n - 1, n)]
    return out


def test_tile_and_level_edges(edges):
    db, raw, res = run(edges)
    check_all(res, edges, "edges")
    check_unwritten(db, raw, edges)
    assert (raw["counts"] != -2).all()


def test_orders():
    dup = lift(5000, 40, 15, mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
    dup.ts[:] = dup.ts[0] + (dup.ts - dup.ts[0]) // np.uint64(64)   # few timestamps ...
    dup.oid_hi[:] = dup.oid_hi % np.uint64(3)                        # ... and ids: side and index decide
    dup.oid_lo[:] = dup.oid_lo % np.uint64(2)
    soas = [lift(5000, 60, 11), lift(5000, 60, 12, shuffle=True, mix=synth.ADVERSARIAL_MIX),
            lift(5000, 30, 13, ops_per_ms=4096, mix=synth.ADVERSARIAL_MIX, divergent=0.3),
            dup, lift(4500, 50, 14, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)]
    assert len(ref(dup)[4]) and len(ref(soas[4])[4])
    check_all(run(soas)[2], soas, "orders")


def test_walk_of_several_rounds():
    soa = lift(6000, 40, 21, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    ren = soa.kind == RENAME
    assert ren[:soa.n_a].sum() > 1024 and ren[soa.n_a:].sum() > 1024
    assert len(ref(soa)[4]) > 64
    sh = lift(6000, 40, 22, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0, shuffle=True)
    db, raw, res = run([soa, sh])
    check_all(res, [soa, sh], "walk")
    check_unwritten(db, raw, [soa, sh])


def test_chains():
    two = lift(4200, 2, 31, mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)  # long per-symbol chains
    full = lift(3000, 3000, 32)                                   # as many symbols as ops: a full table
    rng = np.random.default_rng(33)
    full.sym[:] = rng.permutation(3000).astype(full.sym.dtype)    # ... every op another symbol
    # symbols up to 2^32 - 2: ids are opaque, so the oracle (whose tables are n_sym long) runs on the low ones
    low = lift(3100, 50, 34, mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
    high = dataclasses.replace(low, sym=(np.uint64(2 ** 32 - 2) - low.sym.astype(np.uint64)).astype(low.sym.dtype),
                               n_sym=2 ** 32 - 1)
    assert int(high.sym.max()) == 2 ** 32 - 2 and int(low.sym.min()) == 0
    none = none_moves(lift(4100, 12, 35, ops_per_ms=3), 5)
    one = none_moves(lift(2500, 1, 36, ops_per_ms=3), 6)
    assert ((none.v0 < 0) & (none.kind == MOVE)).any() and ((one.v1 < 0) & (one.kind == MOVE)).any()
    soas = [two, full, none, one]
    check_all(run(soas)[2], soas, "chains")
    check_all(run([high, two], n_sym=2 ** 32 - 1)[2], [low, two], "symbols near 2^32 - 2")


def test_conflict_capacity():
    many = lift(3000, 30, 41, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    after = lift(2600, 30, 42, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    full = ref(many)
    n_conf = len(full[4])
    assert n_conf > 1 and len(ref(after)[4]) > 0
    for cap in (0, 1, n_conf):
        db, raw, res = run([many, after], conflict_caps=[cap, min(after.n_a, after.n_b)])
        assert raw["counts"][:2].tolist() == [len(full[0]), n_conf]  # the full count, the ops complete
        _eq(res[0][:4], full[:4], f"cap {cap}: composed ops of the truncated merge")
        assert np.array_equal(res[0][4], full[4][:cap])
        _eq(res[1], ref(after), f"cap {cap}: the merge after it")
        assert (raw["conf"][2 * (cap + len(ref(after)[4])):] == FILL).all()


def test_mixed_batch_with_failed_merges():
    big = [lift(n, 8, 600 + n, mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0) for n in (2500, 4300, 3000)]
    small = [lift(n, 8, 700 + n, mix=synth.ADVERSARIAL_MIX, divergent=0.3) for n in (120, 1100, 2048)]
    empty = pick(small[0], np.zeros(small[0].n_a, bool), np.zeros(small[0].n_b, bool))
    bad_na, bad_kind, bad_sym = lift(2600, 8, 801), lift(4200, 8, 802), lift(2300, 8, 803)
    bad_kind.kind[4199] = 18   # in the last tile
    bad_sym.sym[2299] = 8      # = n_sym
    soas = [big[0], small[0], bad_na, big[1], empty, bad_kind, small[1], bad_sym, big[2], small[2]]
    n_a = [s.n_a for s in soas]
    n_a[2] = bad_na.n + 1
    failed = (2, 5, 7)
    db, raw, res = run(soas, n_a=n_a, n_sym=8)
    for m, s in enumerate(soas):
        if m in failed:
            assert raw["counts"][2 * m: 2 * m + 2].tolist() == [-1, -1], f"merge {m}"
        else:
            _eq(res[m], ref(s), f"valid merge {m}")
    check_unwritten(db, raw, soas, failed)
    assert raw["counts"][8:10].tolist() == [0, 0]


def test_grid_caps_and_workspace_reuse(edges):
    soas = edges[2:7] + [lift(300, 9, 51, mix=synth.ADVERSARIAL_MIX, divergent=0.3)]
    raws = {}
    for cap in (0, 1, 2):   # one workgroup runs large merge after large merge
        db, raws[cap], res = run(soas, grid_cap=cap)
        check_all(res, soas, f"grid_cap {cap}")
    for cap in (1, 2):
        for name, a in raws[0].items():
            assert np.array_equal(a, raws[cap][name]), f"grid_cap {cap}: {name} differs from grid_cap 0"
    # one workspace: a flagged call, a flags-0 call, a flagged call
    db = DeviceBatch(soas, fill=FILL, flags=LARGE)
    for flags in (LARGE, 0, LARGE):
        for name in db._OUT:
            getattr(db, name).fill_(FILL)
        db.flags = flags
        db.run()
        raw = db.raw()
        if flags:
            for name, a in raws[0].items():
                assert np.array_equal(a, raw[name]), f"reused workspace: {name}"
        else:
            assert [r == -2 if s.n > 2048 else not isinstance(r, int) for r, s in zip(db.results(raw), soas)] \
                == [True] * len(soas)


def test_flags_zero_is_the_unflagged_call():
    soas = [lift(n, max(n // 30, 2), 200 + n, mix=synth.ADVERSARIAL_MIX) for n in (255, 2048, 2049, 1024)]
    db, raw, res = run(soas, flags=0)
    old = DeviceBatch(soas, fill=FILL)
    assert old.ws_bytes == db.ws_bytes
    old._call = lib().smx_compose_batch
    old.run()
    for name, a in old.raw().items():
        assert a.tobytes() == raw[name].tobytes(), name
    assert res[2] == -2 and raw["counts"][4:6].tolist() == [-2, -2]


def shared_from(base, n_shared, lens):
    """A SharedSoA: the first n_shared ops of base's branch A as the shared log, consecutive
    slices of branch B of the lengths `lens` as the own logs."""
    assert n_shared <= base.n_a and sum(lens) <= base.n_b
    keep = np.concatenate([np.arange(n_shared), base.n_a + np.arange(sum(lens))])
    off = n_shared + np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    return SharedSoA(n_shared, off, *[np.ascontiguousarray(getattr(base, c)[keep]) for c in COLS], base.n_sym, [],
                     TS_ISO, ID_UUID)


@pytest.mark.parametrize("is_b", [False, True])
def test_shared_form(is_b):
    base = lift(6200, 40, 61, mix=synth.ADVERSARIAL_MIX, divergent=0.4, rename_overlap=1.0)
    for ssoa in (shared_from(base, 2100, [0, 300, 17, 150, 299, 1, 260, 88]), shared_from(base, 100, [3000])):
        want = [oracle.compose(ssoa.merge(m, is_b)) for m in range(ssoa.n_merges)]
        assert any(len(w[4]) for w in want)
        db = DeviceBatchShared(ssoa, shared_is_b=is_b, fill=FILL, flags=LARGE)
        db.run()
        raw = db.raw()
        for m, (g, w) in enumerate(zip(db.results(raw), want)):
            assert not isinstance(g, int), f"merge {m} failed with counts {g}"
            _eq(g, w, f"shared (is_b {is_b}): merge {m}")
            o, k = db.slot(m), len(w[0])
            end = db.slot(m + 1) if m + 1 < ssoa.n_merges else db.n_out
            for name in ("order", "addr", "file", "ctx"):
                assert (raw[name][o + k: end] == FILL).all(), f"merge {m}: {name} written past its {k} ops"
        got = compose_soa_shared(ssoa, is_b, large=True)
        for m, (g, w) in enumerate(zip(got, want)):
            _eq(g, w, f"compose_soa_shared(large=True): merge {m}")
        last = session().last
        assert last["routed"] == 0 and last["large"] == ssoa.n_merges


def test_one_larger_merge():
    soa = lift(70_000, 700, 71)
    db, raw, res = run([soa])
    check_all(res, [soa], "70,000 ops")
    check_unwritten(db, raw, [soa])


def test_python_layers(edges):
    soas = [edges[1], lift(200, 10, 81), edges[6], lift(2048, 30, 82, mix=synth.ADVERSARIAL_MIX), edges[13]]
    got = compose_soa_many(soas, large=True)
    last = session().last
    assert last["routed"] == 0 and last["large"] == 3
    check_all(got, soas, "compose_soa_many(large=True)")
    for m, (g, w) in enumerate(zip(got, compose_soa_many(soas))):
        _eq(g, w, f"large=True vs large=False: merge {m}")
    got = compose_soa_many(soas, large=True, large_max=4096)   # the 6145-op merge goes through compose()
    last = session().last
    assert last["routed"] == 1 and last["large"] == 2
    check_all(got, soas, "compose_soa_many(large_max=4096)")


def test_dropins():
    from semantic_merge_amd.compose import compose_against, compose_many

    def dicts(res):
        return [(jline([o.to_dict() for o in ops]), jline([c.to_dict() for c in conf])) for ops, conf in res]

    logs = []
    for n, seed in ((3000, 91), (150, 92), (2300, 93)):
        a, b = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(n, 40, seed, mix=synth.ADVERSARIAL_MIX,
                                                                  divergent=0.3, rename_overlap=1.0)))
        logs.append((to_ops(a), to_ops(b)))
    got = compose_many(logs, large=True)
    assert session().last["routed"] == 0 and session().last["large"] == 2
    assert dicts(got) == dicts(compose_many(logs))
    assert any(conf for _, conf in got)
    shared, branches = logs[2][0] + logs[2][1][:1000], [logs[1][0], logs[1][1], logs[0][1][:400]]
    for side in ("a", "b"):
        got = compose_against(shared, branches, side, large=True)
        assert session().last["routed"] == 0 and session().last["large"] == 3
        assert dicts(got) == dicts(compose_against(shared, branches, side))
