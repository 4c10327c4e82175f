"""GPU parity of the batched compose (smx_compose_batch, csrc/smx_batch.h): many independent
merges of at most 2048 ops in one call, each equal to the CPU oracle on that merge alone
(and to the golden JSON where there is one); the size classes' edges, LDS reuse when one
workgroup runs merge after merge, empty merges, failed merges between valid ones, conflict
capacities, None-valued moves and the drop-in compose_many."""
import copy

import numpy as np
import pytest

from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import DeviceBatch, SmxError, compose_soa, compose_soa_many
from semantic_merge_amd.marshal import marshal
from semantic_merge_amd.materialize import materialize_conflicts, materialize_ops

from _batch import check_all, lift, none_moves, ref
from _shapes import SPECS, pick
from _util import _eq_soa as _eq, jline, load, to_ops

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A  # what every output word holds before a run that checks the unwritten ones
MOVE = synth.KIND_RANK["moveDecl"]


@pytest.fixture(scope="module")
def mixed40():
    """40 merges of 30-250 ops: conflicts, None-valued moves, shuffled logs, dense ties."""
    rng = np.random.default_rng(77)
    out = []
    for i, n in enumerate(rng.integers(30, 251, 40).tolist()):
        kw = [dict(mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0), dict(ops_per_ms=3),
              dict(shuffle=True, mix=synth.ADVERSARIAL_MIX), dict(ops_per_ms=4096, mix=synth.ADVERSARIAL_MIX),
              dict()][i % 5]
        soa = lift(n, max(n // (4 + i % 7), 1), 100 + i, **kw)
        out.append(none_moves(soa, i) if i % 5 == 1 else soa)
    assert any(len(ref(s)[4]) for s in out)
    return out


def test_golden_in_one_batch():
    cases = list(load("compose_scenarios.json").items()) + [(f"case {i}", c) for i, c in
                                                            enumerate(load("compose_cases.json"))]
    ops = [(to_ops(c["A"]), to_ops(c["B"])) for _, c in cases]
    soas = [marshal(a, b) for a, b in ops]
    assert all(s.n <= _abi.BATCH_MAX_OPS for s in soas)
    got = compose_soa_many(soas)
    for (name, case), (a, b), soa, (order, addr, file, ctx, pairs) in zip(cases, ops, soas, got):
        out = materialize_ops(a + b, soa.kind, soa.strings, order, addr, file, ctx)
        conf = materialize_conflicts(a + b, np.asarray(pairs).reshape(-1, 2))
        assert jline([o.to_dict() for o in out]) == jline(case["out"]), f"{name}: composed ops differ"
        assert jline([c.to_dict() for c in conf]) == jline(case["conflicts"]), f"{name}: conflicts differ"


def test_small_plan_shapes_in_one_batch():
    soas = [synth.lift_soa(synth.lift_logs(SPECS[i])) for i in (6, 0, 3, 8, 1, 5, 2, 7, 4)]
    got = compose_soa_many(soas)
    check_all(got, soas, "specs")
    for m, s in enumerate(soas):
        _eq(got[m], compose_soa(s), f"specs vs compose_soa: merge {m}")


def test_class_edges():
    sizes = [c + d for c in _abi.BATCH_CLASSES for d in (-1, 0, 1)]
    assert sizes[-1] == _abi.BATCH_MAX_OPS + 1
    soas = [lift(n, max(n // 30, 2), 200 + n, mix=synth.ADVERSARIAL_MIX) for n in sizes]
    check_all(compose_soa_many(soas), soas, "edges (routed)")  # 2049 ops: through compose()
    db = DeviceBatch(soas, fill=FILL)
    db.run()
    raw = db.raw()
    res = db.results(raw)
    assert res[-1] == -2 and raw["counts"][-1] == -2
    check_all(res[:-1], soas[:-1], "edges (C ABI)")
    o = int(db.off[-2])
    for name in ("order", "addr", "file", "ctx"):
        assert (raw[name][o:] == FILL).all(), f"{name} of the merge over 2048 ops was written"
    assert (raw["conf"][2 * int(db.conf_off[-2]):] == FILL).all()


def test_lds_reuse_one_and_two_workgroups(mixed40):
    raws = {}
    for cap in (0, 1, 2):
        db = DeviceBatch(mixed40, grid_cap=cap, fill=FILL)
        db.run()
        raws[cap] = db.raw()
        check_all(db.results(raws[cap]), mixed40, f"grid_cap {cap}")
    for cap in (1, 2):
        for name, a in raws[0].items():
            assert np.array_equal(a, raws[cap][name]), f"grid_cap {cap}: {name} differs from grid_cap 0"


def test_empty_merges():
    base = lift(180, 9, 31, mix=synth.ADVERSARIAL_MIX)
    za, zb = np.zeros(base.n_a, bool), np.zeros(base.n_b, bool)
    empty, a_only, b_only = pick(base, za, zb), pick(base, ~za, zb), pick(base, za, ~zb)
    v1, v2 = lift(200, 10, 32, mix=synth.ADVERSARIAL_MIX, divergent=0.5), lift(90, 5, 33, shuffle=True)
    for order in ((empty, v1, a_only, v2, b_only), (a_only, v1, b_only, v2, empty), (b_only, v1, empty, v2, a_only)):
        soas = list(order)
        db = DeviceBatch(soas, fill=FILL)
        db.run()
        raw = db.raw()
        check_all(db.results(raw), soas, "empty merges")
        for m, s in enumerate(soas):
            if s is not v1 and s is not v2:
                assert raw["counts"][2 * m: 2 * m + 2].tolist() == [s.n, 0]
        check_all(compose_soa_many(soas), soas, "empty merges (session)")
    check_all(compose_soa_many([empty]), [empty], "one empty merge")


def test_failed_merges_do_not_touch_their_neighbours():
    valid = [lift(n, 8, 300 + n, mix=synth.ADVERSARIAL_MIX, divergent=0.3) for n in (120, 300, 77, 1100, 250)]
    bad_sym, bad_kind, bad_na, past_end = (lift(n, 8, 400 + n) for n in (150, 600, 90, 40))
    bad_sym.sym[70] = 8            # = n_sym
    bad_kind.kind[599] = 18
    soas = [valid[0], bad_sym, valid[1], bad_kind, valid[2], bad_na, valid[3], valid[4], past_end]
    n_a = [s.n_a for s in soas]
    n_a[5] = bad_na.n + 1
    total = sum(s.n for s in soas)
    db = DeviceBatch(soas, n_a=n_a, n_sym=8, fill=FILL, n_total=total - 1)  # the last merge ends past n_total
    db.run()
    raw = db.raw()
    res = db.results(raw)
    for m, s in enumerate(soas):
        o, c = int(db.off[m]), int(db.conf_off[m])
        cap = int(db.conf_off[m + 1]) - c
        if m in (1, 3, 5, 8):
            assert raw["counts"][2 * m: 2 * m + 2].tolist() == [-1, -1], f"merge {m}"
            k = nc = 0
        else:
            _eq(res[m], ref(s), f"valid merge {m}")
            k, nc = (int(x) for x in raw["counts"][2 * m: 2 * m + 2])
        for name in ("order", "addr", "file", "ctx"):
            assert (raw[name][o + k: o + s.n] == FILL).all(), f"merge {m}: {name} written past its {k} ops"
        assert (raw["conf"][2 * (c + nc): 2 * (c + cap)] == FILL).all(), f"merge {m}: conflicts past its {nc} pairs"
    assert (raw["conf"][2 * int(db.conf_off[-1]):] == FILL).all()
    with pytest.raises(SmxError, match="merge 3"):
        compose_soa_many([valid[0], valid[1], valid[2], bad_kind])


@pytest.mark.parametrize("cap", [0, 1])
def test_conflict_capacity(cap):
    many = lift(240, 6, 51, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    after = lift(130, 6, 52, mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    full = ref(many)
    assert len(full[4]) > 1 and len(ref(after)[4]) > 0
    db = DeviceBatch([many, after], conflict_caps=[cap, min(after.n_a, after.n_b)], fill=FILL)
    db.run()
    raw = db.raw()
    res = db.results(raw)
    assert raw["counts"][:2].tolist() == [len(full[0]), len(full[4])]  # the full count, the ops complete
    _eq(res[0][:4], full[:4], "composed ops of the truncated merge")
    assert np.array_equal(res[0][4], full[4][:cap])
    _eq(res[1], ref(after), "the merge after it")
    nc = len(ref(after)[4])
    assert (raw["conf"][2 * (cap + nc):] == FILL).all()


def test_none_valued_moves_in_a_batch():
    mixed = none_moves(lift(256, 8, 21, ops_per_ms=3), 5)
    one_symbol = none_moves(lift(256, 1, 21, ops_per_ms=3), 5)
    assert ((mixed.v0 < 0) & (mixed.kind == MOVE)).any() and ((one_symbol.v1 < 0) & (one_symbol.kind == MOVE)).any()
    plain = lift(200, 10, 22)
    soas = [plain, mixed, plain, one_symbol, mixed]
    check_all(compose_soa_many(soas), soas, "None-valued moves")


def test_dropin_compose_many():
    from semantic_merge_amd.compose import compose_many, compose_oplogs
    assert compose_many([]) == []
    pairs = [(to_ops(c["A"]), to_ops(c["B"])) for c in load("compose_cases.json")[:50]]
    a, b = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(3000, 60, 61, mix=synth.ADVERSARIAL_MIX)))
    pairs.insert(20, (to_ops(a), to_ops(b)))  # over 2048 ops: routed through compose_oplogs
    before = [(list(x), list(y), jline([o.to_dict() for o in x + y])) for x, y in pairs]
    got = compose_many(pairs)
    want = [compose_oplogs(x, y) for x, y in pairs]
    assert len(got) == len(want)
    for i, ((go, gc), (wo, wc)) in enumerate(zip(got, want)):
        assert jline([o.to_dict() for o in go]) == jline([o.to_dict() for o in wo]), f"pair {i}: composed ops"
        assert jline([c.to_dict() for c in gc]) == jline([c.to_dict() for c in wc]), f"pair {i}: conflicts"
    for (x, y), (x0, y0, j0) in zip(pairs, before):
        assert len(x) == len(x0) and all(p is q for p, q in zip(x, x0))
        assert len(y) == len(y0) and all(p is q for p, q in zip(y, y0))
        assert jline([o.to_dict() for o in x + y]) == j0
    assert any(gc for _, gc in got)


def test_two_calls_identical_bytes(mixed40):
    raws = []
    for _ in range(2):
        db = DeviceBatch(mixed40 + [lift(1500, 40, 71, mix=synth.ADVERSARIAL_MIX)], fill=FILL)
        db.run()
        raws.append(db.raw())
    for name, a in raws[0].items():
        assert a.tobytes() == raws[1][name].tobytes(), name
    a = compose_soa_many(mixed40)
    b = compose_soa_many(copy.copy(mixed40))
    for x, y in zip(a, b):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
