"""GPU parity of the batched compose against one shared log (smx_compose_batch_shared,
csrc/smx_batch.h): the shared log stored once, every merge equal to the CPU oracle on that
pair alone and bit-equal to smx_compose_batch on the repeated layout; both sides, the size
classes' edges, degenerate shapes, LDS reuse, failed merges between valid ones, conflict
capacities and the drop-in compose_against."""
import copy
import dataclasses

import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import DeviceBatchShared, SmxError, compose_soa_many, compose_soa_shared

from _batch import ADV, branch, own_logs, shared_soa
from _shapes import pick
from _util import _eq_soa as _eq, jline, to_ops

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A  # what every output word holds before a run that checks the unwritten ones
MOVE = synth.KIND_RANK["moveDecl"]


_ref = {}


def ref(ssoa, m, shared_is_b=False):
    """oracle.compose(ssoa.merge(m, shared_is_b)), computed once."""
    key = (id(ssoa), m, bool(shared_is_b))
    got = _ref.get(key)
    if got is None:
        got = _ref[key] = (ssoa, oracle.compose(ssoa.merge(m, shared_is_b)))
    return got[1]


def check_all(got, ssoa, label, shared_is_b=False, skip=()):
    assert len(got) == ssoa.n_merges
    for m, g in enumerate(got):
        if m in skip:
            continue
        assert not isinstance(g, int), f"{label}: merge {m} failed with counts {g}"
        _eq(g, ref(ssoa, m, shared_is_b), f"{label}: merge {m}")


@pytest.fixture(scope="module", params=[60, 700])
def mixed40(request):
    """40 own logs of 10-200 ops against one shared log of 60 or 700 ops."""
    n_shared = request.param
    n_sym = 24
    sizes = np.random.default_rng(77 + n_shared).integers(10, 201, 40).tolist()
    ssoa = shared_soa(branch(n_shared, n_sym, 5, 0, **ADV), own_logs(n_sym, 100, sizes), n_sym)
    assert any(len(ref(ssoa, m)[4]) for m in range(40))
    return ssoa


def test_parity_with_oracle_and_repeated_layout(mixed40):
    got = compose_soa_shared(mixed40)
    check_all(got, mixed40, "shared as A")
    rep = compose_soa_many([mixed40.merge(m) for m in range(mixed40.n_merges)])
    for m, (g, r) in enumerate(zip(got, rep)):
        for name, x, y in zip(("order", "addr", "file", "ctx", "conflicts"), g, r):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"merge {m}: {name} differs from compose_soa_many"
    assert any(len(g[4]) for g in got)


def test_shared_log_as_branch_b(mixed40):
    got_a = compose_soa_shared(mixed40)
    got_b = compose_soa_shared(mixed40, shared_is_b=True)
    check_all(got_b, mixed40, "shared as B", shared_is_b=True)
    # the flag is not ignored: the pairs are (A index, B index), and the sides are swapped
    assert any(len(a[4]) and not np.array_equal(a[4], b[4]) for a, b in zip(got_a, got_b))
    db = DeviceBatchShared(mixed40, shared_is_b=True, fill=FILL)
    db.run()
    check_all(db.results(), mixed40, "shared as B (C ABI)", shared_is_b=True)


def test_class_edges():
    n_shared, n_sym = 200, 40
    totals = [c + d for c in _abi.BATCH_CLASSES for d in (-1, 0, 1)]
    assert totals == [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
    owns = [branch(t - n_shared, n_sym, 200 + t, 1, mix=synth.ADVERSARIAL_MIX) for t in totals]
    ssoa = shared_soa(branch(n_shared, n_sym, 6, 0, mix=synth.ADVERSARIAL_MIX), owns, n_sym)
    for side in (False, True):
        check_all(compose_soa_shared(ssoa, shared_is_b=side), ssoa, f"edges (routed, B={side})", side)  # 2049: compose()
        db = DeviceBatchShared(ssoa, shared_is_b=side, fill=FILL)
        db.run()
        raw = db.raw()
        res = db.results(raw)
        assert res[-1] == -2 and raw["counts"][-2:].tolist() == [-2, -2]
        check_all(res, ssoa, f"edges (C ABI, B={side})", side, skip=(8,))
        o = db.slot(8)
        assert o + 2049 == db.n_out
        for name in ("order", "addr", "file", "ctx"):
            assert (raw[name][o:] == FILL).all(), f"{name} of the merge over 2048 ops was written"
        assert (raw["conf"][2 * int(db.conf_off[8]):] == FILL).all()


def test_degenerate_shapes():
    n_sym = 12
    sh = branch(150, n_sym, 7, 0, **ADV)
    none = pick(sh, np.zeros(sh.n_a, bool), np.zeros(0, bool))
    owns = own_logs(n_sym, 300, [90, 40, 130])
    empty = pick(owns[0], np.zeros(0, bool), np.zeros(owns[0].n_b, bool))
    batches = {
        "no shared log": shared_soa(none, owns, n_sym),
        "an empty own log": shared_soa(sh, [owns[0], empty, owns[1], empty], n_sym),
        "all own logs empty": shared_soa(sh, [empty, empty, empty], n_sym),
        "nothing at all": shared_soa(none, [empty, empty], n_sym),
        "one merge": shared_soa(sh, [owns[2]], n_sym),
        "a gap before the first merge": shared_soa(sh, owns, n_sym, gap=37),
    }
    for label, ssoa in batches.items():
        for side in (False, True):
            db = DeviceBatchShared(ssoa, shared_is_b=side, fill=FILL)
            db.run()
            raw = db.raw()
            check_all(db.results(raw), ssoa, f"{label} (C ABI, B={side})", side)
            for m in range(ssoa.n_merges):
                if ssoa.off[m + 1] == ssoa.off[m]:  # the shared log composed with nothing
                    assert raw["counts"][2 * m: 2 * m + 2].tolist() == [ssoa.n_shared, 0]
                    assert np.array_equal(np.sort(db.results(raw)[m][0]), np.arange(ssoa.n_shared))
            check_all(compose_soa_shared(ssoa, shared_is_b=side), ssoa, f"{label} (session, B={side})", side)
    gap = batches["a gap before the first merge"]
    assert gap.off[0] == gap.n_shared + 37
    db = DeviceBatchShared(gap, fill=FILL)
    db.run()
    raw = db.raw()
    assert db.slot(0) == 37 and (raw["order"][:37] == FILL).all()
    assert compose_soa_shared(shared_soa(sh, [], n_sym)) == []


def test_lds_reuse_one_and_two_workgroups(mixed40):
    raws = {}
    for cap in (0, 1, 2):
        db = DeviceBatchShared(mixed40, grid_cap=cap, fill=FILL)
        db.run()
        raws[cap] = db.raw()
        check_all(db.results(raws[cap]), mixed40, f"grid_cap {cap}")
    for cap in (1, 2):
        for name, a in raws[0].items():
            assert a.tobytes() == raws[cap][name].tobytes(), f"grid_cap {cap}: {name} differs from grid_cap 0"


def check_untouched(db, raw, failed, label):
    """Failed merges report -1 and leave their slots as they were; the others are correct and
    write nothing past their counts."""
    res = db.results(raw)
    ssoa = db.ssoa
    for m in range(db.n_merges):
        o, c = db.slot(m), int(db.conf_off[m])
        cap = int(db.conf_off[m + 1]) - c
        room = max(ssoa.n_shared + int(db.off[m + 1]) - int(db.off[m]), 0)  # n_shared + len_m entries
        if m in failed:
            assert raw["counts"][2 * m: 2 * m + 2].tolist() == [-1, -1], f"{label}: merge {m}"
            k = nc = 0
        else:
            _eq(res[m], ref(ssoa, m), f"{label}: valid merge {m}")
            k, nc = (int(x) for x in raw["counts"][2 * m: 2 * m + 2])
        for name in ("order", "addr", "file", "ctx"):
            assert (raw[name][o + k: o + room] == FILL).all(), f"{label}: merge {m}: {name} written past its {k} ops"
        assert (raw["conf"][2 * (c + nc): 2 * (c + cap)] == FILL).all(), f"{label}: merge {m}: conflicts past its {nc}"
    assert (raw["conf"][2 * int(db.conf_off[-1]):] == FILL).all()


def test_failed_merges_do_not_touch_their_neighbours():
    n_sym = 8
    sh = branch(120, n_sym, 8, 0, **ADV)
    owns = own_logs(n_sym, 400, [100, 60, 300, 150, 1000, 80])
    owns[3].sym[70] = n_sym  # an own op with sym = n_sym
    good = shared_soa(sh, owns, n_sym)
    caps = [min(o.n, sh.n) for o in owns]
    # merge 1's offsets decrease: it ends 5 ops before it starts, and merge 2 starts there, on
    # the last 5 ops of merge 0's log (a valid merge of its own: 5 + 60 + 300 own ops)
    off = good.off.copy()
    off[2] = off[1] - 5
    caps[1] = 0
    ssoa = dataclasses.replace(good, off=off)
    db = DeviceBatchShared(ssoa, conflict_caps=caps, fill=FILL)
    db.run()
    check_untouched(db, db.raw(), (1, 3), "decreasing offsets, a bad symbol")
    # the first merge starts inside the shared log
    off = good.off.copy()
    off[0] -= 1
    db = DeviceBatchShared(good, off=off, fill=FILL)
    db.run()
    raw = db.raw()
    assert raw["counts"][:2].tolist() == [-1, -1]
    db.off = good.off  # (its slot, and those of the merges after it, are where they were)
    check_untouched(db, raw, (0, 3), "off[0] < n_shared")
    # the last merge ends past n_total
    db = DeviceBatchShared(good, fill=FILL, n_total=good.n_total - 1)
    db.run()
    check_untouched(db, db.raw(), (3, 5), "off[M] > n_total")
    with pytest.raises(SmxError, match="merge 3"):
        compose_soa_shared(good)
    # an invalid op in the shared log: every merge reports -1 and nothing else is written
    valid = own_logs(n_sym, 500, [100, 60, 300])
    for col, at, value in (("kind", 119, 18), ("sym", 0, n_sym)):
        bad = shared_soa(sh, valid, n_sym)
        getattr(bad, col)[at] = value
        for side in (False, True):
            db = DeviceBatchShared(bad, shared_is_b=side, fill=FILL)
            db.run()
            raw = db.raw()
            assert (raw["counts"][: 2 * 3] == -1).all(), f"{col}, B={side}"
            for name in ("order", "addr", "file", "ctx", "conf"):
                assert (raw[name] == FILL).all(), f"{col}, B={side}: {name} was written"
    with pytest.raises(SmxError, match="shared log"):
        compose_soa_shared(bad)


@pytest.mark.parametrize("cap", [0, 1])
def test_conflict_capacity(cap):
    n_sym = 6
    sh = branch(150, n_sym, 9, 0, **ADV)
    owns = [branch(n, n_sym, 51 + n, 1, **ADV) for n in (120, 60)]
    ssoa = shared_soa(sh, owns, n_sym)
    full = ref(ssoa, 0)
    assert len(full[4]) > 1 and len(ref(ssoa, 1)[4]) > 0
    db = DeviceBatchShared(ssoa, conflict_caps=[cap, 60], fill=FILL)
    db.run()
    raw = db.raw()
    res = db.results(raw)
    assert raw["counts"][:2].tolist() == [len(full[0]), len(full[4])]  # the full count, the ops complete
    _eq(res[0][:4], full[:4], "composed ops of the truncated merge")
    assert np.array_equal(res[0][4], full[4][:cap])
    _eq(res[1], ref(ssoa, 1), "the merge after it")
    nc = len(ref(ssoa, 1)[4])
    assert (raw["conf"][2 * (cap + nc):] == FILL).all()


def test_dropin_compose_against():
    from semantic_merge_amd import compose_against
    from semantic_merge_amd.compose import compose_oplogs

    def logs(n, seed):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 30, seed, **ADV)))

    shared = to_ops(logs(300, 1)[0])
    branches = [to_ops(logs(n, 10 + n)[1]) for n in (40, 150, 1900, 90)]  # 300 + 1900 ops: over 2048
    branches.insert(2, [])
    assert compose_against(shared, []) == []
    for side in ("a", "b"):
        before = copy.deepcopy((shared, branches))
        ids = [id(o) for o in shared] + [id(o) for b in branches for o in b]
        got = compose_against(shared, branches, shared_side=side)
        want = [compose_oplogs(shared, b) if side == "a" else compose_oplogs(b, shared) for b in branches]
        assert len(got) == len(want)
        for i, ((go, gc), (wo, wc)) in enumerate(zip(got, want)):
            assert jline([o.to_dict() for o in go]) == jline([o.to_dict() for o in wo]), f"{side}, branch {i}: ops"
            assert jline([c.to_dict() for c in gc]) == jline([c.to_dict() for c in wc]), f"{side}, branch {i}: conflicts"
        assert any(gc for _, gc in got)
        assert (shared, branches) == before
        assert ids == [id(o) for o in shared] + [id(o) for b in branches for o in b]
    with pytest.raises(ValueError):
        compose_against(shared, branches, shared_side="c")
