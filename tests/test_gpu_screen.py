"""GPU parity of the conflict screen (smx_screen, csrc/smx_screen.h): for every pair the
conflicts of the CPU oracle on that pair alone, in order, with A||B indices; the limit on
renames (not ops), the size classes' edges, degenerate shapes, LDS reuse, unordered logs, failed
pairs between valid ones, conflict capacities and the drop-in screen_conflicts."""
import copy

import numpy as np
import pytest

from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import DeviceBatch, SmxError, screen_soa

from _batch import ADV, branch, own_logs
from _screen import (FILL, RENAME, check_all, check_unwritten, empty_log, logs_soa, make_log, ref,
                     renames_ordered, run, with_renames)
from _util import jline, to_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twelve():
    """12 logs of 10-400 ops (test_gpu_shared's own_logs recipe), every ordered pair and (l, l)."""
    n_sym = 24
    sizes = np.random.default_rng(5).integers(10, 401, 12).tolist()
    lsoa = logs_soa(own_logs(n_sym, 700, sizes), n_sym)
    pairs = [(i, j) for i in range(12) for j in range(12)]
    return lsoa, pairs


def test_all_pairs(twelve):
    lsoa, pairs = twelve
    got = screen_soa(lsoa, pairs)
    check_all(got, lsoa, pairs, "session")
    ds, raw, res = run(lsoa, pairs)
    check_all(res, lsoa, pairs, "C ABI")
    check_unwritten(ds, raw, "C ABI")
    assert [int(c) for c in raw["counts"]] == [len(ref(lsoa, i, j)) for i, j in pairs]
    assert any(len(g) for g in got)
    assert any(len(ref(lsoa, i, i)) for i in range(12))    # (l, l) is an ordinary pair
    assert any(len(ref(lsoa, i, j)) and not np.array_equal(ref(lsoa, i, j), ref(lsoa, j, i))
               for i, j in pairs if i != j)    # the sides are not interchangeable


def test_limit_is_on_renames_not_ops():
    n_sym = 30
    logs = []
    for side in (0, 1):
        soa = with_renames(branch(20000, n_sym, 40 + side, side, **ADV), 300, others=5700)
        assert soa.n == 6000
        logs.append(soa)
    lsoa = logs_soa(logs, n_sym)
    ds, raw, res = run(lsoa, [(0, 1), (1, 0)])
    check_all(res, lsoa, [(0, 1), (1, 0)], "6000-op logs")
    assert len(res[0]) > 0
    db = DeviceBatch([lsoa.pair(0, 1)])
    db.run()
    assert db.results()[0] == -2    # the batched compose refuses the pair for its length


def test_class_and_limit_edges():
    n_sym = 40
    totals = [c + d for c in _abi.SCREEN_CLASSES for d in (-1, 0, 1)]
    assert totals == [127, 128, 129, 511, 512, 513, 2047, 2048, 2049]
    base = [branch(6000, n_sym, 60 + s, s, **ADV) for s in (0, 1)]   # ~3600 renames each
    logs, pairs = [], []
    for t in totals:
        ra = t // 3
        logs += [with_renames(base[0], ra, others=ra // 4), with_renames(base[1], t - ra, others=50)]
        pairs.append((len(logs) - 2, len(logs) - 1))
    x, e, y = len(logs), len(logs) + 1, len(logs) + 2
    logs += [with_renames(base[1], 2048, others=100), empty_log(n_sym), with_renames(base[0], 2049, others=10)]
    pairs += [(x, e), (e, x), (x, 0), (y, e), (e, y), (y, y), (0, y)]
    lsoa = logs_soa(logs, n_sym)
    over = {8, 11, 12, 13, 14, 15}   # total 2049; 2048 + 42 renames; every pair that holds y
    ds, raw, res = run(lsoa, pairs)
    for p in range(len(pairs)):
        assert (int(raw["counts"][p]) == -2) == (p in over), f"pair {p} {pairs[p]}: counts {raw['counts'][p]}"
    check_all(res, lsoa, pairs, "edges (C ABI)", skip=over)
    check_unwritten(ds, raw, "edges")     # (a -2 pair: its whole region is as it was)
    assert len(res[7]) > 0 and len(res[9]) == 0 and int(raw["counts"][9]) == 0   # 2048 renames against none
    check_all(screen_soa(lsoa, pairs), lsoa, pairs, "edges (session, the -2 pairs routed)")


def test_degenerate_shapes():
    n_sym = 12
    owns = own_logs(n_sym, 300, [90, 40, 130])
    noren = with_renames(owns[0], 0)
    gap = make_log([0xFF] * 37, [0] * 37, [0] * 37, [0] * 37, [0xFFFFFFFF] * 37, [-1] * 37, n_sym)
    cases = {
        "a log without renames": ([owns[0], noren, owns[1]], [(0, 1), (1, 0), (1, 1), (0, 2), (1, 2)]),
        "an empty log": ([owns[0], empty_log(n_sym), owns[1]], [(0, 1), (1, 0), (1, 1), (0, 2)]),
        "all logs empty": ([empty_log(n_sym)] * 3, [(0, 1), (2, 2)]),
        "one pair": ([owns[1], owns[2]], [(1, 0)]),
        "a gap no pair covers": ([owns[0], gap, owns[2]], [(0, 2), (2, 0), (2, 2)]),
    }
    for label, (logs, pairs) in cases.items():
        lsoa = logs_soa(logs, n_sym)
        ds, raw, res = run(lsoa, pairs)
        check_all(res, lsoa, pairs, f"{label} (C ABI)")
        check_unwritten(ds, raw, label)
        check_all(screen_soa(lsoa, pairs), lsoa, pairs, f"{label} (session)")
    lsoa = logs_soa([owns[0], gap, owns[2]], n_sym)
    assert run(lsoa, [(0, 1), (0, 2)])[2][0] == -1     # (the gap, were it a log, is invalid)
    assert screen_soa(lsoa, []) == []


def test_lds_reuse_one_and_two_workgroups(twelve):
    lsoa, pairs = twelve
    raws = {}
    for cap in (0, 1, 2):
        ds, raws[cap], res = run(lsoa, pairs, grid_cap=cap)
        check_all(res, lsoa, pairs, f"grid_cap {cap}")
    for cap in (1, 2):
        for name, a in raws[0].items():
            assert a.tobytes() == raws[cap][name].tobytes(), f"grid_cap {cap}: {name} differs from grid_cap 0"


def test_conflict_runs_and_full_key_ties():
    n = 150
    rng = np.random.default_rng(3)
    ts = 1000 + np.arange(n) // 7
    hi, lo = rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n)
    # one symbol, every name different: each pair of heads conflicts, a run of n conflicts
    a = make_log([RENAME] * n, ts, hi, lo, [2] * n, np.arange(n))
    b = make_log([RENAME] * n, ts + 3, hi[::-1], lo, [2] * n, 1000 + np.arange(n))
    # b's keys are a's: full-key ties between A and B, A goes first
    tie = make_log([RENAME] * n, ts, hi, lo, rng.integers(0, 3, n), 2000 + rng.integers(0, 4, n))
    lsoa = logs_soa([a, b, tie], 4)
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (2, 2), (1, 2)]
    assert len(ref(lsoa, 0, 1)) == n and len(ref(lsoa, 0, 2)) > 0
    assert not np.array_equal(ref(lsoa, 0, 2)[:, 0], ref(lsoa, 2, 0)[:, 1] - n)
    ds, raw, res = run(lsoa, pairs)
    check_all(res, lsoa, pairs, "runs and ties")
    check_unwritten(ds, raw, "runs and ties")


def test_unordered_logs():
    n_sym = 16
    logs = [branch(500, n_sym, 80, 0, **ADV, shuffle=True),                  # shuffled
            branch(400, n_sym, 81, 1, **ADV, ops_per_ms=4096),              # ordered ts, ids unordered in ties
            branch(300, n_sym, 82, 0, **ADV, ops_per_ms=1),                 # ordered: no sort
            branch(350, n_sym, 83, 1, **ADV, shuffle=True, ops_per_ms=4096)]
    # both paths of the per-log kernel run: the bitonic sort and the already-ordered skip
    assert [renames_ordered(x) for x in logs] == [False, False, True, False]
    lsoa = logs_soa(logs, n_sym)
    pairs = [(i, j) for i in range(4) for j in range(4)]
    ds, raw, res = run(lsoa, pairs)
    check_all(res, lsoa, pairs, "unordered logs")
    assert all(len(ref(lsoa, i, j)) for i, j in pairs if i != j)


def test_failed_pairs_do_not_touch_their_neighbours():
    n_sym = 8
    owns = own_logs(n_sym, 400, [100, 60, 300, 150, 80])
    # sym has no bound here: log 2's renames are all of symbol 0xFFFFFFFF (the oracle, whose
    # tables are indexed by symbol, composes the same logs with that symbol called n_sym)
    owns[2].sym[owns[2].kind == RENAME] = n_sym
    oref = logs_soa(owns, n_sym + 1)
    good = copy.deepcopy(oref)
    good.sym[good.sym == n_sym] = 0xFFFFFFFF
    L = 5
    pairs = [(i, j) for i in range(L) for j in range(L)] + [(-1, 0), (0, L), (L, L), (1, -1)]

    def check(ds, raw, res, bad_logs, label):
        for p, (i, j) in enumerate(pairs):
            failing = not (0 <= i < L and 0 <= j < L) or i in bad_logs or j in bad_logs
            if failing:
                assert int(raw["counts"][p]) == -1, f"{label}: pair {p} ({i}, {j}): counts {raw['counts'][p]}"
            else:
                assert not isinstance(res[p], int), f"{label}: pair {p} ({i}, {j}) failed: {res[p]}"
                assert np.array_equal(res[p], ref(oref, i, j)), f"{label}: valid pair {p} ({i}, {j})"
        check_unwritten(ds, raw, label)

    ds, raw, res = run(good, pairs)
    check(ds, raw, res, (), "pair indices outside the logs")
    assert len(ref(oref, 2, 2)) > 0 and (good.sym == 0xFFFFFFFF).sum() > 100
    # log 1 ends 5 ops before it starts; log 2 then starts before log 1's offset: both fail
    off = good.log_off.copy()
    off[2] = off[1] - 5
    ds, raw, res = run(good, pairs, log_off=off)
    check(ds, raw, res, (1, 2), "decreasing offsets")
    # the last log ends past n_total
    ds, raw, res = run(good, pairs, n_total=good.n_total - 1)
    check(ds, raw, res, (4,), "the last offset past n_total")
    # kind 18 in an op of log 3 that is no rename
    bad = copy.deepcopy(good)
    at = int(good.log_off[3]) + int(np.flatnonzero(owns[3].kind != RENAME)[-1])
    bad.kind[at] = 18
    ds, raw, res = run(bad, pairs)
    check(ds, raw, res, (3,), "kind 18")
    with pytest.raises(SmxError, match="pair 3 "):
        screen_soa(bad, [(i, j) for i in range(L) for j in range(L)])
    with pytest.raises(SmxError, match="pair 1"):
        screen_soa(good, [(0, 1), (0, L)])


@pytest.mark.parametrize("cap", [0, 1, "null"])
def test_conflict_capacity(cap):
    n_sym = 6
    lsoa = logs_soa([branch(150, n_sym, 9, 0, **ADV), branch(120, n_sym, 171, 1, **ADV), branch(60, n_sym, 111, 1, **ADV)],
                    n_sym)
    pairs = [(0, 1), (0, 2)]
    full = [ref(lsoa, 0, 1), ref(lsoa, 0, 2)]
    assert len(full[0]) > 1 and len(full[1]) > 0
    ds, raw, res = run(lsoa, pairs, conflict_caps="null" if cap == "null" else [cap, 60])
    assert raw["counts"][:2].tolist() == [len(full[0]), len(full[1])]   # the full counts
    if cap == "null":
        assert (raw["conf"] == FILL).all()
        return
    assert np.array_equal(res[0], full[0][:cap])
    assert np.array_equal(res[1], full[1])
    assert (raw["conf"][2 * (cap + len(full[1])):] == FILL).all()


def test_dropin_screen_conflicts():
    from semantic_merge_amd import screen_conflicts
    from semantic_merge_amd.compose import compose_oplogs

    def logs(n, seed):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 30, seed, **ADV)))

    ops = [to_ops(logs(300, 1)[0])] + [to_ops(logs(n, 10 + n)[1]) for n in (40, 150, 90)] + [[]]
    ops.append(to_ops(logs(3600, 7)[0]))      # ~2160 renames: every pair that holds it is routed
    assert sum(o.type == "renameSymbol" for o in ops[5]) > _abi.SCREEN_MAX_RENAMES
    explicit = [(1, 0), (0, 0), (5, 2), (2, 5), (4, 3), (3, 1)]
    assert screen_conflicts(ops, []) == [] and screen_conflicts([], None) == []
    for pairs in (None, explicit):
        before = copy.deepcopy(ops)
        ids = [id(o) for log in ops for o in log]
        got = screen_conflicts(ops[:5] if pairs is None else ops, pairs)
        todo = [(i, j) for i in range(5) for j in range(i + 1, 5)] if pairs is None else pairs
        assert len(got) == len(todo)
        for (i, j), gc in zip(todo, got):
            wc = compose_oplogs(ops[i], ops[j])[1]
            assert jline([c.to_dict() for c in gc]) == jline([c.to_dict() for c in wc]), f"pair ({i}, {j})"
        assert any(got)
        assert ops == before
        assert ids == [id(o) for log in ops for o in log]
    with pytest.raises(IndexError):
        screen_conflicts(ops, [(0, 6)])
