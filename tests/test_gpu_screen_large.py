"""GPU parity of the screen's large mode (smx_screen_ex with SMX_SCREEN_LARGE,
csrc/smx_screen.h k_screen_extract_large and k_screen_stream): for every pair, whatever its
number of renames, the conflicts of the CPU oracle on that pair alone, in order; the edges of
the 2048-rename limit with and without the flag, the large logs' sort, the walk across rounds,
truncation, one workgroup for everything, and the session and drop-in keyword."""
import copy

import numpy as np
import pytest

from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import ComposeSession, screen_soa

import _cand
from _batch import ADV, branch
from _screen import (FILL, RENAME, check_all, check_unwritten, empty_log, logs_soa, make_log, ref, renames_ordered,
                     run, with_renames)
from _util import jline, to_ops

pytestmark = pytest.mark.gpu

N_SYM = 40
_base = {}


def base(side, shuffle=False):
    """A branch log of 7200 ops, about 4300 of them renames, computed once."""
    key = (side, shuffle)
    if key not in _base:
        _base[key] = branch(7200, N_SYM, 60 + side + 10 * shuffle, side, **ADV, shuffle=shuffle)
    return _base[key]


def renames(ts, hi, lo, sym, v0, extra=0):
    """A log of renames given by column, and `extra` ops of kind 0 after them."""
    n = len(ts)
    pad = [0] * extra
    return make_log([RENAME] * n + pad, list(ts) + pad, list(hi) + pad, list(lo) + pad, list(sym) + pad,
                    list(v0) + pad, N_SYM)


def test_edges_of_the_limit():
    a, b = base(0), base(1)
    logs = [with_renames(a, 1024, others=300), with_renames(b, 1025, others=40),     # 0, 1
            with_renames(a, 2048, others=100), with_renames(b, 1, others=5),         # 2, 3
            with_renames(a, 2049, others=10), empty_log(N_SYM),                      # 4, 5
            with_renames(b, 60, others=20),                                          # 6
            with_renames(a, 42, others=10), with_renames(b, 85, others=20),          # 7, 8: 127 together
            with_renames(a, 171, others=40), with_renames(b, 342, others=90)]        # 9, 10: 513 together
    pairs = [(0, 1), (2, 3), (3, 2), (4, 5), (5, 4), (4, 4), (4, 6), (6, 4), (7, 8), (9, 10)]
    over = {0, 1, 2, 3, 4, 5, 6, 7}     # without the flag: 2049 together, or log 4 (2049 renames) on a side
    lsoa = logs_soa(logs, N_SYM)
    ds, raw, res = run(lsoa, pairs, large=True)
    check_all(res, lsoa, pairs, "edges, large")
    check_unwritten(ds, raw, "edges, large")
    assert [int(c) for c in raw["counts"]] == [len(ref(lsoa, i, j)) for i, j in pairs]
    assert int(raw["counts"][3]) == 0 and int(raw["counts"][4]) == 0      # 2049 renames against none
    assert all(len(res[p]) > 0 for p in (0, 5, 6, 7, 8, 9))
    # the same columns without the flag: -2 exactly there, those regions as they were
    ds, raw, res = run(lsoa, pairs)
    for p in range(len(pairs)):
        assert (int(raw["counts"][p]) == -2) == (p in over), f"pair {p} {pairs[p]}: counts {raw['counts'][p]}"
    check_all(res, lsoa, pairs, "edges, flags 0", skip=over)
    check_unwritten(ds, raw, "edges, flags 0")


def tied_log(n, seed):
    """n renames whose keys come in runs of three equal (ts, id) keys -- index order decides --
    and pairs of runs that differ in oid_lo only, in shuffled order (so that equal keys lie
    tiles apart)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    ts = 1000 + i // 12
    hi = rng.integers(0, 1 << 62, n // 6 + 1)[i // 6]
    lo = rng.integers(0, 1 << 62, n // 3 + 1)[i // 3]
    p = rng.permutation(n)
    return renames(ts[p], hi[p], lo[p], rng.integers(0, 6, n), rng.integers(0, 5, n), extra=7)


def test_large_extract():
    sh0, sh1 = base(0, shuffle=True), base(1, shuffle=True)
    ordered = with_renames(branch(4000, N_SYM, 82, 0, **ADV, ops_per_ms=1), 2100, others=200)
    logs = [with_renames(sh0, 2049, others=500),       # 0: shuffled, one merge level
            with_renames(sh1, 4097, others=900),       # 1: shuffled, two merge levels
            tied_log(2600, 1),                         # 2: equal keys, keys that differ in oid_lo only
            ordered,                                   # 3: in order already, the sort is skipped
            with_renames(base(1), 60, others=20),      # 4: a small partner
            tied_log(300, 2)]                          # 5: tied keys on both sides ((2, 2): every key ties with itself)
    assert [renames_ordered(x) for x in logs[:4]] == [False, False, False, True]
    lsoa = logs_soa(logs, N_SYM)
    pairs = [(l, 4) for l in range(4)] + [(4, l) for l in range(4)] + [(0, 1), (1, 0), (1, 1), (2, 5), (5, 2), (2, 2),
                                                                     (3, 0), (3, 1), (1, 3), (3, 3)]
    ds, raw, res = run(lsoa, pairs, large=True)
    check_all(res, lsoa, pairs, "large extract")
    check_unwritten(ds, raw, "large extract")
    assert all(len(r) >= 50 for r in res[8:])     # (the pairs of two large logs: many conflicts to get wrong)


def test_kind_18_past_the_2048th_rename():
    good = with_renames(base(0), 2100, others=300)
    lsoa = logs_soa([good, with_renames(base(1), 60, others=20), good], N_SYM)
    bad = copy.deepcopy(lsoa)
    k = np.asarray(bad.kind[: good.n])
    at = int(np.flatnonzero(np.cumsum(k == RENAME) >= 2049)[5])    # a few ops past the 2049th rename
    bad.kind[at] = 18
    pairs = [(0, 1), (1, 0), (0, 0), (0, 2), (2, 1), (1, 1)]
    ds, raw, res = run(bad, pairs, large=True)
    assert [int(c) for c in raw["counts"][:4]] == [-1] * 4
    check_unwritten(ds, raw, "kind 18")
    for p in (4, 5):    # its neighbours are served
        assert np.array_equal(res[p], ref(lsoa, *pairs[p])), f"pair {p}"


def test_walk_across_rounds():
    rng = np.random.default_rng(11)

    def keys(n, lo_ts, hi_ts):
        return np.sort(rng.integers(lo_ts, hi_ts, n)), rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n)

    # 0, 1: one symbol, every name different: 3000 conflicts, 1024 per round
    hot = [renames(*keys(3000, 1000, 4000), [2] * 3000, s * 5000 + np.arange(3000)) for s in (0, 1)]
    # 2, 3: every key of 2 below every key of 3: one head stays while the other side streams past
    low = renames(*keys(2500, 1000, 9000), rng.integers(0, N_SYM, 2500), rng.integers(0, 4, 2500))
    high = renames(*keys(1500, 10000, 19000), rng.integers(0, N_SYM, 1500), rng.integers(0, 4, 1500))
    # 4, 5: round one uses up B's 1024 with A's head on its 1024th rename; that rename conflicts
    # with B's 1025th, the first record of B's next chunk
    na = nb = 1100
    ta = np.concatenate([np.arange(1023), [5000], 6000 + 2 * np.arange(na - 1024)])
    tb = np.concatenate([2000 + np.arange(1024), [5001], 6001 + 2 * np.arange(nb - 1025)])
    ea = renames(ta, np.arange(na), np.arange(na), [1] * 1023 + [7] + [3] * (na - 1024), np.arange(na))
    eb = renames(tb, np.arange(nb), np.arange(nb), [2] * 1024 + [7] + [3] * (nb - 1025), 9000 + np.arange(nb))
    # 6, 7: a side that ends exactly at a chunk's edge
    e1, e2 = with_renames(base(0), 1024, others=30), with_renames(base(1), 2048, others=60)
    lsoa = logs_soa(hot + [low, high, ea, eb, e1, e2], N_SYM)
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6)]
    assert len(ref(lsoa, 0, 1)) == 3000
    assert 0 < len(ref(lsoa, 2, 3)) < 1024 and 0 < len(ref(lsoa, 3, 2)) < 1024
    assert ref(lsoa, 4, 5)[0].tolist() == [1023, na + 1024] and len(ref(lsoa, 4, 5)) == 1 + nb - 1025
    ds, raw, res = run(lsoa, pairs, large=True)
    check_all(res, lsoa, pairs, "rounds")
    check_unwritten(ds, raw, "rounds")
    assert [int(c) for c in raw["counts"]] == [len(ref(lsoa, i, j)) for i, j in pairs]


def test_truncation_and_counts_only():
    lsoa = logs_soa([with_renames(base(0), 1500, others=100), with_renames(base(1), 1400, others=100)], N_SYM)
    full = ref(lsoa, 0, 1)
    n = len(full)
    assert n > 2
    pairs = [(0, 1)] * 4
    caps = [0, 1, n - 1, n]
    ds, raw, res = run(lsoa, pairs, large=True, conflict_caps=caps)
    assert raw["counts"][:4].tolist() == [n] * 4     # the full count, whatever the capacity
    for p, cap in enumerate(caps):
        assert np.array_equal(res[p], full[:cap]), f"capacity {cap}"
    check_unwritten(ds, raw, "truncation")
    ds, raw, res = run(lsoa, pairs[:2], large=True, conflict_caps="null")
    assert raw["counts"][:2].tolist() == [n, n]
    assert (raw["conf"] == FILL).all()


def test_grid_cap_one():
    logs = [with_renames(base(0, shuffle=True), 2049, others=100), with_renames(base(1, shuffle=True), 2100, others=100),
            with_renames(base(1), 60, others=20)]
    lsoa = logs_soa(logs, N_SYM)
    pairs = [(0, 1), (1, 0), (0, 0), (0, 2), (2, 1), (2, 2)]
    raws = {}
    for cap in (0, 1):
        ds, raws[cap], res = run(lsoa, pairs, large=True, grid_cap=cap)
        check_all(res, lsoa, pairs, f"grid_cap {cap}")
        check_unwritten(ds, raws[cap], f"grid_cap {cap}")
    for name, a in raws[0].items():
        assert a.tobytes() == raws[1][name].tobytes(), f"grid_cap 1: {name} differs from grid_cap 0"


def test_session_screen_and_screen_all():
    from test_gpu_cand import ren
    logs = [with_renames(base(0), 1100, others=20), with_renames(base(1), 1100, others=30),
            with_renames(base(1), 60, others=10), ren([(N_SYM - 1, 123456)], 5)]
    lsoa = _cand.logs_soa(logs, N_SYM)
    every = [(i, j) for i in range(4) for j in range(4)]
    sess = ComposeSession()
    routed = sess.screen(lsoa, every)
    assert sess.last["routed"] >= 1 and "large" not in sess.last
    streamed = sess.screen(lsoa, every, large=True)
    assert sess.last["routed"] == 0 and sess.last["large"] == 4     # (0, 0), (0, 1), (1, 0), (1, 1)
    for p, (g, w) in enumerate(zip(streamed, routed)):
        assert np.array_equal(g, w), f"pair {every[p]}"
    assert len(routed[1]) > 0
    assert all(np.array_equal(g, w) for g, w in zip(screen_soa(lsoa, every, large=True), routed))
    pairs0, found0 = sess.screen_all(lsoa)
    assert sess.last["routed"] >= 1
    pairs1, found1 = sess.screen_all(lsoa, large=True)
    assert sess.last["routed"] == 0 and sess.last["large"] >= 1
    assert np.array_equal(pairs0, pairs1) and [0, 1] in pairs1.tolist()
    for p, g, w in zip(pairs1.tolist(), found1, found0):
        assert np.array_equal(g, w), f"pair {p}"


def test_dropin_keyword():
    from semantic_merge_amd import screen_all, screen_conflicts

    def logs(n, seed):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 30, seed, **ADV)))

    ops = [to_ops(logs(300, 1)[0])] + [to_ops(logs(n, 10 + n)[1]) for n in (40, 150)] + [[]]
    ops.append(to_ops(logs(3600, 7)[0]))      # ~2160 renames: every pair that holds it is over the limit
    assert sum(o.type == "renameSymbol" for o in ops[4]) > _abi.SCREEN_MAX_RENAMES
    before = copy.deepcopy(ops)

    def dicts(cs):
        return jline([c.to_dict() for c in cs])

    for pairs in (None, [(4, 0), (0, 4), (4, 4), (1, 2), (3, 4)]):
        want = screen_conflicts(ops, pairs)
        got = screen_conflicts(ops, pairs, large=True)
        assert [dicts(g) for g in got] == [dicts(w) for w in want]
        assert any(got)
    want, got = screen_all(ops), screen_all(ops, large=True)
    assert list(got) == list(want) and any(4 in k for k in got)
    assert [dicts(got[k]) for k in got] == [dicts(want[k]) for k in want]
    assert ops == before
