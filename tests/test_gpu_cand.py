"""GPU parity of the candidate pairs (smx_screen_candidates, csrc/smx_cand.h) with the rule
restated in tests/_cand.py: the pairs, their order, counts and log_info; hot symbols across the
bit matrix's word edges, degenerate logs and symbols, invalid logs between valid ones, the pair
capacity, workspace reuse, and screen_all against the screen of all pairs."""
import copy

import numpy as np
import pytest

from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import ComposeSession, DeviceCandidates, SmxError, screen_all_soa, screen_soa

import _cand
from _batch import ADV, branch
from _screen import empty_log, make_log, with_renames
from _util import jline, to_ops

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A  # what every output word holds before a run
RENAME = _cand.RENAME


def ren(sym_v0, ts0=1000, extra=0):
    """A log of renames (sym, v0), one per millisecond, and `extra` ops of kind 0 after them."""
    n = len(sym_v0) + extra
    return make_log([RENAME] * len(sym_v0) + [0] * extra, ts0 + np.arange(n), np.arange(n) + 1, np.arange(n) + 1,
                    [s for s, _ in sym_v0] + [0] * extra, [v for _, v in sym_v0] + [0] * extra)


def run(lsoa, **kw):
    dc = DeviceCandidates(lsoa, fill=FILL, **kw)
    dc.run()
    return dc, dc.raw()


def check(dc, raw, want, info, label, with_log_info=True):
    """The outputs against the expected pairs and log_info; every other word is as it was."""
    n, k, L = len(want), min(len(want), dc.pair_cap), dc.n_logs
    assert int(raw["counts"][0]) == n, f"{label}: {raw['counts'][0]} candidates, {n} expected"
    assert int(raw["counts"][1]) == int((info < 0).sum()), f"{label}: invalid logs"
    assert (raw["counts"][2:] == FILL).all(), f"{label}: written after counts"
    got = np.stack([raw["pair_a"][:k], raw["pair_b"][:k]], axis=1)
    assert np.array_equal(got, want[:k]), f"{label}: the pairs or their order"
    for name in ("pair_a", "pair_b"):
        assert (raw[name][k:] == FILL).all(), f"{label}: {name} written at or past {k}"
    if with_log_info:
        assert raw["log_info"][:L].tolist() == info.tolist(), f"{label}: log_info"
        assert (raw["log_info"][L:] == FILL).all(), f"{label}: written after log_info"
    else:
        assert (raw["log_info"] == FILL).all(), f"{label}: log_info written though NULL"


def run_check(lsoa, label, **kw):
    want, info = _cand.candidates(lsoa, kw.get("log_off"), kw.get("n_total"))
    dc, raw = run(lsoa, **kw)
    check(dc, raw, want, info, label, kw.get("with_log_info", True))
    return want, info, raw


@pytest.fixture(scope="module")
def forty():
    """40 sparse logs of 10-400 ops and their expected candidates."""
    lsoa = _cand.sparse_logs(40, 160, 11)
    want, info = _cand.candidates(lsoa)
    assert 40 < len(want) < 40 * 39 // 2 - 40    # pairs on both sides of the rule
    return lsoa, want, info


def test_sparse_logs(forty):
    lsoa, want, info = forty
    dc, raw = run(lsoa)
    check(dc, raw, want, info, "C ABI")
    sess = ComposeSession()
    got = sess.candidates(lsoa)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert sess.last["retries"] == 0 and sess.last["n_candidates"] == len(want)
    assert sess.last["in_bytes"] < 9 * lsoa.n_total + 8 * 41 + 4 * 256    # kind, sym, v0 and the offsets


def test_constructed_cases():
    three = _cand.logs_soa([ren([(2, 7)]), ren([(2, 7)], 2000), ren([(2, 9)], 3000)], 4)
    want, _, _ = run_check(three, "same name twice, a third that differs")
    assert want.tolist() == [[0, 2], [1, 2]]
    twice = _cand.logs_soa([ren([(2, 7), (2, 8)]), ren([(2, 7)], 1001)], 4)
    want, _, _ = run_check(twice, "x then y against x")
    assert want.tolist() == [[0, 1]]
    same = _cand.logs_soa([ren([(2, 7), (2, 7)]), ren([(2, 7)], 1001)], 4)
    want, _, _ = run_check(same, "x twice against x")
    assert want.tolist() == []


@pytest.mark.parametrize("n_logs", [65, 257])
def test_hot_symbol(n_logs):
    """One symbol renamed in every log: the group loop's wave strides and the matrix's word
    edges (n_logs is no multiple of 32).  Distinct classes: every pair; one class: none."""
    for distinct in (True, False):
        lsoa = _cand.logs_soa([ren([(77, 1000 + l if distinct else 5)], 1000 + l, extra=l % 3)
                               for l in range(n_logs)], 100)
        want, info, _ = run_check(lsoa, f"{n_logs} logs, distinct={distinct}")
        assert len(want) == (n_logs * (n_logs - 1) // 2 if distinct else 0)
        assert len(want) in (2080, 32896, 0)


def test_large_and_degenerate_logs():
    # a log of 2100 renames over 300 symbols next to small ones takes part: the limit is the screen's
    big = ren([(k % 300, 5000 + k) for k in range(2100)])
    small = [ren([(5, 1)], 9000, extra=3), ren([(299, 2)], 9100), ren([(300, 3)], 9200), empty_log(),
             ren([], 9300, extra=12), ren([(5, 1), (300, 4)], 9400)]
    lsoa = _cand.logs_soa([big] + small, 400)
    want, info, _ = run_check(lsoa, "2100 renames")
    assert info[0] == 2100 and info[4] == 0 and info[5] == 0
    assert want.tolist() == [[0, 1], [0, 2], [0, 6], [3, 6]]
    # one log alone; all logs empty; no renames anywhere
    for label, logs in (("one log", [big]), ("empty logs", [empty_log()] * 3), ("no renames", [ren([], 1, extra=40)] * 2)):
        want, info, _ = run_check(_cand.logs_soa(logs, 400), label)
        assert len(want) == 0


def test_symbol_and_class_extremes():
    syms = [0, 1 << 31, 0xFFFFFFFF]
    logs = [ren([(s, v) for s in syms], 1000 + 10 * i) for i, v in enumerate((-1, -1, 0, 0x7FFFFFFF))]
    logs.append(ren([(0xFFFFFFFF, -1), ((1 << 31) - 1, 3)], 2000))
    logs.append(ren([(0xFFFFFFFE, -2), (1, -1)], 2100))
    want, info, _ = run_check(_cand.logs_soa(logs, 4), "sym 0, 2^31, 2^32 - 1; v0 -1")
    assert want.tolist() == [[0, 2], [0, 3], [1, 2], [1, 3], [2, 3], [2, 4], [3, 4]]


def test_entries_no_log_covers_are_not_read(forty):
    lsoa, want, info = forty
    parts = [lsoa.pair(l, l) for l in range(6)]
    for p in parts:   # (log l alone, as a one-branch SoA)
        for c in _cand.COLS:
            setattr(p, c, getattr(p, c)[: p.n_a])
        p.n_b = 0
    gap = _cand.logs_soa(parts, lsoa.n_sym, head=37, tail=300)
    assert (gap.kind[:37] == 0xFF).all() and (gap.kind[-300:] == 0xFF).all()
    w, i, _ = run_check(gap, "kind 255 before the first and after the last log")
    assert (i >= 0).all() and np.array_equal(w, want[(want < 6).all(axis=1)])


def test_invalid_logs_do_not_touch_their_neighbours(forty):
    lsoa, want, info = forty
    L = lsoa.n_logs

    def without(bad):
        return want[~np.isin(want, list(bad)).any(axis=1)]

    # kind 18 in an op of log 3 that is no rename, kind 200 in a rename's place in log 17
    bad = copy.deepcopy(lsoa)
    o3, o17 = int(lsoa.log_off[3]), int(lsoa.log_off[17])
    bad.kind[o3 + int(np.flatnonzero(lsoa.kind[o3: int(lsoa.log_off[4])] != RENAME)[-1])] = 18
    bad.kind[o17 + int(np.flatnonzero(lsoa.kind[o17: int(lsoa.log_off[18])] == RENAME)[0])] = 200
    w, i, _ = run_check(bad, "kind >= 18")
    assert np.flatnonzero(i < 0).tolist() == [3, 17]
    assert len(without({3, 17})) < len(want)
    # (log 17 lost one rename to the bad kind; its pairs are gone with it, every other log is as it was)
    assert np.array_equal(w, without({3, 17}))
    # log 9 ends 5 ops before it starts; log 10 then starts before log 9's offset: both fail
    off = lsoa.log_off.copy()
    off[10] = off[9] - 5
    w, i, _ = run_check(lsoa, "decreasing offsets", log_off=off)
    assert np.flatnonzero(i < 0).tolist() == [9, 10] and np.array_equal(w, without({9, 10}))
    # the last log ends past n_total
    w, i, _ = run_check(lsoa, "the last offset past n_total", n_total=lsoa.n_total - 1)
    assert np.flatnonzero(i < 0).tolist() == [L - 1] and np.array_equal(w, without({L - 1}))
    with pytest.raises(SmxError, match="log 3:"):
        ComposeSession().candidates(bad)


def test_pair_capacity(forty):
    lsoa, want, info = forty
    n = len(want)
    for cap in (n - 1, 7, 1):
        run_check(lsoa, f"pair_cap {cap}", pair_cap=cap)
    run_check(lsoa, "pair_cap = count", pair_cap=n)
    dc, raw = run(lsoa, pair_cap=0, with_log_info=False)    # NULL pair arrays, NULL log_info
    assert dc._arg.pair_a is None and dc._arg.pair_b is None and dc._arg.log_info is None
    check(dc, raw, want, info, "the count alone", with_log_info=False)


def test_one_workgroup_gives_the_same(forty):
    lsoa, want, info = forty
    _, a = run(lsoa)
    dc, b = run(lsoa, grid_cap=1)
    check(dc, b, want, info, "grid_cap 1")
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), f"grid_cap 1: {name} differs from grid_cap 0"


def test_one_workspace_serves_different_calls(forty):
    lsoa, want, info = forty
    hot = _cand.logs_soa([ren([(77, 1000 + l)], 1000 + l) for l in range(40)], 100)
    hw, hi = _cand.candidates(hot)
    first, second = DeviceCandidates(lsoa, fill=FILL), DeviceCandidates(hot, fill=FILL)
    big = first if first.ws_bytes >= second.ws_bytes else second
    first.ws = second.ws = big.ws    # (each call passes its own size, the buffer holds the larger)
    for dc, w, i, label in ((second, hw, hi, "hot"), (first, want, info, "sparse after hot"),
                            (second, hw, hi, "hot after sparse")):
        dc.run()
        check(dc, dc.raw(), w, i, label)


def test_session_retries_with_the_exact_count(forty):
    lsoa, want, info = forty
    sess = ComposeSession()
    got = sess.candidates(lsoa, start_cap=5)
    assert sess.last["retries"] == 1 and np.array_equal(got, want)
    got = sess.candidates(lsoa, start_cap=len(want))
    assert sess.last["retries"] == 0 and np.array_equal(got, want)


def test_screen_all_equals_the_screen_of_all_pairs(forty):
    lsoa, want, info = forty
    L, tot = lsoa.n_logs, lsoa.n_total
    every = [(i, j) for i in range(L) for j in range(i + 1, L)]
    full = dict(zip(every, screen_soa(lsoa, every)))
    sess = ComposeSession()
    pairs, found = sess.screen_all(lsoa)
    assert np.array_equal(pairs, want) and len(found) == len(want)
    cand = set(map(tuple, want.tolist()))
    for p, g in zip(map(tuple, pairs.tolist()), found):
        assert np.array_equal(g, full[p]), f"pair {p}"
    for p in every:
        if p not in cand:
            assert len(full[p]) == 0, f"pair {p} is no candidate but the screen finds conflicts"
    assert any(len(g) for g in found) and any(len(g) == 0 for g in found)
    # the six columns went to the device once: 33 bytes per op, the offsets, conf_off, padding
    last = sess.last
    assert last["n_candidates"] == len(want) and last["routed"] == 0
    assert 33 * tot <= last["in_bytes"] <= 33 * tot + 8 * (L + 1) + 8 * (len(want) + 1) + 7 * 256
    assert last["in_bytes"] < 2 * 33 * tot
    p2, f2 = screen_all_soa(lsoa)
    assert np.array_equal(p2, pairs) and all(np.array_equal(x, y) for x, y in zip(f2, found))


def test_screen_all_routes_pairs_over_the_rename_limit():
    n_sym = 40
    base = [branch(6000, n_sym, 60 + s, s, **ADV) for s in (0, 1)]
    logs = [with_renames(base[0], 1100, others=20), with_renames(base[1], 1100, others=30),
            with_renames(base[1], 60, others=10), ren([(n_sym - 1, 123456)], 5)]
    lsoa = _cand.logs_soa(logs, n_sym)
    want, _ = _cand.candidates(lsoa)
    every = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    full = dict(zip(every, screen_soa(lsoa, every)))
    sess = ComposeSession()
    pairs, found = sess.screen_all(lsoa)
    assert np.array_equal(pairs, want) and [0, 1] in pairs.tolist()
    assert sess.last["routed"] >= 1    # (0, 1): 2200 renames
    for p, g in zip(map(tuple, pairs.tolist()), found):
        assert np.array_equal(g, full[p]), f"pair {p}"
    assert len(full[(0, 1)]) > 0


def test_dropin_screen_all():
    from semantic_merge_amd import screen_all, screen_conflicts

    def logs(n, seed, n_sym):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **ADV)))

    ops = [to_ops(logs(200, 1, 30)[0])] + [to_ops(logs(n, 10 + n, 30)[1]) for n in (40, 150, 90)] + [[]]
    ops += [to_ops(logs(60, 5, 3)[0]), to_ops(logs(50, 6, 2)[1])]
    before = copy.deepcopy(ops)
    ids = [id(o) for log in ops for o in log]
    got = screen_all(ops)
    dense = screen_conflicts(ops)
    every = [(i, j) for i in range(len(ops)) for j in range(i + 1, len(ops))]
    want = {p: c for p, c in zip(every, dense) if c}
    assert list(got) == list(want) and len(want) > 0 and len(want) < len(every)
    for p in want:
        assert jline([c.to_dict() for c in got[p]]) == jline([c.to_dict() for c in want[p]]), f"pair {p}"
    assert ops == before and ids == [id(o) for log in ops for o in log]
    assert screen_all([]) == {} and screen_all([ops[0]]) == {}
