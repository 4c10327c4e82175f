"""GPU parity of merge trains (smx_compose_train, csrc/smx_train.h) with the column-level train
oracle of tests/_train.py, exactly: the final accumulators, the steps that landed, every step's
length, outcome and conflict records.  Every output word starts as a canary, so the words a call
must not write are checked.  Shapes: trains of no log, one log, empty logs; train sums at the
size classes' edges; an accumulator that reaches exactly 2048 ops, and one that a log does not
fit behind (-2) while the next one does; a log in 50 trains and twice in one; 300 trains over
all three classes, also with one workgroup per class; unordered logs; truncated conflict
capacities; invalid logs mid-train; bad train and result offsets; the empty-file rule; and one
workspace serving differently shaped calls with smx_compose_pairs in between."""
import dataclasses

import numpy as np
import pytest

from semantic_merge_amd._lib import DevicePairs, DeviceTrains
from semantic_merge_amd.marshal import SoA

import _pairs
import _train
from _batch import ADV, MOVE, branch, own_logs
from _pairs import logs_soa
from _shapes import pick

pytestmark = pytest.mark.gpu

N_SYM = 64
RENAME = 1


def clean(n, seed):
    """A log of n ops without renames: it conflicts with nothing, so every step with it lands."""
    soa = branch(n, N_SYM, seed, seed & 1)
    soa.kind[soa.kind == RENAME] = 2
    return soa


def spoiled(soa, **cols):
    """A copy of a log with its middle op's columns set (an invalid kind or symbol)."""
    out = SoA(soa.n_a, soa.n_b, *[np.array(getattr(soa, c)) for c in _train.COLS], soa.n_sym)
    for c, v in cols.items():
        getattr(out, c)[out.n // 2] = v
    return out


# the logs of the pool, by name
NAMES = ("empty", "one", "o10", "o25", "o40", "o60", "o90", "o120", "a30", "a50", "c128a", "c128b", "c129", "c512a",
         "c512b", "c513", "c1024", "c1016", "c9", "c8", "badkind", "badsym")
IX = {name: i for i, name in enumerate(NAMES)}


@pytest.fixture(scope="module")
def pool():
    own = own_logs(N_SYM, 100, [10, 25, 40, 60, 90, 120])  # divergent renames, None-valued moves, a shuffled log
    adv = [branch(n, N_SYM, 40 + n, 0, **ADV) for n in (30, 50)]
    sizes = (128, 128, 129, 512, 512, 513, 1024, 1016, 9, 8)
    logs = [pick(own[0], np.zeros(own[0].n_a, bool), np.zeros(own[0].n_b, bool)), branch(1, N_SYM, 3, 1)] + own + adv
    logs += [clean(n, 7 + i) for i, n in enumerate(sizes)]
    logs += [spoiled(own[1], kind=18), spoiled(own[2], sym=N_SYM)]
    assert len(logs) == len(NAMES) and [x.n for x in logs[10:20]] == list(sizes)
    return logs_soa(logs, N_SYM)


def T(*names):
    return [IX[n] for n in names]


def test_small_trains_and_class_edges(pool):
    trains = [[], T("one"), T("empty"), T("empty", "o25", "empty", "o40"), T("o10", "o25", "o40", "o60", "o90", "o120"),
              T("a30", "o60", "a50", "o90", "a30"),
              T("c128a", "c128b"), T("c128a", "c129"), T("c512a", "c512b"), T("c512a", "c513"),
              T("c1024", "c512a", "c512b"), T("c1024", "c1016", "c9", "c8"),
              T("o60", "o60", "c9"), T("a50", "a50", "o25"), T("o120", "a30", "c513", "o90", "a50", "c129")]
    db, raw = _train.run(pool, trains)
    res = _train.check(db, raw, "edges")
    assert res[0][4] == 0 and len(res[0][0]) == 0 and res[2][4] == 1
    assert [len(res[t][0]) for t in (6, 7, 8, 9, 10)] == [256, 257, 1024, 1025, 2048]
    assert [s[:2] for s in res[11][5]] == [(1024, 0), (2040, 0), (2040, -2), (2048, 0)]
    assert any(oc > 0 for r in res if not isinstance(r, int) for _, oc, _ in r[5]), "no step was evicted"
    assert any(oc > 0 and any(o == 0 for _, o, _ in r[5][s + 1:]) for r in res for s, (_, oc, _) in enumerate(r[5]))
    # the accumulated values: some entry carries an addr / file / ctx, and a conflict record one
    for f in (1, 2, 3):
        assert any((r[f] != -1).any() for r in res)
    assert any((recs[:, 2:] != -1).any() for r in res for _, _, recs in r[5])


@pytest.fixture(scope="module")
def many(pool):
    """300 trains: a log in 50 of them, short trains of all three classes."""
    rng = np.random.default_rng(11)
    small = T("empty", "one", "o10", "o25", "o40", "o60", "a30", "a50")
    trains = [[IX["o40"], small[r % len(small)]] for r in range(50)]
    while len(trains) < 280:
        trains.append(rng.choice(small, rng.integers(1, 5)).tolist())
    mid = T("c128a", "c129", "c512a", "o90", "o120", "a50", "o25")
    while len(trains) < 294:
        trains.append(rng.choice(mid, rng.integers(2, 5)).tolist())
    big = T("c1024", "c513", "c512b", "o120", "a30")
    while len(trains) < 300:
        trains.append(rng.choice(big, 3, replace=False).tolist())
    return trains


def test_300_trains_over_all_classes(pool, many):
    lens = np.diff(pool.log_off)
    sums = [int(sum(lens[l] for l in tr)) for tr in many]
    assert min(sums) <= 256 and any(256 < s <= 1024 for s in sums) and any(s > 1024 for s in sums)
    db, raw = _train.run(pool, many)
    res = _train.check(db, raw, "300 trains")
    db1, raw1 = _train.run(pool, many, grid_cap=1)
    res1 = _train.check(db1, raw1, "300 trains, one workgroup per class")
    for name in raw:
        assert raw[name].tobytes() == raw1[name].tobytes(), name
    assert sum(1 for r in res for _, oc, _ in r[5] if oc > 0) > 20


@pytest.mark.parametrize("cap", [0, 1])
def test_truncated_conflict_capacity(pool, cap):
    trains = [T("a50", "a50", "o25"), T("o10", "o25", "o40", "o60", "o90", "o120"), T("o60", "a50", "o25")]
    want = [_train.ref(pool, tr) for tr in trains]
    outcomes = [oc for w in want for _, oc, _ in w[5]]
    truncated = [g for g, oc in enumerate(outcomes) if oc > cap]
    assert truncated
    db, raw = _train.run(pool, trains, conflict_caps=[cap] * len(outcomes))
    _train.check(db, raw, f"capacity {cap}", truncated=truncated)


def test_invalid_logs_mid_train(pool):
    trains = [T("o25", "badkind", "o40", "badsym", "o60") + [-1, IX["o10"], len(NAMES), IX["a30"]], T("badkind"),
              T("o10", "o25")]
    db, raw = _train.run(pool, trains)
    res = _train.check(db, raw, "invalid logs")
    assert [oc for _, oc, _ in res[0][5]][1::2][:3] == [-1, -1, -1] and res[0][5][7][1] == -1
    assert res[0][4] >= 1 and res[1][4] == 0 and res[1][5][0][:2] == (0, -1)
    # a log whose offsets decrease: invalid under smx_screen's rules, and so is no other
    off = np.array(pool.log_off)
    off[IX["o40"]] = off[IX["o25"]] - 1
    db, raw = _train.run(pool, trains, log_off=off)
    res = _train.check(db, raw, "a log with a decreasing offset", log_off=off)
    assert res[0][5][2][1] == -1


def test_bad_train_and_result_offsets(pool):
    trains = [T("o10", "o25"), T("o40", "o60"), T("o90"), T("a30", "o10"), T("one")]
    own = np.array([0, 2, 4, 5, 7, 8], np.int64)
    lens = np.diff(pool.log_off)
    need = [int(sum(lens[l] for l in tr)) for tr in trains]
    res_off = np.concatenate([[0], np.cumsum(need)]).astype(np.int64)
    # train 1's steps end before they start; train 3's leave the steps
    bad_t = own.copy()
    bad_t[2] = 1
    db, raw = _train.run(pool, trains, train_off=bad_t)
    _train.check(db, raw, "train_off decreases", failed={1, 2})
    past = own.copy()
    past[4:] = [9, 9]
    db, raw = _train.run(pool, trains, train_off=past)
    _train.check(db, raw, "train_off past the steps", failed={3, 4})
    # a region one entry short, a negative one, one past n_out
    short = res_off.copy()
    short[3:] -= 1
    db, raw = _train.run(pool, trains, res_off=short)
    _train.check(db, raw, "a region one entry short", failed={2})
    neg = res_off.copy()
    neg[0] = -1
    db, raw = _train.run(pool, trains, res_off=neg)
    _train.check(db, raw, "a negative result offset", failed={0})
    db, raw = _train.run(pool, trains, n_out=int(res_off[-1]) - 1)
    _train.check(db, raw, "a region past n_out", failed={4})


def test_empty_file_rule(pool):
    """empty_str names an id that moves carry as their file: where a move has gathered it, its v1
    is v1_alt's entry instead.  Half of the moves of a copy of the pool get that id."""
    mv = np.flatnonzero((np.asarray(pool.kind) == MOVE) & (np.asarray(pool.v1) >= 0))
    ids = np.unique(np.asarray(pool.v1)[mv])
    empty = int(ids[0])
    v1 = np.array(pool.v1)
    v1[mv[::2]] = empty
    pool = dataclasses.replace(pool, v1=v1)
    alt = np.random.default_rng(3).choice(np.concatenate([ids[1:], [-1]]), pool.n_total).astype(np.int32)
    trains = [T("o10", "o25", "o40", "o60", "o90", "o120"), T("o120", "o90", "a30", "o60", "o25"), T("o25", "o25", "o40")]
    kw = dict(v1_alt=alt, empty_str=empty)
    plain = [_train.ref(pool, tr) for tr in trains]
    ruled = [_train.ref(pool, tr, **kw) for tr in trains]
    assert any(not np.array_equal(p[2], r[2]) for p, r in zip(plain, ruled)), "the rule changes nothing here"
    db, raw = _train.run(pool, trains, **kw)
    _train.check(db, raw, "empty file", **kw)


def test_one_workspace_for_differently_shaped_calls(pool, many):
    a = DeviceTrains(pool, many[:120], fill=_train.FILL)
    b = DeviceTrains(pool, [T("c1024", "c512a", "c512b"), T("a30", "o60", "a50")], fill=_train.FILL)
    pairs = [(IX["o10"], IX["o25"]), (IX["a30"], IX["a50"]), (IX["c128a"], IX["o60"])]
    p = DevicePairs(pool, pairs, fill=_pairs.FILL)
    big = max((a, b, p), key=lambda x: x.ws_bytes)
    for x in (a, b, p):
        x.ws, x.ws_bytes = big.ws, big.ws_bytes
    big.ws.fill_(0xA5)
    a.run()
    p.run()
    b.run()
    _train.check(b, b.raw(), "second shape")
    _pairs.check(p, p.raw(), "pairs in between")
    first = a.raw()
    _train.check(a, first, "first shape")
    a.run()
    again = a.raw()
    for name in first:
        assert first[name].tobytes() == again[name].tobytes(), name
