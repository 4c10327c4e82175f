"""GPU parity of the train screen (smx_screen_train, csrc/smx_screen_train.h) with the train
oracles of tests/_screen_train.py, exactly: every step's outcome, the renames its accumulator
holds and its (A column, B column) conflict records, the final counts.  Every output word starts
as a canary, so the words a call must not write are checked.  Shapes: the golden trains; orders
that decide a walk (equal full keys, a log twice, a log in many trains, eviction, a partner that an
earlier step brought); accumulators and logs at the edges of a round (1023 / 1024 / 1025 renames),
a log through the large extraction, an accumulator past 2048 renames with its conflicts in the
last round; the shape smx_compose_train refuses; empties; truncation; failures; one workgroup
for everything; one workspace for several calls; the public call."""
import copy

import numpy as np
import pytest

from semantic_merge_amd import marshal as M
from semantic_merge_amd import synth
from semantic_merge_amd._lib import DeviceScreen, DeviceScreenTrains, DeviceTrains

import _screen
import _screen_train as ST
from _batch import ADV, branch, own_logs
from _pairs import logs_soa
from _screen import RENAME, make_log, with_renames
from _util import load, to_ops

pytestmark = pytest.mark.gpu

N_SYM = 40
WIDE = 8 * N_SYM   # the symbol bound of the pools: shifted copies of a log rename other symbols
OTHER = 2          # the kind of the ops that are no renames in the logs given by column
_base = {}


def base(side, shuffle=False):
    """A branch log of 7200 ops, about 4300 of them renames, computed once."""
    key = (side, shuffle)
    if key not in _base:
        _base[key] = branch(7200, N_SYM, 60 + side + 10 * shuffle, side, **ADV, shuffle=shuffle)
    return _base[key]


def renames(ts, hi, lo, sym, v0, extra=0):
    """A log of renames given by column, and `extra` other ops after them."""
    n = len(ts)
    pad = [0] * extra
    return make_log([RENAME] * n + [OTHER] * extra, list(ts) + pad, list(hi) + pad, list(lo) + pad,
                    list(sym) + pad, list(v0) + pad, WIDE)


def shifted(soa, k):
    """A copy of a log whose symbols are k * N_SYM higher: it conflicts with nothing of the original."""
    out = copy.deepcopy(soa)
    out.sym[:] = out.sym + np.uint32(k * N_SYM)
    return out


def outcomes(res, t):
    return [oc for _, oc, _ in res[t][2]]


# -- the golden trains ---------------------------------------------------------------------------

def test_golden_trains():
    """All golden cases in one call: their logs marshalled together, one train per case."""
    cases = load("train_cases.json")
    logs, trains, first = [], [], []
    for case in cases:
        first.append(len(logs))
        trains.append([len(logs) + l for l in case["train"]])
        logs += [to_ops([_golden_op(s) for s in log]) for log in case["logs"]]
    lsoa = M.marshal_logs(logs)
    db, raw = ST.run(lsoa, trains)
    res = ST.check(db, raw, "golden", full=False)
    off = np.asarray(lsoa.log_off)
    n_conf = 0
    for c, case in enumerate(cases):
        assert outcomes(res, c) == [len(s) for s in case["steps"]], f"case {c}: outcomes"
        for (_, _, recs), step in zip(res[c][2], case["steps"]):
            want = [[off[first[c] + a[0]] + a[1], off[first[c] + b[0]] + b[1]] for a, b in step]
            assert recs.tolist() == want, f"case {c}: the conflicts' ops"
            n_conf += len(want)
    assert n_conf >= 50


def _golden_op(s):
    prov = {"rev": "base", **({"timestamp": s[5][0]} if s[5] else {})}
    return {"id": s[0], "schemaVersion": 1, "type": s[1], "target": {"symbolId": s[2], "addressId": s[3]},
            "params": s[4], "guards": s[6] if len(s) > 6 else {}, "effects": s[7] if len(s) > 6 else {},
            "provenance": prov}


# -- order ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool():
    """0-5: adversarial logs with divergent renames, None-valued moves, a shuffled log; 6, 7: two more
    branches; 8-10: three logs by column whose renames have equal full keys."""
    logs = own_logs(N_SYM, 100, [10, 25, 40, 60, 90, 120]) + [branch(n, N_SYM, 40 + n, 0, **ADV) for n in (30, 50)]
    ts, ids = [10, 20, 20, 30], [1, 2, 2, 3]     # (the middle two: equal keys inside a log too)
    logs += [renames(ts, ids, ids, [1, 2, 3, 4], [1, 1, 1, 1], extra=2),
             renames(ts, ids, ids, [5, 6, 7, 8], [2, 2, 2, 2], extra=1),
             renames(ts, ids, ids, [5, 2, 7, 4], [2, 9, 9, 1])]
    for x in logs:
        x.n_sym = WIDE
    return logs_soa(logs, WIDE)


def test_order_decides(pool):
    trains = [[8, 9, 10], [9, 8, 10], [10, 9, 8], [8, 8, 10], [10, 10, 9, 9],     # equal full keys, a log twice
              [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [6, 3, 7, 4, 6], [3, 3, 6], [7, 7, 1],
              [2, 4, 0, 5, 1, 3], [4, 6, 5, 7, 2]] + [[3, k] for k in range(8)]      # log 3 in many trains
    db, raw = ST.run(pool, trains)
    res = ST.check(db, raw, "order")
    # the equal keys decide: the same three logs give other conflicts in another order
    assert outcomes(res, 0) != outcomes(res, 1) or not np.array_equal(res[0][2][2][2], res[1][2][2][2])
    assert max(outcomes(res, 0)) > 0 and max(outcomes(res, 3)) > 0
    off = np.asarray(pool.log_off)
    seen = dict.fromkeys(("evicted then the next lands on the same accumulator", "a partner a later step brought"), 0)
    for t, tr in enumerate(trains):
        steps = res[t][2]
        for s, (acc, oc, recs) in enumerate(steps):
            if oc > 0 and s + 1 < len(steps) and steps[s + 1][1] == 0:
                assert acc == (steps[s - 1][0] if s else 0)
                seen["evicted then the next lands on the same accumulator"] += 1
            landed = [q for q in range(s) if steps[q][1] == 0]
            if oc > 0 and len(landed) >= 2:
                logs_a = set((np.searchsorted(off, recs[:, 0], "right") - 1).tolist())
                seen["a partner a later step brought"] += int(bool(logs_a - {tr[landed[0]]}))
    assert all(seen.values()), seen


# -- streaming and merge edges -------------------------------------------------------------------

def test_round_edges():
    """Accumulators of 1023 / 1024 / 1025 renames against logs of 1 / 1024 / 1025: the walk (the
    log conflicts), and the merge (a copy of the log on other symbols lands) with a walk over the
    merged accumulator behind it."""
    A = [with_renames(base(0), r, others=20) for r in (1023, 1024, 1025)]
    B = [with_renames(base(1), r, others=20) for r in (1, 1024, 1025)]
    last = with_renames(base(1, shuffle=True), 60, others=10)
    logs = A + B + [shifted(b, 1) for b in B] + [last, shifted(last, 1)]
    for x in logs:
        x.n_sym = WIDE
    lsoa = logs_soa(logs, WIDE)
    trains = []
    for a in range(3):
        for b in range(3):
            trains += [[a, 3 + b], [a, 6 + b, 9 + (b & 1)]]
    db, raw = ST.run(lsoa, trains)
    res = ST.check(db, raw, "round edges")
    assert all(outcomes(res, t)[1] > 0 for t in range(0, 18, 2) if (t // 2) % 3)     # (a log of one rename may miss)
    assert all(outcomes(res, t)[:2] == [0, 0] and outcomes(res, t)[2] > 0 for t in range(1, 18, 2))
    assert sorted({res[t][2][1][0] for t in range(1, 18, 2)}) == [1024, 1025, 1026, 2047, 2048, 2049, 2050]


def test_large_log_and_accumulator_past_2048():
    rng = np.random.default_rng(5)
    big = with_renames(base(0, shuffle=True), 2049, others=100)      # through k_screen_extract_large
    small = with_renames(base(1, shuffle=True), 300, others=20)
    P = []
    for k in range(3):   # 900 renames each on symbols of their own, interleaved timestamps
        n = 900
        tail = k == 2
        ts = np.sort(rng.integers(1000, 9000, n - 10 * tail)).tolist() + [9001 + i for i in range(10 * tail)]
        sym = (50 + 10 * k + rng.integers(0, 10, n - 10 * tail)).tolist() + [177] * (10 * tail)
        P.append(renames(ts, rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n), sym, rng.integers(0, 3, n), extra=5))
    # its ten renames meet the accumulator's last ten: the conflicts lie in the walk's last round
    Q = renames([9001 + i for i in range(10)], [1 << 62] * 10, range(10), [177] * 10, [7] * 10, extra=3)
    logs = [big, small, shifted(small, 2)] + P + [Q]
    for x in logs:
        x.n_sym = WIDE
    lsoa = logs_soa(logs, WIDE)
    trains = [[0, 1], [1, 0], [2, 0, 1], [0, 0], [3, 4, 5, 6], [5, 4, 3, 6, 1]]
    db, raw = ST.run(lsoa, trains)
    res = ST.check(db, raw, "large")
    assert outcomes(res, 0)[1] > 0 and outcomes(res, 1)[1] > 0
    assert [s[:2] for s in res[2][2]][:2] == [(300, 0), (2349, 0)] and outcomes(res, 2)[2] > 0
    assert [s[:2] for s in res[4][2]] == [(900, 0), (1800, 0), (2700, 0), (2700, 10)]
    assert res[4][2][3][2][:, 1].tolist() == (int(lsoa.log_off[6]) + np.arange(10)).tolist()


def test_the_shape_compose_train_refuses():
    """3 logs of 3000 ops with 40 renames each: smx_compose_train reports -2 for every step (a log
    alone exceeds 2048 ops), the screen answers all of them."""
    rng = np.random.default_rng(9)
    logs = []
    for k in range(3):
        n, r = 3000, 40
        kind = np.full(n, OTHER)
        at = np.sort(rng.choice(n, r, replace=False))
        kind[at] = RENAME
        sym = rng.integers(0, N_SYM, n)
        sym[at] = rng.integers(0, 12, r)
        logs.append(make_log(kind, np.sort(rng.integers(1000, 1400, n)), rng.integers(0, 1 << 62, n),
                             rng.integers(0, 1 << 62, n), sym, rng.integers(0, 2, n), WIDE))
    logs.append(shifted(logs[1], 1))
    lsoa = logs_soa(logs, WIDE)
    trains = [[0, 1, 2], [2, 3, 0, 1]]
    old = DeviceTrains(lsoa, trains)
    old.run()
    assert all(oc == -2 for r in old.results() for _, oc, _ in r[5])
    db, raw = ST.run(lsoa, trains)
    res = ST.check(db, raw, "refused shape")
    assert min(outcomes(res, 0) + outcomes(res, 1)) >= 0 and max(outcomes(res, 0) + outcomes(res, 1)) > 0
    assert outcomes(res, 1)[:2] == [0, 0] and res[1][2][1][0] == 80


# -- empties, truncation, failures ---------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """0: no ops; 1: ops but no renames; 2: one symbol renamed to "1" five times; 3-5: the same
    symbol renamed to other names at the same times; 6, 7: adversarial branches; 8: no renames."""
    t = [10, 20, 30, 40, 50]
    logs = [_screen.empty_log(WIDE), renames([], [], [], [], [], extra=6),
            renames(t, t, t, [3] * 5, [1] * 5, extra=2)]
    logs += [renames(t, t, [x + k for x in t], [3] * 5, [1 + k] * 5, extra=k) for k in (1, 2, 3)]
    logs += [with_renames(base(0), 300, others=40), with_renames(base(1), 200, others=40), renames([], [], [], [], [], extra=1)]
    for x in logs:
        x.n_sym = WIDE
    return logs_soa(logs, WIDE)


def test_empties(small):
    trains = [[], [0], [1], [0, 1, 8, 0], [0, 2, 1, 0, 3, 8], [2, 3, 4, 5], [1, 6, 0, 7, 8], []]
    db, raw = ST.run(small, trains)
    res = ST.check(db, raw, "empties")
    assert res[0] == (0, 0, []) and res[7] == (0, 0, [])
    assert res[3][:2] == (0, 4) and outcomes(res, 3) == [0] * 4        # logs without renames land
    assert [s[:2] for s in res[4][2]] == [(0, 0), (5, 0), (5, 0), (5, 0), (5, 5), (5, 0)]
    assert res[5][:2] == (5, 1) and outcomes(res, 5) == [0, 5, 5, 5]   # the accumulator stays at the first log


@pytest.mark.parametrize("caps", [0, 2, "null"])
def test_truncated_capacity(small, caps):
    trains = [[2, 3, 4], [6, 7], [3, 2]]
    want = [ST.ref(small, tr) for tr in trains]
    oc = [o for w in want for _, o, _ in w[2]]
    assert oc[1] == 5 and oc[4] > 2
    truncated = [g for g, o in enumerate(oc) if o > (0 if caps == "null" else caps)]
    db, raw = ST.run(small, trains, conf_caps=caps if caps == "null" else [caps] * len(oc))
    ST.check(db, raw, f"capacity {caps}", truncated=truncated)
    if caps == "null":
        assert (raw["conf"] == np.int32(ST.FILL)).all()


def test_failures(small):
    bad = copy.deepcopy(small)
    bad.kind[int(bad.log_off[3]) + 2] = 18
    trains = [[2, 3, 4, -1, 5, 99, 6], [3], [7, 3, 6], [2, 4]]
    db, raw = ST.run(bad, trains)
    res = ST.check(db, raw, "kind 18 and indices out of range")
    assert outcomes(res, 0)[1] == -1 and outcomes(res, 0)[3] == -1 and outcomes(res, 0)[5] == -1
    assert outcomes(res, 0)[2] == 5 and res[1][:2] == (0, 0) and res[1][2][0][:2] == (0, -1)
    assert outcomes(res, 2)[1] == -1 and outcomes(res, 2)[0] == 0 and outcomes(res, 3) == [0, 5]
    # offsets
    trains = [[2, 3], [6, 7], [4], [7, 2], [5]]
    own = np.array([0, 2, 4, 5, 7, 8], np.int64)
    acc = np.concatenate([[0], np.cumsum([10, 500, 5, 205, 5])]).astype(np.int64)
    bad_t = own.copy()
    bad_t[2] = 1
    ST.check(*ST.run(small, trains, train_off=bad_t), "train_off decreases", failed={1, 2})
    past = own.copy()
    past[4:] = [9, 9]
    ST.check(*ST.run(small, trains, train_off=past), "train_off past the steps", failed={3, 4})
    neg = acc.copy()
    neg[0] = -1
    ST.check(*ST.run(small, trains, acc_off=neg), "a negative accumulator offset", failed={0})
    down = acc.copy()
    down[2] = 5
    ST.check(*ST.run(small, trains, acc_off=down), "acc_off decreases", failed={1, 2})
    ST.check(*ST.run(small, trains, n_acc=int(acc[-1]) - 1), "a region past n_acc", failed={4})
    short = acc.copy()
    short[4:] -= 1
    ST.check(*ST.run(small, trains, acc_off=short), "a region one rename too small", failed={3})


def test_grid_cap_one(small):
    big = with_renames(base(0, shuffle=True), 2100, others=50)
    big.n_sym = WIDE
    parts = [M_log(small, l) for l in range(small.n_logs)] + [big]
    lsoa = logs_soa(parts, WIDE)
    trains = [[2, 3], [6, 7, 2], [9, 7], [], [1, 0], [7, 9, 6], [2, 4, 5], [6, 6], [3, 6, 7, 2, 9]]
    raws = {}
    for cap in (0, 1):
        db, raws[cap] = ST.run(lsoa, trains, grid_cap=cap)
        ST.check(db, raws[cap], f"grid_cap {cap}")
    for name, a in raws[0].items():
        assert a.tobytes() == raws[1][name].tobytes(), f"grid_cap 1: {name} differs from grid_cap 0"


def M_log(lsoa, l):
    """Log l of a LogsSoA as a one-branch SoA."""
    from semantic_merge_amd.marshal import SoA
    a, b = int(lsoa.log_off[l]), int(lsoa.log_off[l + 1])
    return SoA(b - a, 0, *[np.asarray(getattr(lsoa, c))[a:b].copy() for c in ST.COLS], lsoa.n_sym)


def test_one_workspace_for_several_calls(small, pool):
    a = DeviceScreenTrains(small, [[2, 3, 4], [6, 7, 2], [7, 6]], fill=ST.FILL)
    b = DeviceScreenTrains(pool, [[0, 1, 2, 3, 4, 5], [8, 9, 10]], fill=ST.FILL)
    pairs = [(6, 7), (2, 3), (7, 7)]
    p = DeviceScreen(small, pairs, fill=_screen.FILL, large=True)
    size = max(x.ws_bytes for x in (a, b, p))
    ws = a.torch.full((size,), 0xA5, dtype=a.torch.uint8, device=a.device)
    for x in (a, b, p):
        x.ws, x.ws_bytes = ws, size
    a.run()
    b.run()
    ST.check(b, b.raw(), "second shape")
    p.run()
    a.run()
    first = a.raw()
    ST.check(a, first, "after smx_screen_ex on the same workspace")
    _screen.check_all(p.results(p.raw()), small, pairs, "smx_screen_ex in between")
    a.run()
    again = a.raw()
    for name in first:
        assert first[name].tobytes() == again[name].tobytes(), name


# -- the public call -----------------------------------------------------------------------------

def _positions(logs, conflicts):
    """((log, index), (log, index)) of every conflict's two ops, by op id (unique in `logs`)."""
    at = {o.id: (l, i) for l, log in enumerate(logs) for i, o in enumerate(log)}
    assert len(at) == sum(len(x) for x in logs)
    return [(at[c.opA["id"]], at[c.opB["id"]]) for c in conflicts]


def test_screen_train_public():
    from semantic_merge_amd import compose_train, screen_train
    import _train
    cases = load("train_cases.json")
    pick = next(c for c in cases if any(c["steps"]) and len({s[0] for log in c["logs"] for s in log}) ==
                sum(len(log) for log in c["logs"]))
    logs = [to_ops(x) for x in _train.golden_case(pick)["logs"]]

    def lift(n, seed):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 30, seed, **ADV)))

    synthetic = [to_ops(lift(120, 1)[0])] + [to_ops(lift(n, 10 + n)[1]) for n in (40, 150, 80)] + [[]]
    for ops, trains in ((logs, [pick["train"]]), (synthetic, [[0, 1, 2, 3, 4], [3, 2, 1, 0], [4, 2, 2]])):
        before = copy.deepcopy(ops)
        got = screen_train(ops, trains)
        want = [[_positions(ops, step) for step in steps] for _, steps in compose_train(ops, trains)]
        assert got == want
        assert any(any(step for step in tr) for tr in got)
        assert ops == before
    assert screen_train(synthetic) == screen_train(synthetic, [list(range(5))])
    with pytest.raises(IndexError):
        screen_train(synthetic, [[0, 5]])
    assert screen_train(synthetic, []) == []
