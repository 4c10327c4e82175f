"""GPU parity of the batched compose of pairs of logs stored once (smx_compose_pairs,
csrc/smx_batch.h): every pair equal to the CPU oracle on that pair alone, bit-equal to
smx_compose_batch on the repeated layout and to smx_compose_batch_shared when all pairs share a
log; the size classes' edges, degenerate shapes, LDS reuse, failed pairs between valid ones,
conflict capacities, the session and the drop-in compose_pairs.  Every output word starts as a
canary, so the words a call must not write are checked."""
import copy

import numpy as np
import pytest

from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import DeviceBatch, DeviceBatchShared, SmxError, compose_pairs_soa, compose_soa_many, session
from semantic_merge_amd._session import ComposeSession
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, SharedSoA

from _batch import ADV, branch, own_logs
from _pairs import COLS, FILL, check, gap_log, logs_soa, ref, run, same_bytes
from _shapes import pick
from _util import _eq_soa as _eq, jline, to_ops

pytestmark = pytest.mark.gpu

LARGE = _abi.BATCH_LARGE


def empty_log(like):
    return pick(like, np.zeros(like.n_a, bool), np.zeros(like.n_b, bool))


@pytest.fixture(scope="module")
def mixed():
    """14 logs of 0-200 ops (an adversarial mix with divergent renames, None-valued moves, a
    shuffled log, dense ties; an empty log and a one-op log among them) and 60 pairs: all i < j
    of the first 9, reversed pairs, self pairs, a pair listed twice, pairs with the later logs."""
    n_sym = 24
    sizes = np.random.default_rng(7).integers(10, 201, 12).tolist()
    logs = own_logs(n_sym, 100, sizes[:6]) + [branch(n, n_sym, 40 + n, 0, **ADV) for n in sizes[6:]]
    logs += [empty_log(logs[0]), branch(1, n_sym, 3, 1)]
    lsoa = logs_soa(logs, n_sym)
    pairs = [(i, j) for i in range(9) for j in range(i + 1, 9)]
    pairs += [(j, i) for i, j in pairs[:10]] + [(3, 3), (12, 12), (13, 13), (0, 0)] + [pairs[5], pairs[5]]
    pairs += [(12, 4), (4, 12), (13, 12), (12, 13), (13, 9), (10, 13), (11, 10), (9, 11)]
    assert len(pairs) == 60
    assert any(len(ref(lsoa, i, j)[4]) for i, j in pairs)
    return lsoa, pairs


def test_parity_with_oracle_and_repeated_layout(mixed):
    lsoa, pairs = mixed
    db, raw, res = run(lsoa, pairs)
    check(db, raw, "mixed")
    assert any(len(r[4]) for r in res)
    rep = DeviceBatch([lsoa.pair(i, j) for i, j in pairs], n_sym=lsoa.n_sym, fill=FILL)
    rep.run()
    same_bytes(res, rep.results(), "smx_compose_pairs vs smx_compose_batch on the repeated layout")
    # (i, j) and (j, i) differ: the conflict pairs are (A index, B index)
    assert [pairs[36 + p] for p in range(10)] == [(j, i) for i, j in pairs[:10]]
    assert any(len(res[p][4]) and not np.array_equal(res[p][4], res[36 + p][4]) for p in range(10))


def test_more_pairs_than_one_classify_workgroup(mixed):
    """300 pairs: the pre-pass classifies 256 pairs per workgroup, so two workgroups append to the
    same class lists, the second one partly filled."""
    lsoa, _ = mixed
    L = lsoa.n_logs
    every = [(i, j) for i in range(L) for j in range(L)]
    pairs = every + every[:300 - len(every)]
    assert len(every) == 196 and len(pairs) == 300
    db, raw, res = run(lsoa, pairs)
    check(db, raw, "300 pairs")
    same_bytes(res[:104], res[196:], "the pairs listed twice")
    check(*run(lsoa, pairs, grid_cap=1)[:2], "300 pairs, one workgroup per class")


@pytest.mark.parametrize("is_b", [False, True])
def test_equal_to_the_shared_form_when_all_pairs_share_log_0(mixed, is_b):
    lsoa, _ = mixed
    L = lsoa.n_logs
    pairs = [(m, 0) if is_b else (0, m) for m in range(1, L)]
    db, raw, res = run(lsoa, pairs)
    check(db, raw, f"log 0 on side {'B' if is_b else 'A'}")
    ssoa = SharedSoA(int(lsoa.log_off[1]), lsoa.log_off[1:].copy(), *[getattr(lsoa, c) for c in COLS], lsoa.n_sym, [],
                     TS_ISO, ID_UUID)
    sh = DeviceBatchShared(ssoa, shared_is_b=is_b, fill=FILL)
    sh.run()
    same_bytes(res, sh.results(), "smx_compose_pairs vs smx_compose_batch_shared")


def test_class_edges():
    n_sym = 40
    totals = [c + d for c in _abi.BATCH_CLASSES for d in (-1, 0, 1)]
    assert totals == [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]
    a = branch(100, n_sym, 6, 0, mix=synth.ADVERSARIAL_MIX)
    logs = [a, empty_log(a), branch(1, n_sym, 8, 1), branch(1, n_sym, 9, 0)]
    logs += [branch(t - 100, n_sym, 200 + t, 1, mix=synth.ADVERSARIAL_MIX) for t in totals]
    lsoa = logs_soa(logs, n_sym)
    pairs = [(1, 1), (1, 2), (2, 1), (2, 3)] + [(0, 4 + k) if k % 2 else (4 + k, 0) for k in range(len(totals))]
    lens = np.diff(lsoa.log_off)
    assert [int(lens[i] + lens[j]) for i, j in pairs] == [0, 1, 1, 2] + totals
    db, raw, res = run(lsoa, pairs)
    check(db, raw, "edges, flags 0", sent_back=(len(pairs) - 1,))
    assert raw["counts"][:6].tolist() == [0, 0, 1, 0, 1, 0] and int(raw["counts"][6] + 2 * raw["counts"][7]) == 2
    db, raw, large = run(lsoa, pairs, flags=LARGE)
    check(db, raw, "edges, SMX_BATCH_LARGE")
    assert (raw["counts"] != -2).all() and len(large[-1][0]) > 0
    same_bytes(res[:-1], large[:-1], "flags 0 vs SMX_BATCH_LARGE")


def test_degenerate_shapes():
    n_sym = 12
    big = own_logs(n_sym, 300, [90, 40, 130, 77])
    empty, one = empty_log(big[0]), branch(1, n_sym, 4, 1)
    # (gaps of invalid entries before, between and after the logs: logs 0, 3 and 8, which no pair holds)
    logs = [gap_log(37), big[0], empty, gap_log(5), big[1], one, big[2], big[3], gap_log(300)]
    lsoa = logs_soa(logs, n_sym)
    pairs = [(2, 1), (1, 2), (2, 2),           # an empty log as A, as B, as both
             (5, 4), (4, 5), (5, 5), (5, 2),   # a one-op log
             (6, 6), (1, 1),                   # self pairs
             (4, 7), (7, 4),                   # (i, j) together with (j, i)
             (6, 1), (6, 1),                   # a pair listed twice
             (7, 1), (6, 4)]                   # log b stored before log a
    db, raw, res = run(lsoa, pairs)
    check(db, raw, "degenerate")
    assert raw["counts"][4:6].tolist() == [0, 0]
    same_bytes([res[11]], [res[12]], "the same pair listed twice")
    assert np.array_equal(np.sort(res[0][0]), np.arange(90))  # the empty log composed with log 1
    # a self pair has conflicts only if the log conflicts with itself; its order holds every kept op of both copies
    k = int(raw["counts"][2 * 7])
    assert k == 2 * 130 - 2 * int(raw["counts"][2 * 7 + 1])
    check(*run(lsoa, pairs, grid_cap=1)[:2], "degenerate, one workgroup")
    for got, (i, j) in zip(compose_pairs_soa(lsoa, pairs), pairs):
        _eq(got, ref(lsoa, i, j), f"session: pair ({i}, {j})")
    assert compose_pairs_soa(lsoa, []) == []


def test_lds_reuse_one_and_two_workgroups(mixed):
    lsoa, pairs = mixed
    raws = {}
    for cap in (0, 1, 2):  # one workgroup runs many pairs of different sizes one after another
        db, raws[cap], _ = run(lsoa, pairs, grid_cap=cap)
        check(db, raws[cap], f"grid_cap {cap}")
    for cap in (1, 2):
        for name, a in raws[0].items():
            assert a.tobytes() == raws[cap][name].tobytes(), f"grid_cap {cap}: {name} differs from grid_cap 0"


@pytest.fixture(scope="module")
def six():
    n_sym = 8
    logs = own_logs(n_sym, 400, [100, 60, 300, 150, 1000, 80])
    logs[0] = branch(120, n_sym, 8, 0, **ADV)
    pairs = [(0, 1), (2, 3), (0, 4), (5, 0), (3, 1), (4, 5), (0, 2), (2, 2)]
    return logs, n_sym, pairs


def test_failed_pairs_do_not_touch_their_neighbours(six):
    logs, n_sym, pairs = six
    good = logs_soa(logs, n_sym)
    L = good.n_logs
    # a pair index outside [0, n_logs), on either side
    odd = pairs[:2] + [(-1, 1), (2, L)] + pairs[2:4] + [(L, -1)] + pairs[4:]
    db, raw, _ = run(good, odd)
    check(db, raw, "pair indices -1 and n_logs", failed=(2, 3, 6))
    # an op with kind = 18 in log 3, one with sym = n_sym in log 5: every pair that holds them, and only those
    bad = logs_soa([copy.deepcopy(x) for x in logs], n_sym)
    bad.kind[int(bad.log_off[3]) + 149] = 18
    bad.sym[int(bad.log_off[5])] = n_sym
    db, raw, _ = run(bad, pairs)
    check(db, raw, "kind = 18, sym = n_sym", failed=[p for p, (i, j) in enumerate(pairs) if {i, j} & {3, 5}])
    with pytest.raises(SmxError, match="pair 3"):
        compose_pairs_soa(bad, pairs)
    # log_off decreases: log 2 ends 5 ops before it starts, and log 3 starts there, below an earlier offset
    off = good.log_off.copy()
    off[3] = off[2] - 5
    db, raw, _ = run(good, pairs, log_off=off)
    check(db, raw, "a decreasing log_off", failed=[p for p, (i, j) in enumerate(pairs) if {i, j} & {2, 3}])
    # the last log ends past n_total
    db, raw, _ = run(good, pairs, n_total=good.n_total - 1)
    check(db, raw, "log_off[n_logs] > n_total", failed=[p for p, (i, j) in enumerate(pairs) if 5 in (i, j)])
    # res_off: pair 2's region one entry too short (the regions after it start one entry earlier)
    lens = np.diff(good.log_off)
    room = np.asarray([lens[i] + lens[j] for i, j in pairs], np.int64)
    short = room.copy()
    short[2] -= 1
    db, raw, _ = run(good, pairs, res_off=np.concatenate([[0], np.cumsum(short)]))
    check(db, raw, "res_off one entry too short", failed=(2,))
    # res_off[4] below res_off[3]: pair 3 ends before it starts, pair 4 starts below an earlier entry
    # (its own region, up to res_off[5], has all the room it needs)
    res_off = np.concatenate([[0], np.cumsum(room)])
    low = res_off.copy()
    low[4] = low[3] - 1
    db, raw, _ = run(good, pairs, res_off=low)
    check(db, raw, "res_off below an earlier entry", failed=(3, 4))
    # res_off[n_pairs] > n_out
    db, raw, _ = run(good, pairs, n_out=int(res_off[-1]) - 1)
    check(db, raw, "res_off[n_pairs] > n_out", failed=(len(pairs) - 1,))
    # conf_off decreases at pair 1 (pair 2's region then starts 3 pairs earlier: pair 0 has 3 to spare)
    caps = [int(min(lens[i], lens[j])) for i, j in pairs]
    caps[0] += 3
    caps[1] = -3
    db, raw, _ = run(good, pairs, conflict_caps=caps)
    check(db, raw, "a decreasing conf_off", failed=(1,))
    # a negative conf_off
    caps = [int(min(lens[i], lens[j])) for i, j in pairs]
    db = run(good, pairs, conflict_caps=caps)[0]
    db._idx[4][0] = -1  # (the device's conf_off[0])
    for name in db._OUT:
        getattr(db, name).fill_(FILL)
    db.run()
    raw = db.raw()
    assert raw["counts"][:2].tolist() == [-1, -1]
    assert (raw["counts"][2:] >= 0).all()


def test_conflict_truncation():
    n_sym = 6
    logs = [branch(150, n_sym, 9, 0, **ADV)] + [branch(n, n_sym, 51 + n, 1, **ADV) for n in (120, 60)]
    lsoa = logs_soa(logs, n_sym)
    pairs = [(0, 1), (0, 2), (1, 0)]
    n_conf = len(ref(lsoa, 0, 1)[4])
    assert n_conf > 1 and len(ref(lsoa, 0, 2)[4]) > 0
    for cap in (0, n_conf - 1):
        db, raw, res = run(lsoa, pairs, conflict_caps=[cap, 60, 120])
        check(db, raw, f"capacity {cap}", truncated=(0,))
        assert raw["counts"][:2].tolist() == [len(ref(lsoa, 0, 1)[0]), n_conf]  # the full count, the ops complete
        assert len(res[0][4]) == cap


def test_session_routes_and_counts_bytes():
    n_sym = 30
    logs = own_logs(n_sym, 700, [300, 40, 150, 1900, 90])  # 300 + 1900 and 150 + 1900 ops: over 2048
    lsoa = logs_soa(logs + [empty_log(logs[0])], n_sym)
    pairs = [(0, 1), (0, 3), (2, 4), (3, 2), (5, 0), (1, 1), (4, 3)]
    lens = np.diff(lsoa.log_off)
    over = [p for p, (i, j) in enumerate(pairs) if lens[i] + lens[j] > _abi.BATCH_MAX_OPS]
    assert over == [1, 3]
    for kw, routed, large in ((dict(), 2, 0), (dict(large=True, large_max=2048), 2, 0), (dict(large=True), 0, 2)):
        got = compose_pairs_soa(lsoa, pairs, **kw)
        last = session().last
        for (i, j), g in zip(pairs, got):
            _eq(g, ref(lsoa, i, j), f"compose_pairs_soa({kw}): pair ({i}, {j})")
        assert set(last) == {"pack_s", "device_s", "unpack_s", "in_bytes", "large", "routed"}
        assert (last["routed"], last["large"]) == (routed, large), kw
        assert last["pack_s"] > 0 and last["device_s"] > 0 and last["unpack_s"] > 0
    # bytes in: every log once and the index arrays, against every pair's two logs in the repeated layout
    L, P, tot = lsoa.n_logs, len(pairs), int(lsoa.n_total)
    index = 8 * (L + 1) + 2 * 4 * P + 2 * 8 * (P + 1)
    assert last["in_bytes"] == ComposeSession._pairs_layout(tot, L, P)["in_bytes"]
    assert 37 * tot + index <= last["in_bytes"] <= 37 * tot + index + 12 * 255  # (12 segments, each 256-aligned)
    ns = [int(lens[i] + lens[j]) for i, j in pairs]
    rep = ComposeSession._batch_layout(ns)["in_bytes"]
    index_rep = 8 * (P + 1) + 8 * P + 8 * (P + 1)
    assert 37 * sum(ns) + index_rep <= rep <= 37 * sum(ns) + index_rep + 10 * 255
    assert sum(ns) > 2 * tot and last["in_bytes"] < rep
    assert abs((rep - last["in_bytes"]) - (37 * (sum(ns) - tot) + index_rep - index)) <= 12 * 255
    same_bytes(compose_pairs_soa(lsoa, pairs, large=True), compose_soa_many([lsoa.pair(i, j) for i, j in pairs], large=True),
               "compose_pairs_soa vs compose_soa_many on the repeated layout")
    with pytest.raises(SmxError, match="pair 1"):
        compose_pairs_soa(lsoa, [(0, 1), (0, 6)])


def test_dropin_compose_pairs():
    from semantic_merge_amd import compose_pairs
    from semantic_merge_amd.compose import compose_oplogs

    def dicts(n, seed):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 30, seed, **ADV)))

    logs = [to_ops(dicts(300, 1)[0])] + [to_ops(dicts(n, 10 + n)[1]) for n in (40, 150, 1900, 90)]  # 300 + 1900: over 2048
    logs.insert(2, [])
    assert compose_pairs([], None) == [] and compose_pairs(logs, []) == []
    listed = [(0, 1), (4, 0), (2, 3), (3, 3), (5, 1), (1, 5), (0, 1), (2, 2)]
    for pairs, large in ((None, False), (listed, False), (listed, True)):
        before = copy.deepcopy(logs)
        ids = [id(o) for x in logs for o in x]
        got = compose_pairs(logs, pairs, large=large)
        ij = [(i, j) for i in range(len(logs)) for j in range(i + 1, len(logs))] if pairs is None else pairs
        assert len(got) == len(ij)
        for (i, j), (go, gc) in zip(ij, got):
            wo, wc = compose_oplogs(logs[i], logs[j])
            assert jline([o.to_dict() for o in go]) == jline([o.to_dict() for o in wo]), f"pair ({i}, {j}): ops"
            assert jline([c.to_dict() for c in gc]) == jline([c.to_dict() for c in wc]), f"pair ({i}, {j}): conflicts"
        assert any(gc for _, gc in got)
        assert logs == before
        assert ids == [id(o) for x in logs for o in x]
    for bad in ((0, 6), (-1, 0), (6, 6)):
        with pytest.raises(IndexError):
            compose_pairs(logs, [(0, 1), bad])
