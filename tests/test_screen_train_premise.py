"""The premise of smx_screen_train on the CPU, independently of the device: as far as conflicts
go, a train's accumulator is its landed logs' renames in (ts, oid_hi, oid_lo) order, a step is the
reference's two-head walk of that list against the log's stably sorted renames, and a step that
lands is a stable merge of the two, A first on equal keys.  That rename-only train
(tests/_screen_train.py rename_train) equals the full loop over oracle.compose with the re-log
rule of include/smx.h and no limit on ops (full_train) in every step's outcome and (A column,
B column) pairs: on every golden train, and on seeded random trains of synthetic logs, trains of
more than 2048 ops among them."""
import numpy as np
import pytest

from semantic_merge_amd import marshal as M
from semantic_merge_amd._abi import BATCH_MAX_OPS

import _screen_train as ST
import _train
from _batch import ADV, branch, own_logs
from _pairs import logs_soa
from _util import load, to_ops


def test_golden_trains():
    cases = [_train.golden_case(c) for c in load("train_cases.json")]
    assert len(cases) >= 100
    evicted = 0
    for c, case in enumerate(cases):
        lsoa = M.marshal_logs([to_ops(x) for x in case["logs"]])
        full = ST.full_train(lsoa, case["train"])
        ST.same(ST.rename_train(lsoa, case["train"]), full, f"case {c}")
        # and both are the reference's: which steps landed, and how many conflicts each other had
        assert [len(s) for s in case["steps"]] == [oc for _, oc, _ in full[2]], f"case {c}"
        evicted += sum(1 for _, oc, _ in full[2] if oc > 0)
    assert evicted >= 50


N_SYM = 48


@pytest.fixture(scope="module")
def pool():
    """Logs of 10 to 1500 ops: adversarial mixes with divergent renames, None-valued moves, a
    shuffled log, dense ties; two of them hold one log's ops again (equal full keys)."""
    sizes = [10, 25, 40, 60, 90, 120, 300, 700, 1500, 33, 77, 150]
    logs = own_logs(N_SYM, 200, sizes) + [branch(n, N_SYM, 300 + n, n & 1, **ADV) for n in (50, 400, 1200)]
    return logs_soa(logs, N_SYM)


def test_random_trains(pool):
    rng = np.random.default_rng(17)
    lens = np.diff(pool.log_off)
    seen = dict.fromkeys(("over the limit", "evicted then lands", "a log twice"), 0)
    for k in range(40):
        train = rng.choice(pool.n_logs, rng.integers(1, 9)).tolist()
        if k % 5 == 0:
            train = rng.permutation(pool.n_logs).tolist()      # every log: 4755 ops
        full = ST.full_train(pool, train)
        ST.same(ST.rename_train(pool, train), full, f"train {k} {train}")
        outcome = [oc for _, oc, _ in full[2]]
        assert min(outcome) >= 0
        before = np.concatenate([[0], np.cumsum([lens[l] if oc == 0 else 0 for l, oc in zip(train, outcome)])])[:-1]
        seen["over the limit"] += int(any(n + lens[l] > BATCH_MAX_OPS for n, l in zip(before, train)))
        seen["evicted then lands"] += int(any(oc > 0 and 0 in outcome[s + 1:] for s, oc in enumerate(outcome)))
        seen["a log twice"] += int(len(set(train)) < len(train))
    assert all(seen.values()), seen


def test_invalid_logs_in_both_oracles(pool):
    import copy
    bad = copy.deepcopy(pool)
    bad.kind[int(bad.log_off[3]) + 5] = 18
    off = np.array(pool.log_off)
    off[6] = off[5] - 1
    train = [0, 3, 1, -1, 2, pool.n_logs, 5, 6, 7]
    for lsoa, kw in ((bad, {}), (pool, dict(log_off=off))):
        full = ST.full_train(lsoa, train, **kw)
        ST.same(ST.rename_train(lsoa, train, **kw), full, "invalid logs")
        assert [oc for _, oc, _ in full[2]].count(-1) >= 3
