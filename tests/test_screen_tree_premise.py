"""The premise of smx_screen_tree without a GPU: the accumulator of smx_screen_train's premise
(a sorted list of renames; tests/_screen_train.rename_train) carried from parent to child over a
tree gives, at every node, what rename_train and full_train give on the node's whole root path;
a node that does not land, or whose log has no renames, leaves its parent's list as it is; and the
regions the host lays out by the room rule are never below the accumulator that arises."""
import numpy as np
import pytest

from semantic_merge_amd import marshal as M

import _screen_train as ST
import _screen_tree as T
import _train
import _tree
from _util import load


@pytest.fixture(scope="module")
def pool():
    return T.make_pool()


def check_tree(lsoa, nodes, label, full=True):
    parents, logs, _, _ = T.level_tree(nodes)
    got = T.carry(lsoa, parents, logs)
    acc_off = T.host_acc_off(lsoa, parents, logs)
    seen = dict.fromkeys(("conflict", "lands below a conflict", "no renames", "own list"), 0)
    for n, (step, acc, holder) in enumerate(got):
        path = T.root_path(parents, logs, n)
        want = ST.ref(lsoa, path, full=False)[2][-1]
        assert step[:2] == want[:2] and np.array_equal(step[2], want[2]), f"{label}: node {n}: rename_train differs"
        if full:
            want = ST.ref(lsoa, path)[2][-1]
            assert step[:2] == want[:2] and np.array_equal(step[2], want[2]), f"{label}: node {n}: full_train differs"
        p = int(parents[n])
        before, held = (got[p][1], got[p][2]) if p >= 0 else (None, T.NONE)
        l = int(logs[n])
        has = 0 <= l < lsoa.n_logs and bool((np.asarray(lsoa.kind)[int(lsoa.log_off[l]): int(lsoa.log_off[l + 1])]
                                              == T.RENAME).any())
        if step[1] != 0 or not has:
            assert holder == held and (before is None or acc is before), f"{label}: node {n} made a list of its own"
            seen["conflict"] += step[1] > 0
            seen["no renames"] += step[1] == 0
        else:
            assert holder == n and len(acc) == step[0]
            assert len(acc) <= acc_off[n + 1] - acc_off[n], f"{label}: node {n}: {len(acc)} renames, room {acc_off[n + 1] - acc_off[n]}"
            seen["own list"] += 1
            up = p
            while up >= 0 and got[up][0][1] <= 0:
                up = int(parents[up])
            seen["lands below a conflict"] += up >= 0
        if holder != n:
            assert acc_off[n + 1] == acc_off[n] or has, f"{label}: node {n}: room for a log without renames"
    return seen


@pytest.mark.parametrize("seed", T.SEEDS)
def test_random_trees(pool, seed):
    seen = check_tree(pool, _tree.random_nodes(seed, logs=T.SMALL), f"seed {seed}")
    assert all(seen.values()), seen


def test_shapes_of_the_pool(pool):
    nodes = T.named([(None, "free6"), (0, "r5"), (1, "free1"), (2, "r5b"), (1, "r5c"), (4, "r5d"), (1, "bad18"),
                     (6, "r5b"), (1, "r5"), (8, "r5b"), (None, "eqA"), (10, "eqA"), (11, "eqC"), (10, "eqB"),
                     (13, "eqC"), (None, "d64a"), (15, "d64b"), (15, "d65"), (16, "hit64"), (17, "hit64"),
                     (None, 99), (20, "o10"), (4, "d64a"), (22, "r5d")])
    seen = check_tree(pool, nodes, "pool shapes")
    assert all(seen.values()), seen


def test_golden_trains_joined():
    cases = [_train.golden_case(c) for c in load("train_cases.json")]
    total = dict.fromkeys(("conflict", "lands below a conflict", "no renames", "own list"), 0)
    for g0 in range(0, len(cases), 30):
        logs, nodes, ends, _ = T.joined(cases[g0: g0 + 30])
        assert sum(len(e) for e in ends) > len({n for e in ends for n in e}) or g0, "no shared prefix"
        seen = check_tree(M.marshal_logs(logs), nodes, f"group {g0}", full=False)
        for k, v in seen.items():
            total[k] += v
    assert all(total.values()), total
