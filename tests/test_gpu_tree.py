"""GPU parity of smx_compose_tree (csrc/smx_tree.h) with the oracle of tests/_tree.py, exactly:
every node's length, outcome, conflict records, node_acc and the accumulator read through it
equal `_train.run_train` on the node's root path.  Every output word starts as a canary, so the
words a call must not write are checked.  Shapes: random trees with conflicting nodes above
landed ones; a star, a path, a binary tree, a log twice on a path and in many nodes; the 2048
limit with a node that goes on from its grandparent; one level over all three size classes;
empty logs; step failures that let the children go on; structural failures that fail a subtree
and nothing else; truncated conflict capacities; one workgroup per launch; one workspace for
different trees and for smx_compose_train; and bit-equality with smx_compose_train on the same
paths."""
import dataclasses

import numpy as np
import pytest

from semantic_merge_amd._lib import DeviceTrains, DeviceTree

import _train
import _tree
from _batch import MOVE
from _tree import FILL, IX, NAMES, NONE, SEEDS, named, random_nodes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    return _tree.make_pool()


def outcomes(pool, db, **kw):
    return [_tree.node_ref(pool, db.parents, db.node_log, n, **kw)[4][1] for n in range(db.n_nodes)]


def conflict_above_landed(pool, db, **kw):
    oc = outcomes(pool, db, **kw)
    for n in range(db.n_nodes):
        up = int(db.parents[n])
        while up >= 0 and oc[n] == 0 and db.node_len[n] > 0:
            if oc[up] > 0:
                return True
            up = int(db.parents[up])
    return False


@pytest.mark.parametrize("seed", SEEDS)
def test_random_trees(pool, seed):
    nodes = random_nodes(seed)
    db, raw = _tree.run(pool, nodes)
    assert db.n_levels <= 6 and conflict_above_landed(pool, db), "the seed shows no conflicting node above a landed one"
    res = _tree.check(db, raw, f"random tree {seed}")
    # some node's accumulator is an ancestor's, and some entry carries an addr / file / ctx
    assert any(r[4] not in (n, NONE) for n, r in enumerate(res))
    for f in (1, 2, 3):
        assert any((r[f] != NONE).any() for r in res)


def test_empty_file_rule(pool):
    """empty_str names an id that moves carry as their file: where a move has gathered it, its v1
    is v1_alt's entry instead (test_gpu_train.py's recipe)."""
    mv = np.flatnonzero((np.asarray(pool.kind) == MOVE) & (np.asarray(pool.v1) >= 0))
    ids = np.unique(np.asarray(pool.v1)[mv])
    empty = int(ids[0])
    v1 = np.array(pool.v1)
    v1[mv[::2]] = empty
    pool = dataclasses.replace(pool, v1=v1)
    alt = np.random.default_rng(3).choice(np.concatenate([ids[1:], [-1]]), pool.n_total).astype(np.int32)
    nodes = named([(None, "o10"), (0, "o25"), (1, "o40"), (2, "o60"), (3, "o90"), (4, "o120"), (None, "o120"), (6, "o90"),
                   (7, "a30"), (8, "o60"), (9, "o25"), (1, "o25"), (11, "o40"), (3, "a30")])
    kw = dict(v1_alt=alt, empty_str=empty)
    db, raw = _tree.run(pool, nodes, **kw)
    plain = [_tree.node_ref(pool, db.parents, db.node_log, n)[2] for n in range(db.n_nodes)]
    ruled = [_tree.node_ref(pool, db.parents, db.node_log, n, **kw)[2] for n in range(db.n_nodes)]
    assert any(not np.array_equal(p, r) for p, r in zip(plain, ruled)), "the rule changes nothing here"
    _tree.check(db, raw, "empty file", **kw)


def test_star_path_and_binary_tree(pool):
    star = named([(None, n) for n in NAMES[:10]])
    db, raw = _tree.run(pool, star)
    assert db.n_levels == 1
    _tree.check(db, raw, "star")
    names = ("o10", "o25", "a30", "o40", "c9", "o60", "a50", "o90", "c8", "o120", "one", "c128a")
    path = named([(i - 1 if i else None, n) for i, n in enumerate(names)])
    db, raw = _tree.run(pool, path)
    assert db.n_levels == 12 and db.n_nodes == 12
    res = _tree.check(db, raw, "path of 12 levels")
    assert any(r[6] > 0 for r in res) and res[11][6] == 0
    rng = np.random.default_rng(5)
    binary = [((i - 1) // 2 if i else None, int(rng.choice(_tree.SMALL[2:]))) for i in range(15)]
    db, raw = _tree.run(pool, binary)
    assert db.level_off.tolist() == [0, 1, 3, 7, 15]
    _tree.check(db, raw, "complete binary tree")


def test_a_log_twice_on_a_path_and_in_many_nodes(pool):
    nodes = named([(None, "o60"), (0, "o60"), (1, "c9"), (None, "a50"), (3, "a50"), (4, "o25"), (2, "o60")])
    nodes += named([(i % 7, "o40") for i in range(20)])
    db, raw = _tree.run(pool, nodes)
    _tree.check(db, raw, "a log twice on a path, a log in 20 nodes")


def test_the_2048_limit(pool):
    nodes = named([(None, "c1024"), (0, "c1016"), (1, "c8"), (1, "c9"), (3, "one"), (3, "c8"), (2, "one")])
    db, raw = _tree.run(pool, nodes)
    res = _tree.check(db, raw, "2048 and 2049")
    par, logs, _, order = _tree.level_tree(nodes)
    at = {int(n): i for i, n in enumerate(order)}
    assert res[at[2]][5:7] == (2048, 0) and res[at[3]][5:7] == (2040, -2)
    # the child of the -2 node goes on from the grandparent's accumulator, and lands there
    assert res[at[4]][4] == at[4] and res[at[4]][5:7] == (2041, 0) and int(raw["node_acc"][at[3]]) == at[1]
    assert res[at[5]][5:7] == (2048, 0) and res[at[6]][5:7] == (2048, -2) and res[at[6]][4] == at[2]


def test_one_level_over_all_classes(pool):
    nodes = named([(None, "c128a"), (None, "c512a"), (None, "o10"), (0, "c128b"), (0, "c129"), (1, "c512b"), (1, "c513"),
                   (2, "o25"), (1, "c1024"), (0, "empty")])
    db, raw = _tree.run(pool, nodes)
    res = _tree.check(db, raw, "path sums 256, 257, 1024, 1025")
    assert {256, 257, 1024, 1025, 1536, 128} <= {r[5] for r in res[3:]}
    db1, raw1 = _tree.run(pool, nodes, grid_cap=1)
    _tree.check(db1, raw1, "one workgroup per launch")
    for name in raw:
        assert raw[name].tobytes() == raw1[name].tobytes(), name


def test_grid_cap_one_walks_a_whole_level(pool):
    nodes = random_nodes(SEEDS[0])
    db, raw = _tree.run(pool, nodes)
    db1, raw1 = _tree.run(pool, nodes, grid_cap=1)
    _tree.check(db1, raw1, "grid_cap 1")
    for name in raw:
        assert raw[name].tobytes() == raw1[name].tobytes(), name


def test_empty_logs_and_one_level(pool):
    nodes = named([(None, "empty"), (0, "empty"), (1, "o25"), (2, "empty"), (None, "one"), (4, "empty")])
    db, raw = _tree.run(pool, nodes)
    res = _tree.check(db, raw, "empty logs")
    assert res[0][4:7] == (0, 0, 0), "an empty log lands on an empty accumulator"
    db, raw = _tree.run(pool, named([(None, "empty")]))
    assert db.n_levels == 1
    _tree.check(db, raw, "a single empty root")
    db, raw = _tree.run(pool, named([(None, "o40")]))
    _tree.check(db, raw, "a single root")


def test_step_failures_let_the_children_go_on(pool):
    nodes = named([(None, "o25"), (0, "badkind"), (1, "o40"), (2, "badsym"), (3, "o60"), (4, -1), (5, "o10"),
                   (6, len(NAMES)), (7, "a30"), (None, "badkind"), (9, "o10"), (None, 1 << 20), (11, "one")])
    at = {int(n): i for i, n in enumerate(_tree.level_tree(nodes)[3])}
    db, raw = _tree.run(pool, nodes)
    res = _tree.check(db, raw, "step failures")
    assert [res[at[n]][6] for n in (1, 3, 5, 7, 11)] == [-1] * 5
    assert res[at[9]][4:7] == (NONE, 0, -1) and res[at[10]][6] == 0 and res[at[10]][4] == at[10]
    assert res[at[1]][4] == at[0] and res[at[12]][6] == 0
    # a log whose offsets decrease: invalid under smx_screen's rules, and so is no other
    off = np.array(pool.log_off)
    off[IX["o40"]] = off[IX["o25"]] - 1
    db, raw = _tree.run(pool, nodes, log_off=off)
    res = _tree.check(db, raw, "a log with a decreasing offset", log_off=off)
    assert res[at[2]][6] == -1


def raw_run(pool, parents, logs, level_off, **kw):
    db = DeviceTree(pool, parents, logs, level_off, fill=FILL, **kw)
    db.run()
    return db, db.raw()


# three levels: nodes 0-2, 3-6, 7-9
PARENTS = np.array([-1, -1, -1, 0, 0, 1, 2, 3, 4, 6], np.int32)
LOGS = np.array([IX[n] for n in ("o10", "o25", "a30", "o40", "o25", "o60", "a50", "one", "o10", "c9")], np.int32)
LEVELS = np.array([0, 3, 7, 10], np.int64)


def test_structural_failures_of_parents(pool):
    db, raw = raw_run(pool, PARENTS, LOGS, LEVELS)
    _tree.check(db, raw, "the valid tree")
    for label, node, parent, failed in (("a parent in the node's own level", 4, 3, {4}),
                                        ("a parent two levels up", 8, 1, {8}),
                                        ("a parent in a later level", 3, 7, {3}),
                                        ("a level-0 node with a parent", 1, 0, {1}),
                                        ("a parent outside the nodes", 5, 10, {5}),
                                        ("a parent below SMX_NONE", 6, -2, {6}),
                                        ("no parent below level 0", 4, -1, {4})):
        par = PARENTS.copy()
        par[node] = parent
        db, raw = raw_run(pool, par, LOGS, LEVELS)
        # (the failed node's children fail with it: check() adds them)
        kept = PARENTS.copy()
        db.parents = kept  # the oracle's paths follow the valid tree
        _tree.check(db, raw, label, failed=failed)


def test_structural_failures_of_level_off(pool):
    for label, levels, failed in (("level_off decreases", [0, 7, 3, 10], set(range(3, 10))),
                                  ("a negative level_off", [-1, 3, 7, 10], set(range(10))),
                                  ("level_off[0] is not 0", [1, 3, 7, 10], set(range(10))),
                                  ("level_off past n_nodes", [0, 3, 7, 11], {7, 8, 9}),
                                  ("level_off ends before n_nodes", [0, 3, 7, 9], {7, 8, 9}),
                                  ("a level past the nodes in the middle", [0, 3, 11, 10], set(range(3, 10)))):
        db, raw = raw_run(pool, PARENTS, LOGS, np.array(levels, np.int64))
        _tree.check(db, raw, label, failed=failed)
    # fewer levels than the tree has: the nodes behind the last level's end fail
    db, raw = raw_run(pool, PARENTS, LOGS, LEVELS, n_levels=2)
    _tree.check(db, raw, "n_levels short of the nodes", failed=set(range(3, 10)))


def test_structural_failures_of_res_off(pool):
    db, _ = raw_run(pool, PARENTS, LOGS, LEVELS)
    res_off = db.res_off
    need = np.diff(res_off)
    short = res_off.copy()
    short[4:] -= 1
    db, raw = raw_run(pool, PARENTS, LOGS, LEVELS, res_off=short)
    _tree.check(db, raw, "a region one entry short", failed={3})
    assert int(raw["node_counts"][2 * 7]) == -1, "the short node's child fails with it"
    neg = res_off.copy()
    neg[0] = -1
    db, raw = raw_run(pool, PARENTS, LOGS, LEVELS, res_off=neg)
    _tree.check(db, raw, "a negative result offset", failed={0})
    dec = res_off.copy()
    dec[2] = dec[1] - 1
    db, raw = raw_run(pool, PARENTS, LOGS, LEVELS, res_off=dec)
    _tree.check(db, raw, "a result offset below an earlier one", failed={1, 2})
    db, raw = raw_run(pool, PARENTS, LOGS, LEVELS, n_out=int(res_off[-1]) - 1)
    _tree.check(db, raw, "a region past n_out", failed={9})
    # the path sum counts valid logs only, and a node needs min(2048, path sum) and no more
    nodes = named([(None, "c1024"), (0, "c1016"), (1, "c513"), (0, "badkind"), (0, len(NAMES))])
    par, logs, levels, _ = _tree.level_tree(nodes)
    lens = np.diff(pool.log_off)
    # (level order: the root, its three children, then c513)
    exact = np.concatenate([[0], np.cumsum([1024, 2040, 1024 + lens[IX["badkind"]], 1024, 2048])]).astype(np.int64)
    db, raw = raw_run(pool, par, logs, levels, res_off=exact)
    _tree.check(db, raw, "regions of exactly min(2048, path sum)")


def conflicting_path(pool):
    """A path whose last node conflicts, and that holds a node of several conflicts before it."""
    names = ["o10", "o25", "o40", "o60", "o90", "o120", "a30", "a50", "o25", "o60"]
    w = _train.ref(pool, [IX[n] for n in names])
    hits = [s for s, (_, oc, _) in enumerate(w[5]) if oc > 0]
    assert len(hits) >= 2 and any(w[5][s][1] > 1 for s in hits), "the path has no step of several conflicts"
    return named([(i - 1 if i else None, n) for i, n in enumerate(names[:hits[-1] + 1])]), hits


def test_truncated_conflict_capacity(pool):
    nodes, hits = conflicting_path(pool)
    db, _ = _tree.run(pool, nodes)
    oc = outcomes(pool, db)
    for cap in (0, 1):
        db, raw = _tree.run(pool, nodes, conflict_caps=[cap] * len(nodes))
        _tree.check(db, raw, f"capacity {cap}", truncated=[n for n, o in enumerate(oc) if o > cap])
    db, raw = _tree.run(pool, nodes, conflict_caps=[max(o, 0) for o in oc])
    _tree.check(db, raw, "the exact capacities")
    caps = [max(o, 0) for o in oc]
    caps[-1] = -2  # conf_off decreases at the last node: it gets no record
    db, raw = _tree.run(pool, nodes, conflict_caps=caps)
    _tree.check(db, raw, "a decreasing conf_off", truncated=[len(nodes) - 1])


def test_one_workspace_for_two_trees_and_a_train_call(pool):
    first = random_nodes(SEEDS[1])
    second = named([(None, "c1024"), (0, "c512a"), (1, "c512b"), (None, "a30"), (3, "o60"), (4, "a50")])
    p1, l1, v1, _ = _tree.level_tree(first)
    p2, l2, v2, _ = _tree.level_tree(second)
    tr = DeviceTrains(pool, [[IX["c1024"], IX["c512a"], IX["c512b"]], [IX["a30"], IX["o60"], IX["a50"]]], fill=_train.FILL)
    big = DeviceTree(pool, p2, l2, v2, fill=FILL)
    assert big.ws_bytes >= tr.ws_bytes, "the train call fits the tree's workspace"
    a = DeviceTree(pool, p1, l1, v1, fill=FILL, share=big)
    tr.ws, tr.ws_bytes = big.ws, big.ws_bytes
    big.ws.fill_(0xA5)
    a.run()
    tr.run()
    big.run()
    _tree.check(big, big.raw(), "second tree")
    _train.check(tr, tr.raw(), "trains in between")
    one = a.raw()
    _tree.check(a, one, "first tree")
    a.run()
    again = a.raw()
    for name in one:
        assert one[name].tobytes() == again[name].tobytes(), name


def test_bit_equal_to_compose_train_on_the_root_paths(pool):
    nodes = random_nodes(SEEDS[2]) + named([(None, "c1024"), (40, "c1016"), (41, "c9"), (42, "c8")])
    db, raw = _tree.run(pool, nodes)
    res = db.results(raw)
    trains = _tree.as_trains(db)
    dt = DeviceTrains(pool, trains, fill=_train.FILL)
    dt.run()
    tres = dt.results(dt.raw())
    assert any(r[6] == -2 for r in res) and any(r[6] > 0 for r in res)
    for n, (r, t) in enumerate(zip(res, tres)):
        for name, g, w in zip(_tree.RES, r[:4], t[:4]):
            assert g.tobytes() == w.tobytes(), (n, name)
        length, oc, recs = t[5][-1]
        assert (r[5], r[6]) == (length, oc) and r[7].tobytes() == recs.tobytes(), n
