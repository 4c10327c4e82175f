"""GPU parity of the tree screen (smx_screen_tree, csrc/smx_screen_tree.h), exactly: every node's
outcome, the renames its accumulator holds and its (A column, B column) conflict records equal
full_train on the node's root path (tests/_screen_train.py) and, bit for bit, an smx_screen_train
run of the same root paths in the same test.  Every output word starts as a canary, so the words a
call must not write are checked.  Shapes: random trees; a chain, a star over the classes, a single
level, a root without renames; nodes that leave the list where it was (no renames, a conflict, a
-1) above a node that reads it; a log twice on a path; the class edges; nodes over 2048 renames in
rounds; truncation; structural failures; one workgroup for everything; one workspace for several
calls."""
import numpy as np
import pytest

from semantic_merge_amd._lib import DeviceScreenTrains, DeviceScreenTree

import _screen_train as ST
import _screen_tree as T
import _tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    return T.make_pool()


def direct(pool, parents, logs, level_off, **kw):
    """A run on a tree given in level order as it is, broken or not."""
    db = DeviceScreenTree(pool, parents, logs, level_off, fill=T.FILL, **kw)
    db.run()
    return db, db.raw()


def outcomes(res):
    return [r if isinstance(r, int) else r[1] for r in res]


SHAPES = T.named([
    (None, "free6"), (0, "r5"), (1, "free1"), (2, "r5b"),      # a root without renames; rename-free under a landed node
    (1, "r5c"), (4, "r5d"),                                     # under a conflicting node
    (1, "bad18"), (6, "r5b"), (1, 99), (8, "r5d"),              # under a -1 node (kind 18; an index outside the logs)
    (1, "r5"), (10, "r5b"),                                     # the same log twice: equal keys, A first
    (None, "eqA"), (12, "eqA"), (13, "eqC"), (12, "eqB"), (15, "eqC"), (12, "eqC"), (17, "eqB"),
    (None, "o10"), (19, "o25"), (20, "o40"), (21, "o60"), (22, "a30"), (23, "a50"), (24, "o10"),   # a chain
    (None, "d64a"), (26, "d64b"), (26, "d65"), (26, "d256a"), (26, "d1024a"), (26, "free6"), (26, "r5"),  # a star
    (26, "hit64"), (27, "hit64"), (28, "hit64"), (29, "hit64"), (30, "hit64"), (31, "hit64"), (32, "hit64"),
    (None, "empty"), (40, "empty"), (41, "r5b")])


@pytest.mark.parametrize("seed", T.SEEDS)
def test_random_trees(pool, seed):
    nodes = _tree.random_nodes(seed, logs=T.SMALL)
    db, raw = T.run(pool, nodes)
    assert db.n_levels <= 6
    res = T.check(db, raw, f"seed {seed}")
    below = 0
    for n in range(db.n_nodes):
        up = int(db.parents[n])
        while up >= 0 and res[up][1] <= 0:
            up = int(db.parents[up])
        below += res[n][1] == 0 and res[n][0] > (res[up][0] if up >= 0 else 0) and up >= 0
    assert below, "no node lands below a conflicting one"


def test_shapes(pool):
    db, raw = T.run(pool, SHAPES)
    res = T.check(db, raw, "shapes")
    back = {int(c): i for i, c in enumerate(T.level_tree(SHAPES)[3])}   # the caller's node -> its place
    r = [res[back[n]] for n in range(len(SHAPES))]
    assert [x[:2] for x in r[:4]] == [(0, 0), (5, 0), (5, 0), (5, 5)]
    assert r[4][:2] == (5, 5) and r[5][:2] == (5, 5)
    assert r[6][:2] == (5, -1) and r[7][:2] == (5, 5) and r[8][:2] == (5, -1) and r[9][:2] == (5, 5)
    assert r[10][:2] == (10, 0) and r[11][1] > 0
    assert r[14][1] > 0 and (r[16][1], r[16][2].tolist()) != (r[18][1], r[18][2].tolist())   # the order decides
    assert [x[:2] for x in r[26:33]] == [(64, 0), (128, 0), (129, 0), (320, 0), (1088, 0), (64, 0), (69, 0)]
    assert [x[1] for x in r[33:40]] == [1] * 7
    assert [x[:2] for x in r[40:]] == [(0, 0), (0, 0), (5, 0)]
    # a node whose log has no renames, or is outside the logs, needs and has no room
    for n in (0, 2, 8, 31, 40, 41):
        assert db.acc_off[back[n] + 1] == db.acc_off[back[n]]
    single = T.named([(None, l) for l in ("r5", "free6", "empty", "o60", "bad18", "d257", "eqC", 99)])
    db, raw = T.run(pool, single)
    assert db.n_levels == 1
    res = T.check(db, raw, "a single level")
    assert outcomes(res) == [0, 0, 0, 0, -1, 0, 0, -1] and res[5][0] == 257


def test_class_edges_and_rounds(pool):
    nodes = T.named([(None, "d64a"), (0, "d64b"), (1, "hit64"), (0, "d65"), (3, "hit64"),
                     (None, "d256a"), (5, "d256b"), (6, "hit256"), (5, "d257"), (8, "hit256"),
                     (None, "d1024a"), (10, "d1024b"), (11, "hit1024"), (10, "d1025"), (13, "hit1024"),
                     (None, "x1100"), (15, "y1100c"), (15, "y1100"), (17, "hitx"), (16, "hitx")])
    db, raw = T.run(pool, nodes)
    res = T.check(db, raw, "edges")
    back = {int(c): i for i, c in enumerate(T.level_tree(nodes)[3])}
    r = [res[back[n]] for n in range(len(nodes))]
    assert [r[n][:2] for n in (1, 3, 6, 8, 11, 13)] == [(128, 0), (129, 0), (512, 0), (513, 0), (2048, 0), (2049, 0)]
    assert [r[n][1] for n in (2, 4, 7, 9, 12, 14)] == [1] * 6
    off = np.asarray(pool.log_off)
    # the only conflict of two lists of 1100: their last records, past the first 1024 of each side
    assert r[16][:2] == (1100, 1) and r[16][2].tolist() == [[off[T.IX["x1100"]] + 1099, off[T.IX["y1100c"]] + 1099]]
    # no conflict: the child walks a merged region of 2200 records, and meets x's last one
    assert r[17][:2] == (2200, 0) and r[18][:2] == (2200, 1) and r[18][2][0, 0] == off[T.IX["x1100"]] + 1099
    assert r[19][:2] == (1100, 1)


TRUNC = T.named([(None, "r5"), (0, "r5b"), (0, "r5c"), (1, "r5d"), (None, "o40"), (4, "o60"), (4, "a50"),
                 (None, "eqA"), (7, "eqC")])


@pytest.mark.parametrize("caps", [0, 2, "null"])
def test_truncated_capacity(pool, caps):
    parents, logs, _, _ = T.level_tree(TRUNC)
    oc = [T.node_ref(pool, parents, logs, n)[1] for n in range(len(TRUNC))]
    assert oc.count(5) == 3 and 0 < min(o for o in oc if o) <= 2
    truncated = [n for n, o in enumerate(oc) if o > (0 if caps == "null" else caps)]
    db, raw = T.run(pool, TRUNC, conf_caps=caps if caps == "null" else [caps] * len(oc))
    T.check(db, raw, f"capacity {caps}", truncated=truncated)
    if caps == "null":
        assert (raw["conf"] == np.int32(T.FILL)).all()


def test_conf_off_that_describes_no_region(pool):
    nodes = T.named([(None, "r5"), (0, "r5b"), (0, "r5c"), (0, "r5d")])
    T.check(*T.run(pool, nodes, conf_off=[0, 5, -1, 15, 20]), "a negative conf_off entry", truncated={1, 2})
    T.check(*T.run(pool, nodes, conf_off=[0, 5, 12, 10, 20]), "a decreasing conf_off entry", truncated={2})


def test_structural_failures(pool):
    """Level 0: nodes 0-2; level 1: 3, 4 under 0, 5 under 1, 6 under 2; level 2: 7 under 3, 8
    under 5, 9 under 6."""
    parents = np.array([-1, -1, -1, 0, 0, 1, 2, 3, 5, 6], np.int32)
    logs = np.array([T.IX[l] for l in ("r5", "o10", "eqA", "r5b", "o25", "o40", "eqB", "r5c", "o60", "eqC")], np.int32)
    good = np.array([0, 3, 7, 10], np.int64)
    T.check(*direct(pool, parents, logs, good), "the tree as it is")
    T.check(*direct(pool, parents, logs, [0, 3, 2, 10]), "level_off decreases", failed=set(range(3, 10)))
    T.check(*direct(pool, parents, logs, [1, 3, 7, 10]), "level 0 does not start at node 0", failed=set(range(10)))
    T.check(*direct(pool, parents, logs, [0, 3, 7, 9]), "the last level ends before the nodes", failed={7, 8, 9})
    p = parents.copy()
    p[5] = 6
    T.check(*direct(pool, p, logs, good), "a parent in the node's own level", failed={5})
    p = parents.copy()
    p[8] = 1
    T.check(*direct(pool, p, logs, good), "a parent two levels up", failed={8})
    p = parents.copy()
    p[1] = 0
    T.check(*direct(pool, p, logs, good), "a level-0 node with a parent", failed={1})
    wide = np.arange(11, dtype=np.int64) * 700
    T.check(*direct(pool, parents, logs, good, acc_off=wide), "regions with room to spare")
    down = wide.copy()
    down[5] = 5
    T.check(*direct(pool, parents, logs, good, acc_off=down), "acc_off decreases", failed={4, 5})
    neg = wide.copy()
    neg[0] = -1
    T.check(*direct(pool, parents, logs, good, acc_off=neg), "a negative acc_off entry", failed={0})
    T.check(*direct(pool, parents, logs, good, acc_off=wide, n_acc=6999), "a region past n_acc", failed={9})
    own = T.host_acc_off(pool, parents, logs)
    assert own[8] - own[7] == 15      # P(7): r5, r5b and r5c on its path, five renames each
    short = own.copy()
    short[8:] -= 1
    T.check(*direct(pool, parents, logs, good, acc_off=short), "a region one rename below P(n)", failed={7})


def test_no_room_for_a_node_without_renames(pool):
    """A region of 0 is accepted for a node whose log has no renames, however long its path's
    list is, and its child reads the list where it was."""
    nodes = T.named([(None, "d256a"), (0, "free6"), (1, "hit256"), (1, "d257")])
    parents, logs, level_off, _ = T.level_tree(nodes)
    acc_off = np.array([0, 256, 256, 256 + 257, 256 + 257 + 513], np.int64)
    db, raw = direct(pool, parents, logs, level_off, acc_off=acc_off)
    res = T.check(db, raw, "no room")
    assert [r[:2] for r in res] == [(256, 0), (256, 0), (256, 1), (513, 0)]


def test_grid_cap_one(pool):
    raws = {}
    for cap in (0, 1):
        db, raws[cap] = T.run(pool, SHAPES, grid_cap=cap)
        T.check(db, raws[cap], f"grid_cap {cap}", trains=cap == 0)
    for name, a in raws[0].items():
        assert a.tobytes() == raws[1][name].tobytes(), f"grid_cap 1: {name} differs from grid_cap 0"


def test_one_workspace_for_several_calls(pool):
    pa, la, va, _ = T.level_tree(SHAPES)
    pb, lb, vb, _ = T.level_tree(_tree.random_nodes(T.SEEDS[0], logs=T.SMALL))
    a = DeviceScreenTree(pool, pa, la, va, fill=T.FILL)
    b = DeviceScreenTree(pool, pb, lb, vb, fill=T.FILL)
    t = DeviceScreenTrains(pool, [[T.IX[l] for l in tr] for tr in (("r5", "r5b", "o40"), ("d256a", "d257", "hit256"))],
                           fill=ST.FILL)
    size = max(x.ws_bytes for x in (a, b, t))
    ws = a.torch.full((size,), 0xA5, dtype=a.torch.uint8, device=a.device)
    for x in (a, b, t):
        x.ws, x.ws_bytes = ws, size
    a.run()
    b.run()
    T.check(b, b.raw(), "second tree", trains=False)
    t.run()
    a.run()
    first = a.raw()
    T.check(a, first, "after smx_screen_train on the same workspace", trains=False)
    ST.check(t, t.raw(), "smx_screen_train in between")
    a.run()
    again = a.raw()
    for name in first:
        assert first[name].tobytes() == again[name].tobytes(), name
