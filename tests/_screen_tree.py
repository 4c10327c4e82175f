"""What the smx_screen_tree tests share, on top of tests/_screen_train.py (the two oracles of a
train's conflicts) and tests/_tree.py (trees as lists of (parent, log), level order, root paths):
the oracle of node n -- the last step of full_train / rename_train on the logs of n's root path --,
the accumulator carried from parent to child, a pool of small logs, the check of a
DeviceScreenTree run against the oracle, canaries included, and against a DeviceScreenTrains run
of the same root paths, and the golden trains joined under shared prefixes."""
import copy
import json

import numpy as np

from semantic_merge_amd._session import tree_room

import _screen_train as ST
from _batch import ADV, branch, own_logs
from _pairs import logs_soa
from _screen import RENAME, make_log
from _screen_train import FILL, full_train, rename_train  # noqa: F401
from _train import N_KINDS, NONE, logs_ok
from _tree import level_tree, root_path, subtree  # noqa: F401
from _util import to_ops

N_SYM = 40
WIDE = 8192   # the symbol bound of the pool
OTHER = 2     # the kind of the ops that are no renames in the logs given by column


def renames(ts, hi, lo, sym, v0, extra=0):
    """A log of renames given by column, and `extra` other ops after them."""
    n = len(ts)
    pad = [0] * extra
    return make_log([RENAME] * n + [OTHER] * extra, list(ts) + pad, list(hi) + pad, list(lo) + pad,
                    list(sym) + pad, list(v0) + pad, WIDE)


def distinct(n, sym0, seed, extra=3):
    """n renames on the symbols sym0 .. sym0 + n - 1, one each, at random sorted times: such logs
    on ranges of their own conflict with nothing and interleave when they merge."""
    rng = np.random.default_rng(seed)
    return renames(np.sort(rng.integers(1000, 9000, n)), rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n),
                   sym0 + rng.permutation(n), rng.integers(0, 3, n), extra=extra)


def hit(log, name=7):
    """One rename, later than every other one, of the symbol of `log`'s last rename to a name of
    its own: it conflicts with any accumulator that holds `log`, at that record."""
    r = np.flatnonzero(log.kind == RENAME)[-1]
    return renames([9500], [1 << 62], [5], [int(log.sym[r])], [name], extra=1)


NAMES = ("empty", "free6", "free1", "r5", "r5b", "r5c", "r5d", "o10", "o25", "o40", "o60", "a30", "a50", "eqA", "eqB",
         "eqC", "d64a", "d64b", "d65", "d256a", "d256b", "d257", "d1024a", "d1024b", "d1025", "hit64", "hit256",
         "hit1024", "x1100", "y1100", "y1100c", "hitx", "bad18")
IX = {name: i for i, name in enumerate(NAMES)}
SMALL = [IX[n] for n in ("empty", "free6", "r5", "r5b", "r5c", "o10", "o25", "o40", "o60", "a30", "a50", "eqA", "eqB",
                         "eqC")]
SEEDS = [4, 5, 10]  # _tree.random_nodes over SMALL in which a node conflicts and a node below it lands


def make_pool():
    """The logs of NAMES as one LogsSoA: empty and rename-free logs; one symbol renamed five
    times, to one name (r5) or to others at the same times (r5b-d); logs with divergent renames,
    None-valued moves and a shuffled one (o*, a*); three logs whose renames have equal full keys
    (eq*); logs on symbols of their own in sizes that give path sums of 128 / 129, 512 / 513 and
    2048 / 2049 (d*) and a late conflict with the first of each size (hit*); two lists of 1100
    whose only conflict is between their last records (x1100, y1100c; y1100: none); one kind 18."""
    t = [10, 20, 30, 40, 50]
    ts, ids = [10, 20, 20, 30], [1, 2, 2, 3]     # (the middle two: equal keys inside a log too)
    logs = [renames([], [], [], [], []), renames([], [], [], [], [], extra=6), renames([], [], [], [], [], extra=1),
            renames(t, t, t, [3] * 5, [1] * 5, extra=2)]
    logs += [renames(t, t, [x + k for x in t], [3] * 5, [1 + k] * 5, extra=k) for k in (1, 2, 3)]
    logs += own_logs(N_SYM, 100, [10, 25, 40, 60]) + [branch(n, N_SYM, 40 + n, 0, **ADV) for n in (30, 50)]
    logs += [renames(ts, ids, ids, [1, 2, 3, 4], [1, 1, 1, 1], extra=2),
             renames(ts, ids, ids, [5, 6, 7, 8], [2, 2, 2, 2], extra=1),
             renames(ts, ids, ids, [5, 2, 7, 4], [2, 9, 9, 1])]
    sym0, d = 100, []
    for i, n in enumerate((64, 64, 65, 256, 256, 257, 1024, 1024, 1025)):
        d.append(distinct(n, sym0, 20 + i))
        sym0 += n
    logs += d + [hit(d[0]), hit(d[3]), hit(d[6])]
    x, y = distinct(1100, sym0, 40), distinct(1100, sym0 + 1100, 41)
    # (x's and y's last renames: the latest of both lists, y's on x's symbol under another name)
    x.ts[1099], y.ts[1099], x.v0[1099] = 9100, 9101, 1
    yc = copy.deepcopy(y)
    yc.sym[1099], yc.v0[1099] = x.sym[1099], 2
    logs += [x, y, yc, hit(x)]
    bad = copy.deepcopy(logs[IX["r5b"]])
    bad.kind[2] = N_KINDS
    logs.append(bad)
    assert len(logs) == len(NAMES)
    for s in logs:
        s.n_sym = WIDE
    return logs_soa(logs, WIDE)


def named(nodes):
    """[(parent, log name)] as [(parent, log index)]."""
    return [(p, IX[l] if isinstance(l, str) else l) for p, l in nodes]


def node_ref(lsoa, parents, logs, n, full=True, **kw):
    """(renames, outcome, records) of node n: the last step of the train that is its root path."""
    return ST.ref(lsoa, root_path(parents, logs, n), full=full, **kw)[2][-1]


def carry(lsoa, parents, logs):
    """rename_train's accumulator carried from parent to child (level order): per node
    ((renames, outcome, records), list, holder) -- the node's step against its parent's list, the
    list after it (the parent's own list object where the node leaves it as it was: it did not
    land, or its log has no renames) and the node whose step made that list (NONE: none did)."""
    off = np.asarray(lsoa.log_off, np.int64)
    ok = logs_ok(off, int(lsoa.n_total))
    kind = np.asarray(lsoa.kind)
    key = list(zip(np.asarray(lsoa.ts).tolist(), np.asarray(lsoa.oid_hi).tolist(), np.asarray(lsoa.oid_lo).tolist()))
    sym, v0 = np.asarray(lsoa.sym).tolist(), np.asarray(lsoa.v0).astype(np.int32).tolist()
    out = []
    for n in range(len(parents)):
        p, l = int(parents[n]), int(logs[n])
        acc, holder = (out[p][1], out[p][2]) if p >= 0 else ([], NONE)
        if not (0 <= l < len(ok)) or not ok[l] or (kind[int(off[l]): int(off[l + 1])] >= N_KINDS).any():
            out.append(((len(acc), -1, ST.NO_PAIRS), acc, holder))
            continue
        b = ST.sorted_renames(lsoa, int(off[l]), int(off[l + 1])).tolist()
        i = j = 0
        merged, conf = [], []
        while i < len(acc) and j < len(b):
            x, y = acc[i], b[j]
            if sym[x] == sym[y] and v0[x] != v0[y]:
                conf.append((x, y))
                i += 1
                j += 1
            elif key[x] <= key[y]:   # A first on equal keys
                merged.append(x)
                i += 1
            else:
                merged.append(y)
                j += 1
        if conf:
            out.append(((len(acc), len(conf), np.asarray(conf, np.int32).reshape(-1, 2)), acc, holder))
        elif not b:
            out.append(((len(acc), 0, ST.NO_PAIRS), acc, holder))
        else:
            new = merged + acc[i:] + b[j:]
            out.append(((len(new), 0, ST.NO_PAIRS), new, n))
    return out


def host_acc_off(lsoa, parents, logs):
    """acc_off as the host lays it out: the room rule on the logs' rename counts, regions one
    after another."""
    from semantic_merge_amd._lib import _rename_counts
    ren = _rename_counts(lsoa.kind, lsoa.log_off)
    logs = np.asarray(logs)
    ok = (logs >= 0) & (logs < lsoa.n_logs)   # (a log index outside the logs counts as empty)
    return np.concatenate([[0], np.cumsum(tree_room(parents, np.where(ok, ren[np.where(ok, logs, 0)], 0)),
                                          dtype=np.int64)])


def run(lsoa, nodes, **kw):
    from semantic_merge_amd._lib import DeviceScreenTree
    parents, logs, level_off, _ = level_tree(nodes)
    db = DeviceScreenTree(lsoa, parents, logs, kw.pop("level_off", level_off), fill=FILL, **kw)
    db.run()
    return db, db.raw()


def node_cap(db, n):
    """Node n's capacity in conflict records as the device reads conf_off."""
    if db.null_conf:
        return 0
    c0, c1 = int(db.conf_off[n]), int(db.conf_off[n + 1])
    return c1 - c0 if c0 >= 0 and c1 >= c0 else 0


def check(db, raw, label, failed=(), truncated=(), trains=True):
    """Nodes of `failed` (level-order indices, as every index here) and the nodes below them
    report -1, -1 and wrote nothing else; every other node equals full_train on its root path: the
    renames after it, its outcome and its records (nodes of `truncated`: the oracle's first
    records, the full count); no word outside node_counts and the written records was touched.
    trains: the nodes also equal, bit for bit, a DeviceScreenTrains run of the same root paths."""
    res = db.results(raw)
    parents, logs = db.parents, db.node_log
    failed = subtree(parents, failed)
    fill32, fill64 = np.int32(FILL), np.int64(FILL)
    wrote = {name: np.zeros(len(raw[name]), bool) for name in ("conf", "node_counts")}
    for n in range(db.n_nodes):
        k, oc = (int(x) for x in raw["node_counts"][2 * n: 2 * n + 2])
        wrote["node_counts"][2 * n: 2 * n + 2] = True
        if n in failed:
            assert (k, oc) == (-1, -1), f"{label}: node {n} reports {(k, oc)}, not -1"
            continue
        assert not isinstance(res[n], int), f"{label}: node {n} failed structurally"
        exp = node_ref(db.lsoa, parents, logs, n)
        assert (k, oc) == exp[:2], f"{label}: node {n}: (renames, outcome) {(k, oc)}, not {exp[:2]}"
        cap, recs = node_cap(db, n), exp[2]
        if n in truncated:
            assert exp[1] > cap, f"{label}: node {n} is not truncated"
            recs = recs[:cap]
        assert np.array_equal(res[n][2], recs), f"{label}: node {n}: conflict records differ"
        if len(recs):
            c = int(db.conf_off[n])
            wrote["conf"][2 * c: 2 * (c + len(recs))] = True
    for name in wrote:
        fill = fill64 if raw[name].dtype == np.int64 else fill32
        bad = np.flatnonzero(~wrote[name] & (raw[name] != fill))
        assert not len(bad), f"{label}: {name} written outside the valid regions, at {bad[:5].tolist()}"
    if trains:
        same_as_trains(db, raw, label, failed)
    return res


def same_as_trains(db, raw, label, failed=()):
    """Every node outside `failed` against smx_screen_train on its root path, run here: the last
    step's pair of step_counts and its records, word for word (up to the node's capacity)."""
    from semantic_merge_amd._lib import DeviceScreenTrains
    nodes = [n for n in range(db.n_nodes) if n not in failed]
    if not nodes:
        return
    tr = DeviceScreenTrains(db.lsoa, [root_path(db.parents, db.node_log, n) for n in nodes], fill=FILL)
    tr.run()
    traw = tr.raw()
    for r, n in enumerate(nodes):
        g = int(tr.train_off[r + 1]) - 1
        assert int(traw["counts"][2 * r]) >= 0, f"{label}: the train of node {n} failed"
        pair = traw["step_counts"][2 * g: 2 * g + 2]
        assert raw["node_counts"][2 * n: 2 * n + 2].tobytes() == pair.tobytes(), \
            f"{label}: node {n}: {raw['node_counts'][2 * n: 2 * n + 2].tolist()}, smx_screen_train {pair.tolist()}"
        k = min(max(int(pair[1]), 0), node_cap(db, n))
        c, ct = int(db.conf_off[n]), int(tr.conf_off[g])
        assert raw["conf"][2 * c: 2 * (c + k)].tobytes() == traw["conf"][2 * ct: 2 * (ct + k)].tobytes() or not k, \
            f"{label}: node {n}: records differ from smx_screen_train's"


def joined(group):
    """Golden cases (tests/_train.golden_case) as one tree: (logs, nodes, ends, owns).  Logs of
    equal content are pooled once and the trains inserted into a trie, so that trains that start
    with the same logs share those nodes; ends[c]: the nodes of case c's train, root first;
    owns[c][l]: the pooled log that is case c's log l.  Each train of two logs or more comes a
    second time with its last two logs swapped, a sibling path under the shared prefix."""
    logs, where, nodes, child, ends, owns = [], {}, [], {}, [], []

    def walk(train):
        at, path = None, []
        for l in train:
            if (at, l) not in child:
                child[(at, l)] = len(nodes)
                nodes.append((at, l))
            at = child[(at, l)]
            path.append(at)
        return path

    for case in group:
        own = []
        for log in case["logs"]:
            key = json.dumps(log, sort_keys=True)
            if key not in where:
                where[key] = len(logs)
                logs.append(to_ops(log))
            own.append(where[key])
        owns.append(own)
        train = [own[l] for l in case["train"]]
        ends.append(walk(train))
        if len(train) >= 2:
            walk(train[:-2] + [train[-1], train[-2]])
    return logs, nodes, ends, owns


def path_of(nodes, n):
    """The logs from the root to node n of [(parent or None, log)]."""
    path = []
    while n is not None:
        path.append(nodes[n][1])
        n = nodes[n][0]
    return path[::-1]
