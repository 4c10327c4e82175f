"""What the smx_compose_tree tests share, on top of tests/_train.py: trees as lists of (parent,
log) in any order with parents first, brought into the level order the C ABI takes; the oracle
of node n, `_train.run_train` on the logs of n's root path (its last step: the node's length,
outcome and records; its result: the node's accumulator); and the check of a DeviceTree run
against it, canaries included."""
import numpy as np

from semantic_merge_amd._session import tree_levels
from semantic_merge_amd.marshal import SoA

import _train
from _batch import ADV, branch, own_logs
from _pairs import logs_soa
from _shapes import pick
from _train import FILL, NONE, RES

N_SYM = 64
RENAME = 1
NAMES = ("empty", "one", "o10", "o25", "o40", "o60", "o90", "o120", "a30", "a50", "c128a", "c128b", "c129", "c512a",
         "c512b", "c513", "c1024", "c1016", "c9", "c8", "badkind", "badsym")
IX = {name: i for i, name in enumerate(NAMES)}


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


def make_pool():
    """The logs of NAMES as one LogsSoA: the recipe of test_gpu_train.py's pool -- logs with
    divergent renames, None-valued moves and a shuffled one (o*, a*), rename-free logs of the
    sizes the class and the 2048 edges need (c*), and two invalid ones."""
    own = own_logs(N_SYM, 100, [10, 25, 40, 60, 90, 120])
    adv = [branch(n, N_SYM, 40 + n, 0, **ADV) for n in (30, 50)]
    sizes = (128, 128, 129, 512, 512, 513, 1024, 1016, 9, 8)
    logs = [pick(own[0], np.zeros(own[0].n_a, bool), np.zeros(own[0].n_b, bool)), branch(1, N_SYM, 3, 1)] + own + adv
    logs += [clean(n, 7 + i) for i, n in enumerate(sizes)]
    logs += [spoiled(own[1], kind=18), spoiled(own[2], sym=N_SYM)]
    assert len(logs) == len(NAMES) and [x.n for x in logs[10:20]] == list(sizes)
    return logs_soa(logs, N_SYM)


SMALL = [IX[n] for n in ("empty", "one", "o10", "o25", "o40", "o60", "a30", "a50")]
SEEDS = [4, 5, 10]  # random_nodes in which a node conflicts and a node below it lands (the tests assert it)


def random_nodes(seed, n=40, depth=6, logs=SMALL):
    """~n nodes (parent, log), parents first, at most `depth` levels: logs of 0..60 ops over a
    few symbols, so that steps do conflict, with None-valued moves among them."""
    rng = np.random.default_rng(seed)
    nodes, level = [], []
    for i in range(n):
        cand = [p for p in range(i) if level[p] < depth - 1]
        p = None if i < 3 or not cand or rng.random() < 0.1 else int(rng.choice(cand))
        nodes.append((p, int(rng.choice(logs))))
        level.append(0 if p is None else level[p] + 1)
    return nodes


def named(nodes):
    """[(parent, log name)] as [(parent, log index)]."""
    return [(p, IX[l] if isinstance(l, str) else l) for p, l in nodes]


def level_tree(nodes):
    """[(parent or None, log)] in the caller's order as (parents, logs, level_off, order) in
    level order: what DeviceTree takes, and order[i], the caller's index of the node stored at i."""
    order, level_off, back = tree_levels([p for p, _ in nodes])
    parents = np.asarray([NONE if nodes[n][0] is None else back[nodes[n][0]] for n in order], np.int32)
    return parents, np.asarray([nodes[n][1] for n in order], np.int32), level_off, order


def root_path(parents, logs, n):
    """The logs from the root to node n."""
    path = []
    while n >= 0:
        path.append(int(logs[n]))
        n = int(parents[n])
    return path[::-1]


def node_ref(lsoa, parents, logs, n, **kw):
    """(src, addr, file, ctx, (length, outcome, records)) of node n: the train that is its path."""
    w = _train.ref(lsoa, root_path(parents, logs, n), **kw)
    return w[:4] + (w[5][-1],)


def expected_acc(lsoa, parents, logs, failed=(), **kw):
    """node_acc as the oracle has it: the nearest node on the root path, itself included, that landed."""
    acc = np.full(len(parents), NONE, np.int64)
    for n in range(len(parents)):  # (level order: a parent lies before its children)
        if n in failed:
            continue
        landed = node_ref(lsoa, parents, logs, n, **kw)[4][1] == 0
        acc[n] = n if landed else (acc[parents[n]] if parents[n] >= 0 else NONE)
    return acc


def carry_step(lsoa, state, l, v1_alt=None, empty_str=NONE):
    """One node by hand, from its parent's state (src, addr, file, ctx): (the node's state, (length,
    outcome, records)) -- run_train's step, written out so that the state can come from anywhere.
    A step that does not land returns the parent's state itself."""
    from oracle import oracle
    from semantic_merge_amd._abi import BATCH_MAX_OPS
    from semantic_merge_amd.ops import KIND_MOVE
    cols = {c: np.asarray(getattr(lsoa, c)) for c in _train.COLS}
    off = np.asarray(lsoa.log_off, np.int64)
    src, addr, file, ctx = state
    none = np.zeros((0, 4), np.int32)
    if not (0 <= l < len(off) - 1) or not _train.logs_ok(off, int(lsoa.n_total))[l]:
        return state, (len(src), -1, none)
    lo, nb = int(off[l]), int(off[l + 1] - off[l])
    if len(src) + nb > BATCH_MAX_OPS:
        return state, (len(src), -2, none)
    idx = np.concatenate([src, np.arange(lo, lo + nb, dtype=np.int32)]).astype(np.int32)
    fresh = np.full(nb, NONE, np.int32)
    a, f, x = np.concatenate([addr, fresh]), np.concatenate([file, fresh]), np.concatenate([ctx, fresh])
    kind, sym = cols["kind"][idx], cols["sym"][idx]
    if (kind >= _train.N_KINDS).any() or (sym.astype(np.int64) >= int(lsoa.n_sym)).any():
        return state, (len(src), -1, none)
    move = kind == KIND_MOVE
    v0 = np.where(move & (a != NONE), a, cols["v0"][idx]).astype(np.int32)
    v1 = np.where(move & (f != NONE), f, cols["v1"][idx]).astype(np.int32)
    if empty_str != NONE:
        v1 = np.where(move & (f == empty_str), np.asarray(v1_alt, np.int32)[idx], v1).astype(np.int32)
    soa = SoA(len(src), nb, kind, cols["ts"][idx], cols["oid_hi"][idx], cols["oid_lo"][idx], sym, v0, v1,
              int(lsoa.n_sym))
    order, ra, rf, rx, pairs = oracle.compose(soa)
    if len(pairs):
        ea, eb = pairs[:, 0], pairs[:, 1]
        return state, (len(src), len(pairs), np.stack([idx[ea], idx[eb], a[ea], f[ea]], axis=1).astype(np.int32))
    new = (idx[order], np.where(ra != NONE, ra, a[order]).astype(np.int32),
           np.where(rf != NONE, rf, f[order]).astype(np.int32), np.where(rx != NONE, rx, x[order]).astype(np.int32))
    return new, (len(new[0]), 0, none)


def run(lsoa, nodes, **kw):
    from semantic_merge_amd._lib import DeviceTree
    parents, logs, level_off, _ = level_tree(nodes)
    db = DeviceTree(lsoa, parents, logs, kw.pop("level_off", level_off), fill=FILL, **kw)
    db.run()
    return db, db.raw()


def subtree(parents, roots):
    """The nodes of `roots` and every node below them (level order)."""
    out = set(roots)
    for n in range(len(parents)):
        if int(parents[n]) in out:
            out.add(n)
    return out


def check(db, raw, label, failed=(), truncated=(), **kw):
    """Nodes of `failed` (level-order indices, as every index here) and the nodes below them
    report -1, -1 and SMX_NONE and wrote nothing else; every other node equals the oracle: its
    length, outcome and records (nodes of `truncated`: the oracle's first records, the full
    count), node_acc, and the accumulator read through node_acc; no word outside the landed
    nodes' count-long regions, the records, node_counts and node_acc was written."""
    res = db.results(raw)
    parents, logs = db.parents, db.node_log
    failed = subtree(parents, failed)
    want_acc = expected_acc(db.lsoa, parents, logs, failed, **kw)
    fill32, fill64 = np.int32(FILL), np.int64(FILL)
    wrote = {name: np.zeros(len(raw[name]), bool) for name in RES + ("conf", "node_counts", "node_acc")}
    for n in range(db.n_nodes):
        k, oc = (int(x) for x in raw["node_counts"][2 * n: 2 * n + 2])
        wrote["node_counts"][2 * n: 2 * n + 2] = True
        wrote["node_acc"][n] = True
        if n in failed:
            assert (k, oc, int(raw["node_acc"][n])) == (-1, -1, NONE), f"{label}: node {n} reports {(k, oc)}, not -1"
            continue
        assert not isinstance(res[n], int), f"{label}: node {n} failed structurally"
        w = node_ref(db.lsoa, parents, logs, n, **kw)
        exp = w[4]
        assert (k, oc) == exp[:2], f"{label}: node {n}: (length, outcome) {(k, oc)}, not {exp[:2]}"
        assert int(raw["node_acc"][n]) == want_acc[n], f"{label}: node {n}: node_acc {raw['node_acc'][n]}, not {want_acc[n]}"
        for name, g, r in zip(RES, res[n][:4], w[:4]):
            assert np.array_equal(g, r), f"{label}: node {n}: {name} differs: {g[:8]} vs {r[:8]} ({len(g)}, {len(r)})"
        c, cap = int(db.conf_off[n]), int(db.conf_off[n + 1] - db.conf_off[n])
        recs = exp[2]
        if n in truncated:
            assert exp[1] > max(cap, 0), f"{label}: node {n} is not truncated"
            recs = recs[:max(cap, 0)]
        assert np.array_equal(res[n][7], recs), f"{label}: node {n}: conflict records differ"
        if len(recs):
            wrote["conf"][4 * c: 4 * (c + len(recs))] = True
        if oc == 0:
            o = int(db.res_off[n])
            for name in RES:
                wrote[name][o: o + k] = True
    for name in wrote:
        fill = fill64 if raw[name].dtype == np.int64 else fill32
        bad = np.flatnonzero(~wrote[name] & (raw[name] != fill))
        assert not len(bad), f"{label}: {name} written outside the valid regions, at {bad[:5].tolist()}"
    return res


def as_trains(db):
    """The root paths of a DeviceTree's nodes as trains."""
    return [root_path(db.parents, db.node_log, n) for n in range(db.n_nodes)]
