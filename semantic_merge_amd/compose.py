"""Drop-in ``compose_oplogs`` (semmerge/compose.py:11) running on the MI355X.

Same signature, same result objects, same exceptions for malformed ops:

    compose_oplogs(delta_a: List[Op], delta_b: List[Op]) -> (List[Op], List[Conflict])

Inputs are never mutated; outputs are fresh ``Op`` objects built with
``type(op)`` / ``type(op.target)`` (so reference ``Op`` instances round-trip),
and conflicts are built from the uncloned inputs, as in the reference.  Marshal and
materialise run in the native host module (csrc/smx_host.cpp), the merge on the GPU.  To wire
it into the reference CLI, rebind the module attribute the CLI looks up
(``semmerge.__main__.compose_oplogs``).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._abi import BATCH_MAX_OPS
from ._session import ComposeSession, dropin_session
from .marshal import marshal_logs, marshal_native, marshal_shared, move_file_alt
from .materialize import conflict_factory, materialize_conflicts, materialize_ops_native


def compose_oplogs(delta_a: Sequence[Any], delta_b: Sequence[Any]) -> Tuple[List[Any], List[Any]]:
    """Compose two op logs into one deterministic sequence plus DivergentRename conflicts."""
    ops_a = list(delta_a)
    ops_b = list(delta_b)
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns; the results are
        # views of its staging area too, materialised while the session is held
        soa = marshal_native(ops_a, ops_b, sess.staging(len(ops_a) + len(ops_b)))
        order, addr, file, ctx, pairs = sess.compose(soa, copy=False)
        ops = ops_a + ops_b
        out = materialize_ops_native(ops, soa.kind, soa.strings, order, addr, file, ctx)
        conflicts = materialize_conflicts(ops, pairs)
    return out, conflicts


def compose_many(pairs: Sequence[Tuple[Sequence[Any], Sequence[Any]]],
                 large: bool = False) -> List[Tuple[List[Any], List[Any]]]:
    """``[compose_oplogs(a, b) for a, b in pairs]`` with the merges of at most 2048 ops run
    as one GPU batch (one copy in, one smx_compose_batch, one copy back, one sync); larger
    merges take ``compose_oplogs`` one by one.  ``large=True``: merges of up to
    ``ComposeSession.LARGE_MAX`` ops join the batch too (smx_compose_batch_ex, SMX_BATCH_LARGE),
    for batches with a tail just past 2048 ops; only longer ones go one by one.  Inputs are
    never mutated."""
    logs = [(list(a), list(b)) for a, b in pairs]
    res: List[Any] = [None] * len(logs)
    limit = ComposeSession.LARGE_MAX if large else BATCH_MAX_OPS
    small = [i for i, (a, b) in enumerate(logs) if len(a) + len(b) <= limit]
    if small:
        with dropin_session() as sess:
            # each merge marshalled straight into its slice of the pinned staging columns;
            # the results are views of the staging area, materialised while the session is held
            cols = sess.staging_many([len(logs[i][0]) + len(logs[i][1]) for i in small])
            soas = [marshal_native(logs[i][0], logs[i][1], c) for i, c in zip(small, cols)]
            for i, soa, (order, addr, file, ctx, cpairs) in zip(small, soas, sess.compose_many(soas, copy=False, large=large)):
                ops = logs[i][0] + logs[i][1]
                res[i] = (materialize_ops_native(ops, soa.kind, soa.strings, order, addr, file, ctx),
                          materialize_conflicts(ops, cpairs))
    for i, (a, b) in enumerate(logs):
        if res[i] is None:
            res[i] = compose_oplogs(a, b)
    return res


def compose_against(shared: Sequence[Any], branches: Sequence[Sequence[Any]],
                    shared_side: str = "a", large: bool = False) -> List[Tuple[List[Any], List[Any]]]:
    """``[compose_oplogs(shared, b) for b in branches]`` -- or ``compose_oplogs(b, shared)``
    with ``shared_side="b"`` -- for merges that all have one log on one side: a merge queue
    composing every pull request's delta against the target branch's, a rebase composing
    every commit of a stack against the upstream delta.  The shared log is marshalled and
    copied to the GPU once, and the merges of at most 2048 ops run as one batch (one copy in,
    one smx_compose_batch_shared, one copy back, one sync); larger merges follow one by one.
    ``large=True``: merges of up to ``ComposeSession.LARGE_MAX`` ops, the shared log counted,
    run in the batch too (smx_compose_batch_shared_ex, SMX_BATCH_LARGE) -- a shared log of more
    than 2048 ops no longer sends every merge through the loop.  Inputs are never mutated."""
    if shared_side not in ("a", "b"):
        raise ValueError("shared_side must be 'a' or 'b'")
    is_b = shared_side == "b"
    sh = list(shared)
    logs = [list(b) for b in branches]
    if not logs:
        return []
    res: List[Tuple[List[Any], List[Any]]] = []
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns; the results are
        # views of its staging area too, materialised while the session is held
        n_total = len(sh) + sum(len(b) for b in logs)
        ssoa = marshal_shared(sh, logs, sess.staging_shared(n_total, len(sh), len(logs)))
        kind = ssoa.kind.copy()  # (a merge routed through compose() reuses the staging columns)
        k_sh = kind[: len(sh)]
        for m, (order, addr, file, ctx, cpairs) in enumerate(sess.compose_shared(ssoa, is_b, copy=False, large=large)):
            k_own = kind[int(ssoa.off[m]): int(ssoa.off[m + 1])]
            ops = logs[m] + sh if is_b else sh + logs[m]
            k = np.concatenate([k_own, k_sh] if is_b else [k_sh, k_own])
            res.append((materialize_ops_native(ops, k, ssoa.strings, order, addr, file, ctx),
                        materialize_conflicts(ops, cpairs)))
    return res


def compose_pairs(logs: Sequence[Sequence[Any]], pairs: Optional[Sequence[Tuple[int, int]]] = None,
                  large: bool = False) -> List[Tuple[List[Any], List[Any]]]:
    """``[compose_oplogs(logs[i], logs[j]) for i, j in pairs]`` for pairs over logs given once:
    the clean pairs that ``screen_all`` left over, M pull requests against K release branches,
    every pair of a merge train.  ``pairs=None``: all ``i < j``.  Every log is marshalled and
    copied to the GPU once, whatever the number of pairs that hold it, and the pairs of at most
    2048 ops run as one batch (one copy in, one smx_compose_pairs, one copy back, one sync);
    larger pairs follow one by one.  ``large=True``: pairs of up to ``ComposeSession.LARGE_MAX``
    ops run in the batch too (SMX_BATCH_LARGE).  A pair outside the logs raises ``IndexError``.
    Inputs are never mutated."""
    ops = [list(x) for x in logs]
    if pairs is None:
        pairs = [(i, j) for i in range(len(ops)) for j in range(i + 1, len(ops))]
    pairs = [(int(i), int(j)) for i, j in pairs]
    for i, j in pairs:
        if not (0 <= i < len(ops) and 0 <= j < len(ops)):
            raise IndexError(f"pair ({i}, {j}) outside the {len(ops)} logs")
    if not pairs:
        return []
    res: List[Tuple[List[Any], List[Any]]] = []
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns; the results are
        # views of its staging area too, materialised while the session is held
        lsoa = marshal_logs(ops, sess.staging_pairs(sum(len(x) for x in ops), len(ops), len(pairs)))
        kind = lsoa.kind.copy()  # (a pair routed through compose() reuses the staging columns)
        off = lsoa.log_off.tolist()
        for (i, j), (order, addr, file, ctx, cpairs) in zip(pairs, sess.compose_pairs(lsoa, pairs, copy=False,
                                                                                      large=large)):
            both = ops[i] + ops[j]
            k = np.concatenate([kind[off[i]: off[i + 1]], kind[off[j]: off[j + 1]]])
            res.append((materialize_ops_native(both, k, lsoa.strings, order, addr, file, ctx),
                        materialize_conflicts(both, cpairs)))
    return res


def _train_on_host(logs: Sequence[Sequence[Any]], train: Sequence[int]) -> Tuple[List[Any], List[List[Any]]]:
    """One train as the host loop over compose_oplogs with eviction (any size)."""
    acc: List[Any] = []
    steps: List[List[Any]] = []
    for l in train:
        out, conf = compose_oplogs(acc, logs[l])
        steps.append(conf)
        if not conf:
            acc = out
    return acc, steps


LOOP_MAX_SYM = 1 << 30  # symbols that smx_compose's window plans accept (more: the host loop)


def compose_train(logs: Sequence[Sequence[Any]], trains: Optional[Sequence[Sequence[int]]] = None,
                  large: bool = False) -> List[Tuple[List[Any], List[List[Any]]]]:
    """Merge trains over logs given once.  A train takes its logs in order: each is composed
    against what landed before it, ``compose_oplogs(acc, log)``; a log that conflicts is put
    off the train (as ``semmerge`` exits before applying anything) and the next one goes on
    against what landed; else the composed ops become ``acc``.  ``trains``: lists of log
    indices (a log may be in many trains, and more than once in one); ``None``: one train of
    all the logs in order.  Per train the result is ``(ops, steps)``: the ops the last landed
    step leaves, and per step its conflicts (an empty list: the step landed) -- equal to that
    host loop.  Every log is marshalled and copied to the GPU once and all the trains run in one
    call (one copy in, one smx_compose_train, one copy back, one sync); the ops are materialised
    once per train.  A train whose accumulator and next log exceed 2048 ops runs as the host
    loop instead.  ``large=True``: such a train runs on the GPU too, step by step over columns
    that stay on the device (smx_train_stage, smx_compose, smx_train_land per step:
    ``ComposeSession.compose_train_loop``), and is materialised once like the others; only logs
    with more than 2^30 symbols keep the host loop.  An index outside the logs raises
    ``IndexError``.  Inputs are never mutated."""
    ops = [list(x) for x in logs]
    if trains is None:
        trains = [list(range(len(ops)))]
    trains = [[int(l) for l in tr] for tr in trains]
    for r, tr in enumerate(trains):
        for l in tr:
            if not 0 <= l < len(ops):
                raise IndexError(f"train {r}: log {l} outside the {len(ops)} logs")
    if not trains:
        return []
    make = conflict_factory()
    res: List[Any] = []
    with dropin_session() as sess:
        lsoa = marshal_logs(ops)
        flat = [o for x in ops for o in x]
        alt, empty = move_file_alt(flat, lsoa.kind, lsoa.strings)
        found = sess.compose_trains(lsoa, trains, v1_alt=alt, empty_str=empty)
        if large and int(lsoa.n_sym) <= LOOP_MAX_SYM:
            found = [sess.compose_train_loop(lsoa, tr, v1_alt=alt, empty_str=empty)
                     if any(oc == -2 for _, oc, _ in f[5]) else f for tr, f in zip(trains, found)]
    for tr, (src, addr, file, ctx, _, steps) in zip(trains, found):
        if any(oc == -2 for _, oc, _ in steps):
            res.append(_train_on_host(ops, tr))
            continue
        out = materialize_ops_native(flat, lsoa.kind, lsoa.strings, src, addr, file, ctx)
        conf = []
        for _, _, recs in steps:
            a = materialize_ops_native(flat, lsoa.kind, lsoa.strings, recs[:, 0], recs[:, 2], recs[:, 3],
                                       np.full(len(recs), -1, np.int32)) if len(recs) else []
            conf.append([make(x, flat[b]) for x, b in zip(a, recs[:, 1].tolist())])
        res.append((out, conf))
    return res


def compose_tree(logs: Sequence[Sequence[Any]], nodes: Sequence[Tuple[Optional[int], int]],
                 want: Any = "leaves") -> List[Tuple[Optional[List[Any]], List[Any]]]:
    """Merge trains that share prefixes, over logs given once: a speculative merge queue (the
    state after pull request 1, after 1+2, ... and the fallbacks that drop a member), every
    prefix of a commit stack.  ``nodes``: per node ``(parent, log)`` -- the index of an earlier
    node or ``None`` for a root, and a log index; the node's root path is a train of
    ``compose_train``: the node composes its log against what landed on the way to it, and a
    node that conflicts leaves that state to its children.  Per node the result is
    ``(ops, conflicts)``: ``conflicts`` is the node's step's conflicts (an empty list: it
    landed), and ``ops`` what has landed after the node, for the nodes ``want`` selects --
    ``"leaves"``, ``"all"`` or an iterable of node indices -- and ``None`` for the others; equal,
    per node, to the host loop over ``compose_oplogs`` on its root path.  Every log is marshalled
    and copied to the GPU once and every node is composed once, whatever the number of paths
    through it (one copy in, one smx_compose_tree, one copy back, one sync); the ops are
    materialised once per selected node.  A node whose accumulator and log exceed 2048 ops, and
    every node below it, is computed by the host loop instead.  A parent that does not precede
    its node raises ``ValueError``, an index outside the nodes or the logs ``IndexError``.
    Inputs are never mutated."""
    from ._session import tree_levels
    ops = [list(x) for x in logs]
    nodes = [(None if p is None else int(p), int(l)) for p, l in nodes]
    parents = [p for p, _ in nodes]
    tree_levels(parents)  # (the parents' checks)
    for n, (_, l) in enumerate(nodes):
        if not 0 <= l < len(ops):
            raise IndexError(f"node {n}: log {l} outside the {len(ops)} logs")
    N = len(nodes)
    if N == 0:
        return []
    if isinstance(want, str):
        if want not in ("leaves", "all"):
            raise ValueError("want must be 'leaves', 'all' or node indices")
        inner = {p for p in parents if p is not None}
        chosen = set(range(N)) if want == "all" else set(range(N)) - inner
    else:
        chosen = {int(n) for n in want}
        for n in chosen:
            if not 0 <= n < N:
                raise IndexError(f"want: node {n} outside the {N} nodes")
    make = conflict_factory()
    with dropin_session() as sess:
        lsoa = marshal_logs(ops)
        flat = [o for x in ops for o in x]
        alt, empty = move_file_alt(flat, lsoa.kind, lsoa.strings)
        found = sess.compose_tree(lsoa, parents, [l for _, l in nodes], v1_alt=alt, empty_str=empty)
    res: List[Any] = []
    on_host = [False] * N  # the node or one above it reports -2
    for n, (state, acc, _, oc, recs) in enumerate(found):
        p = parents[n]
        on_host[n] = oc == -2 or (p is not None and on_host[p])
        if on_host[n]:
            path, up = [], n
            while up is not None:
                path.append(nodes[up][1])
                up = parents[up]
            out, steps = _train_on_host(ops, path[::-1])
            res.append((out if n in chosen else None, steps[-1]))
            continue
        out = None
        if n in chosen:
            src, addr, file, ctx = found[acc][0] if acc >= 0 else (np.zeros(0, np.int32),) * 4
            out = materialize_ops_native(flat, lsoa.kind, lsoa.strings, src, addr, file, ctx)
        a = materialize_ops_native(flat, lsoa.kind, lsoa.strings, recs[:, 0], recs[:, 2], recs[:, 3],
                                   np.full(len(recs), -1, np.int32)) if len(recs) else []
        res.append((out, [make(x, flat[b]) for x, b in zip(a, recs[:, 1].tolist())]))
    return res


def screen_train(logs: Sequence[Sequence[Any]], trains: Optional[Sequence[Sequence[int]]] = None
                 ) -> List[List[List[Tuple[Tuple[int, int], Tuple[int, int]]]]]:
    """Which logs fall off a merge train, and over which ops, without composing anything: per
    train of ``compose_train(logs, trains)``, per step, the conflicts of that step as
    ``((log_a, index_a), (log_b, index_b))`` -- the positions in ``logs`` of the two ops of every
    conflict, in the reference's order; an empty list means the step landed.  ``trains``: lists
    of log indices (a log may be in many trains, and more than once in one); ``None``: one train
    of all the logs in order.  The answer comes from the logs' renames alone (one copy in, one
    smx_screen_train, one copy back, one sync), so trains of any size are served in the one
    call: no size is refused and no host loop stands behind it.  ``opA`` of the reference's
    ``Conflict`` is the accumulated clone, whose ``params`` and ``addressId`` a move chain may
    have changed; that clone comes from ``compose_train``, and this call names the ops only.  An
    index outside the logs raises ``IndexError``.  Inputs are never mutated."""
    ops = [list(x) for x in logs]
    if trains is None:
        trains = [list(range(len(ops)))]
    trains = [[int(l) for l in tr] for tr in trains]
    for r, tr in enumerate(trains):
        for l in tr:
            if not 0 <= l < len(ops):
                raise IndexError(f"train {r}: log {l} outside the {len(ops)} logs")
    if not trains:
        return []
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns
        lsoa = marshal_logs(ops, sess.staging_logs(sum(len(x) for x in ops), len(ops), 0))
        found = sess.screen_trains(lsoa, trains)
    off = np.asarray(lsoa.log_off, np.int64)

    def where(cols):
        log = np.searchsorted(off, cols, "right") - 1
        return list(zip(log.tolist(), (cols - off[log]).tolist()))

    return [[list(zip(where(recs[:, 0].astype(np.int64)), where(recs[:, 1].astype(np.int64)))) for _, _, recs in steps]
            for _, _, steps in found]


def screen_tree(logs: Sequence[Sequence[Any]], nodes: Sequence[Tuple[Optional[int], int]]
                ) -> List[List[Tuple[Tuple[int, int], Tuple[int, int]]]]:
    """Which nodes of a tree of merge trains lose their log, and over which ops, without
    composing anything: per node of ``compose_tree(logs, nodes)`` the conflicts of that node as
    ``((log_a, index_a), (log_b, index_b))`` -- the positions in ``logs`` of the two ops of every
    conflict, in the reference's order; an empty list means the node landed.  ``nodes``: per node
    ``(parent, log)`` -- the index of an earlier node or ``None`` for a root, and a log index; per
    node the answer is ``screen_train``'s for the last step of the node's root path.  It comes
    from the logs' renames alone (one copy in, one smx_screen_tree, one copy back, one sync): every
    log's renames are sorted once and every node is walked once, whatever the number of paths
    through it, and trees of any size are served in the one call: no size is refused, nothing is
    materialised and no host loop stands behind it.  ``opA`` of the reference's ``Conflict`` is
    the accumulated clone, which comes from ``compose_tree``; this call names the ops only.  A
    parent that does not precede its node raises ``ValueError``, an index outside the nodes or
    the logs ``IndexError``.  Inputs are never mutated."""
    from ._session import tree_levels
    ops = [list(x) for x in logs]
    nodes = [(None if p is None else int(p), int(l)) for p, l in nodes]
    parents = [p for p, _ in nodes]
    tree_levels(parents)  # (the parents' checks)
    for n, (_, l) in enumerate(nodes):
        if not 0 <= l < len(ops):
            raise IndexError(f"node {n}: log {l} outside the {len(ops)} logs")
    if not nodes:
        return []
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns
        lsoa = marshal_logs(ops, sess.staging_logs(sum(len(x) for x in ops), len(ops), 0))
        found = sess.screen_tree(lsoa, parents, [l for _, l in nodes])
    off = np.asarray(lsoa.log_off, np.int64)

    def where(cols):
        log = np.searchsorted(off, cols, "right") - 1
        return list(zip(log.tolist(), (cols - off[log]).tolist()))

    return [list(zip(where(recs[:, 0].astype(np.int64)), where(recs[:, 1].astype(np.int64)))) for _, _, recs in found]


def screen_conflicts(logs: Sequence[Sequence[Any]],
                     pairs: Optional[Sequence[Tuple[int, int]]] = None, large: bool = False) -> List[List[Any]]:
    """``[compose_oplogs(logs[i], logs[j])[1] for i, j in pairs]`` -- the DivergentRename
    conflicts alone, no composed ops -- for a caller that asks which of many logs conflict
    (a merge queue: every pull request against the target branch, or against each other
    before they share a merge train).  ``pairs=None``: all ``i < j``.  Every log is
    marshalled, copied to the GPU and has its renames sorted once, whatever the number of
    pairs that hold it; a pair costs one merge of two short lists (one copy in, one
    smx_screen, one copy back, one sync).  Pairs of more than 2048 renames follow through
    the full composition one by one; ``large=True`` screens them in the same call instead
    (smx_screen_ex, SMX_SCREEN_LARGE), for logs of thousands of renames such as a busy target
    branch's delta.  Inputs are never mutated and no ``Op`` is cloned: the
    conflicts are built from the input objects, as in the reference."""
    ops = [list(x) for x in logs]
    if pairs is None:
        pairs = [(i, j) for i in range(len(ops)) for j in range(i + 1, len(ops))]
    pairs = [(int(i), int(j)) for i, j in pairs]
    for i, j in pairs:
        if not (0 <= i < len(ops) and 0 <= j < len(ops)):
            raise IndexError(f"pair ({i}, {j}) outside the {len(ops)} logs")
    if not pairs:
        return []
    make = conflict_factory()
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns
        lsoa = marshal_logs(ops, sess.staging_logs(sum(len(x) for x in ops), len(ops), len(pairs)))
        found = sess.screen(lsoa, pairs, large=large)
    res: List[List[Any]] = []
    for (i, j), cp in zip(pairs, found):
        a, b, na = ops[i], ops[j], len(ops[i])
        res.append([make(a[x], b[y - na]) for x, y in cp.tolist()])
    return res


def screen_all(logs: Sequence[Sequence[Any]], large: bool = False) -> Dict[Tuple[int, int], List[Any]]:
    """``{(i, j): compose_oplogs(logs[i], logs[j])[1]}`` for the pairs ``i < j`` that have at
    least one conflict, keys ascending: ``screen_conflicts(logs)`` restricted to its non-empty
    entries, for a queue of many logs of which few can conflict.  The GPU first finds the pairs
    that rename one symbol to different names (smx_screen_candidates; every other pair has no
    conflicts) and screens only those, on columns copied once, so the cost follows the
    conflicting part of the queue and not the number of pairs.  The result is sparse because
    a dense list over thousands of logs is the cost this call removes.  ``large`` as in
    ``screen_conflicts``.  Inputs are never
    mutated and no ``Op`` is cloned."""
    ops = [list(x) for x in logs]
    if len(ops) < 2:
        return {}
    make = conflict_factory()
    with dropin_session() as sess:
        # marshalled straight into the session's pinned staging columns
        # (sized for screen_all's starting capacity of pairs, so that it stages them in place)
        lsoa = marshal_logs(ops, sess.staging_logs(sum(len(x) for x in ops), len(ops), max(9 * len(ops), 2048)))
        pairs, found = sess.screen_all(lsoa, large=large)
    res: Dict[Tuple[int, int], List[Any]] = {}
    for (i, j), cp in zip(pairs.tolist(), found):
        if len(cp):
            a, b, na = ops[i], ops[j], len(ops[i])
            res[(i, j)] = [make(a[x], b[y - na]) for x, y in cp.tolist()]
    return res
