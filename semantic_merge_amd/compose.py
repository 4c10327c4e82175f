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

from typing import Any, List, Sequence, Tuple

import numpy as np

from ._abi import BATCH_MAX_OPS
from ._lib import dropin_session
from .marshal import marshal_native, marshal_shared
from .materialize import materialize_conflicts, materialize_ops_native


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


def compose_many(pairs: Sequence[Tuple[Sequence[Any], Sequence[Any]]]) -> List[Tuple[List[Any], List[Any]]]:
    """``[compose_oplogs(a, b) for a, b in pairs]`` with the merges of at most 2048 ops run
    as one GPU batch (one copy in, one smx_compose_batch, one copy back, one sync); larger
    merges take ``compose_oplogs`` one by one.  Inputs are never mutated."""
    logs = [(list(a), list(b)) for a, b in pairs]
    res: List[Any] = [None] * len(logs)
    small = [i for i, (a, b) in enumerate(logs) if len(a) + len(b) <= BATCH_MAX_OPS]
    if small:
        with dropin_session() as sess:
            # each merge marshalled straight into its slice of the pinned staging columns;
            # the results are views of the staging area, materialised while the session is held
            cols = sess.staging_many([len(logs[i][0]) + len(logs[i][1]) for i in small])
            soas = [marshal_native(logs[i][0], logs[i][1], c) for i, c in zip(small, cols)]
            for i, soa, (order, addr, file, ctx, cpairs) in zip(small, soas, sess.compose_many(soas, copy=False)):
                ops = logs[i][0] + logs[i][1]
                res[i] = (materialize_ops_native(ops, soa.kind, soa.strings, order, addr, file, ctx),
                          materialize_conflicts(ops, cpairs))
    for i, (a, b) in enumerate(logs):
        if res[i] is None:
            res[i] = compose_oplogs(a, b)
    return res


def compose_against(shared: Sequence[Any], branches: Sequence[Sequence[Any]],
                    shared_side: str = "a") -> List[Tuple[List[Any], List[Any]]]:
    """``[compose_oplogs(shared, b) for b in branches]`` -- or ``compose_oplogs(b, shared)``
    with ``shared_side="b"`` -- for merges that all have one log on one side: a merge queue
    composing every pull request's delta against the target branch's, a rebase composing
    every commit of a stack against the upstream delta.  The shared log is marshalled and
    copied to the GPU once, and the merges of at most 2048 ops run as one batch (one copy in,
    one smx_compose_batch_shared, one copy back, one sync); larger merges follow one by one.
    Inputs are never mutated."""
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
        for m, (order, addr, file, ctx, cpairs) in enumerate(sess.compose_shared(ssoa, is_b, copy=False)):
            k_own = kind[int(ssoa.off[m]): int(ssoa.off[m + 1])]
            ops = logs[m] + sh if is_b else sh + logs[m]
            k = np.concatenate([k_own, k_sh] if is_b else [k_sh, k_own])
            res.append((materialize_ops_native(ops, k, ssoa.strings, order, addr, file, ctx),
                        materialize_conflicts(ops, cpairs)))
    return res
