"""Ordered-list CRDT (RGA) entry points, batched onto the GPU.

Reference: ``semmerge/crdt.py:8-57``.  ``Key``, ``Elem`` and the ``RGA`` method names and
argument meaning are unchanged; ``RGA`` records its event stream and
``materialize()`` replays it through ``smx_rga_replay`` (include/smx.h); ``RGA.list``
(the reference's state, crdt.py:26-27) replays it in the library's list mode, which
keeps the tombstoned elements.
:func:`replay` is the batched entry point: many independent lists in one launch;
:func:`replay_onto` replays many event streams onto base lists that are stored once
(``smx_rga_replay_onto``); :func:`replay_chain` replays jobs that are runs of segments stored
once (``smx_rga_replay_chain``).

Exact parallel restatement used by the device: the fate
of every element depends only on the events of its (list, value); survivors
are ordered by (key, creation order) because every insert keeps the list
sorted by key with equal keys in insertion order (``_find_insert_index``,
crdt.py:48-57, inserts before the first strictly greater key).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Sequence, Tuple

import numpy as np

from .marshal import _EqClasses, _encode_ids

INSERT, MOVE, DELETE = 0, 1, 2


@dataclass(frozen=True)
class Key:
    """Position key (crdt.py:8-13); compared as the tuple (anchor, t, author, opid)."""

    anchor: str
    t: int
    author: str
    opid: str


@dataclass
class Elem:
    """List element (crdt.py:16-20)."""

    key: Key
    value: str
    tombstone: bool = False


Event = Tuple[int, Any, Any]  # (INSERT|MOVE|DELETE, key or None, value)


@dataclass
class RgaBatch:
    """Host image of ``smx_rga_ops``."""

    n_lists: int
    list_id: np.ndarray
    op: np.ndarray
    value: np.ndarray
    anchor: np.ndarray
    t: np.ndarray
    author: np.ndarray
    opid_hi: np.ndarray
    opid_lo: np.ndarray
    values: List[Any]          # event index -> value object (what materialize returns)

    @property
    def n(self) -> int:
        return len(self.op)


def _rank(xs: Sequence[Any]) -> np.ndarray:
    table = {x: i for i, x in enumerate(sorted(set(xs)))}
    return np.fromiter((table[x] for x in xs), np.uint32, len(xs))


def _event_columns(streams: Sequence[Sequence[Event]]):
    """The event columns of `streams`, one after another, in one id domain: (list ids, op,
    value, anchor, t, author, opid_hi, opid_lo, value objects).  Values are interned by one
    _EqClasses; anchors, authors and a non-int t are ranked over all the events."""
    lids, ops, vals, anchors, ts, authors, opids, objs = [], [], [], [], [], [], [], []
    eq = _EqClasses()
    for lid, stream in enumerate(streams):
        for kind, key, value in stream:
            lids.append(lid)
            ops.append(kind)
            vals.append(eq(value))
            objs.append(value)
            if key is None:  # delete: key unused
                anchors.append("")
                ts.append(0)
                authors.append("")
                opids.append("")
            else:
                anchors.append(key.anchor)
                ts.append(key.t)
                authors.append(key.author)
                opids.append(key.opid)
    n = len(ops)
    tarr = np.fromiter(ts, np.int64, n) if all(
        type(x) is int and -2 ** 63 <= x < 2 ** 63 for x in ts) else _rank(ts).astype(np.int64)
    _, hi, lo = _encode_ids(opids) if n else (0, np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    return (np.asarray(lids, np.uint32), np.asarray(ops, np.uint8), np.asarray(vals, np.uint32),
            _rank(anchors), tarr, _rank(authors), hi, lo, objs)


def marshal_streams(streams: Sequence[Sequence[Event]]) -> RgaBatch:
    return RgaBatch(len(streams), *_event_columns(streams))


@dataclass
class RgaOntoBatch:
    """Host image of ``smx_rga_onto``: every base's events once, then the jobs' own events."""

    n_bases: int
    n_jobs: int
    base_off: np.ndarray       # i64 [n_bases + 1]
    own_off: np.ndarray        # i64 [n_jobs + 1]
    job_base: np.ndarray       # i32 [n_jobs], -1 (SMX_NONE): no base
    op: np.ndarray
    value: np.ndarray
    anchor: np.ndarray
    t: np.ndarray
    author: np.ndarray
    opid_hi: np.ndarray
    opid_lo: np.ndarray
    values: List[Any]          # column index -> value object

    @property
    def n(self) -> int:
        return len(self.op)

    @property
    def job_len(self) -> np.ndarray:
        """Events per job: its base's and its own."""
        base_len = np.diff(self.base_off)
        b = self.job_base
        return np.where(b >= 0, base_len[np.maximum(b, 0)] if self.n_bases else 0, 0) + np.diff(self.own_off)

    @property
    def n_out(self) -> int:
        return int(self.job_len.sum())


Job = Tuple[Any, Sequence[Event]]  # (base index or None, own events)


def marshal_onto(bases: Sequence[Sequence[Event]], jobs: Sequence[Job]) -> RgaOntoBatch:
    """The columns of ``smx_rga_replay_onto``: each base marshalled once, the jobs' own
    streams after them, all in one id domain (a value, anchor or author of a base and of an
    own stream gets one id, so an own move or delete reaches the base's elements)."""
    nb, nj = len(bases), len(jobs)
    job_base = np.full(nj, -1, np.int32)
    for j, (b, _) in enumerate(jobs):
        if b is not None:
            if not 0 <= int(b) < nb:
                raise IndexError(f"job {j}: base {b} of {nb}")
            job_base[j] = int(b)
    streams = list(bases) + [own for _, own in jobs]
    lid, *cols = _event_columns(streams)
    off = np.zeros(nb + nj + 1, np.int64)
    np.cumsum(np.bincount(lid, minlength=nb + nj), out=off[1:])
    return RgaOntoBatch(nb, nj, off[:nb + 1].copy(), off[nb:].copy(), job_base, *cols)


def job_columns(batch: RgaOntoBatch) -> Tuple[np.ndarray, np.ndarray]:
    """The jobs' events spelled out: (column index of every event, job by job -- its base's,
    then its own; the jobs' starts in that array, n_jobs + 1)."""
    starts = np.concatenate([[0], np.cumsum(batch.job_len)]).astype(np.int64)
    parts = []
    for j in range(batch.n_jobs):
        b = int(batch.job_base[j])
        if b >= 0:
            parts.append(np.arange(batch.base_off[b], batch.base_off[b + 1], dtype=np.int64))
        parts.append(np.arange(batch.own_off[j], batch.own_off[j + 1], dtype=np.int64))
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), starts


def replay_onto(bases: Sequence[Sequence[Event]], jobs: Sequence[Job]) -> List[List[Any]]:
    """Materialize, for every job (base index or None, own events), the list that its base's
    events followed by its own build -- ``replay([bases[b] + own ...])`` with every base
    marshalled, copied and stored once."""
    from ._lib import rga_replay_onto_device  # the HIP library; raises if missing
    batch = marshal_onto(bases, jobs)
    _, src, offsets = rga_replay_onto_device(batch)
    srcl = src.tolist()
    offl = offsets.tolist()
    return [[batch.values[s] for s in srcl[offl[i]:offl[i + 1]]] for i in range(len(jobs))]


def replay_lists_onto(bases: Sequence[Sequence[Event]], jobs: Sequence[Job]) -> List[List[Elem]]:
    """Every job's final list state, as :func:`replay_lists` returns it for its base's events
    followed by its own."""
    from ._lib import rga_replay_onto_device  # the HIP library; raises if missing
    batch = marshal_onto(bases, jobs)
    _, src, offsets, tomb = rga_replay_onto_device(batch, tombstones=True)
    events = [ev for stream in bases for ev in stream] + [ev for _, own in jobs for ev in own]
    srcl, tl, offl = src.tolist(), tomb.tolist(), offsets.tolist()
    return [[Elem(events[s][1], events[s][2], bool(tb)) for s, tb in
             zip(srcl[offl[i]:offl[i + 1]], tl[offl[i]:offl[i + 1]])] for i in range(len(jobs))]


@dataclass
class RgaChainBatch:
    """Host image of ``smx_rga_chain``: every segment's events once, and the jobs as runs of
    segment indices."""

    n_segs: int
    n_jobs: int
    seg_off: np.ndarray        # i64 [n_segs + 1]
    job_off: np.ndarray        # i64 [n_jobs + 1], into job_seg
    job_seg: np.ndarray        # i32 [n_links], strictly ascending within a job
    op: np.ndarray
    value: np.ndarray
    anchor: np.ndarray
    t: np.ndarray
    author: np.ndarray
    opid_hi: np.ndarray
    opid_lo: np.ndarray
    values: List[Any]          # column index -> value object

    @property
    def n(self) -> int:
        return len(self.op)

    @property
    def n_links(self) -> int:
        return len(self.job_seg)

    @property
    def job_len(self) -> np.ndarray:
        """Events per job: its segments'."""
        csum = np.concatenate([[0], np.cumsum(np.diff(self.seg_off)[self.job_seg])]).astype(np.int64)
        return csum[self.job_off[1:]] - csum[self.job_off[:-1]]

    @property
    def n_out(self) -> int:
        return int(self.job_len.sum())


def _chain_tables(n_segs: int, jobs: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """(job_off, job_seg) of `jobs`; ValueError for a job whose segment indices are out of range
    or do not strictly ascend (the column index breaks ties between equal keys, so a job's
    segments must lie in the columns in the order the job replays them)."""
    job_off = np.zeros(len(jobs) + 1, np.int64)
    links: List[int] = []
    for j, job in enumerate(jobs):
        prev = -1
        for s in job:
            s = int(s)
            if not 0 <= s < n_segs:
                raise ValueError(f"job {j}: segment {s} of {n_segs}")
            if s <= prev:
                raise ValueError(f"job {j}: segment {s} after segment {prev}: indices must strictly ascend")
            prev = s
            links.append(s)
        job_off[j + 1] = len(links)
    return job_off, np.asarray(links, np.int32).reshape(len(links))


def marshal_chain(segments: Sequence[Sequence[Event]], jobs: Sequence[Sequence[int]]) -> RgaChainBatch:
    """The columns of ``smx_rga_replay_chain``: each segment marshalled once, all in one id
    domain (a move or delete in one segment reaches the elements an earlier one created)."""
    ns = len(segments)
    job_off, job_seg = _chain_tables(ns, jobs)  # (before anything is marshalled)
    lid, *cols = _event_columns(segments)
    seg_off = np.zeros(ns + 1, np.int64)
    np.cumsum(np.bincount(lid, minlength=ns), out=seg_off[1:])
    return RgaChainBatch(ns, len(jobs), seg_off, job_off, job_seg, *cols)


def chain_columns(batch: RgaChainBatch) -> Tuple[np.ndarray, np.ndarray]:
    """The jobs' events spelled out: (column index of every event, job by job, segment after
    segment; the jobs' starts in that array, n_jobs + 1)."""
    starts = np.concatenate([[0], np.cumsum(batch.job_len)]).astype(np.int64)
    a, b = int(batch.job_off[0]), int(batch.job_off[-1])
    parts = [np.arange(batch.seg_off[s], batch.seg_off[s + 1], dtype=np.int64) for s in batch.job_seg[a:b].tolist()]
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), starts


def replay_chain(segments: Sequence[Sequence[Event]], jobs: Sequence[Sequence[int]]) -> List[List[Any]]:
    """Materialize, for every job (a strictly ascending sequence of segment indices), the list
    that its segments' events build one segment after another --
    ``replay([sum((segments[s] for s in job), []) for job in jobs])`` with every segment
    marshalled, copied and stored once."""
    from ._lib import rga_replay_chain_device  # the HIP library; raises if missing
    batch = marshal_chain(segments, jobs)
    _, src, offsets = rga_replay_chain_device(batch)
    srcl = src.tolist()
    offl = offsets.tolist()
    return [[batch.values[s] for s in srcl[offl[i]:offl[i + 1]]] for i in range(len(jobs))]


def replay_lists_chain(segments: Sequence[Sequence[Event]], jobs: Sequence[Sequence[int]]) -> List[List[Elem]]:
    """Every job's final list state, as :func:`replay_lists` returns it for its segments' events
    one segment after another."""
    from ._lib import rga_replay_chain_device  # the HIP library; raises if missing
    batch = marshal_chain(segments, jobs)
    _, src, offsets, tomb = rga_replay_chain_device(batch, tombstones=True)
    events = [ev for stream in segments for ev in stream]
    srcl, tl, offl = src.tolist(), tomb.tolist(), offsets.tolist()
    return [[Elem(events[s][1], events[s][2], bool(tb)) for s, tb in
             zip(srcl[offl[i]:offl[i + 1]], tl[offl[i]:offl[i + 1]])] for i in range(len(jobs))]


def replay(streams: Sequence[Sequence[Event]]) -> List[List[Any]]:
    """Materialize every stream (one RGA per stream) on the GPU."""
    from ._lib import rga_replay_device  # the HIP library; raises if missing
    batch = marshal_streams(streams)
    _, src, offsets = rga_replay_device(batch, grouped=True)  # (marshal_streams: stream after stream)
    srcl = src.tolist()
    offl = offsets.tolist()
    return [[batch.values[s] for s in srcl[offl[i]:offl[i + 1]]] for i in range(len(streams))]


def replay_lists(streams: Sequence[Sequence[Event]]) -> List[List[Elem]]:
    """Every stream's final list state (crdt.py:26-27 ``RGA.list``) on the GPU: the
    elements in list order, tombstoned ones included, each as ``Elem(key, value,
    tombstone)`` with the key and value of the event that created it."""
    from ._lib import rga_replay_device  # the HIP library; raises if missing
    batch = marshal_streams(streams)
    _, src, offsets, tomb = rga_replay_device(batch, tombstones=True, grouped=True)
    events = [ev for stream in streams for ev in stream]
    srcl, tl, offl = src.tolist(), tomb.tolist(), offsets.tolist()
    return [[Elem(events[s][1], events[s][2], bool(tb)) for s, tb in
             zip(srcl[offl[i]:offl[i + 1]], tl[offl[i]:offl[i + 1]])] for i in range(len(streams))]


class RGA:
    """Drop-in for crdt.py:23-46: same methods, and ``list`` (crdt.py:26-27) is the
    reference's mutable ``List[Elem]`` state.

    Events are recorded and replayed on the GPU (``smx_rga_replay``) when the state is
    needed.  Reading ``list`` folds the pending events into the state and returns the
    SAME list object on every read, before and after new events, so
    ``rga.list.append(e)`` or ``rga.list[0].tombstone = True`` change the RGA as they do in
    the reference; assigning ``rga.list = L`` makes ``L`` the state, and later events are
    folded into ``L`` itself.  (The reference mutates the object at each call; here a
    held reference sees the events at the next fold: the next read of ``list`` or
    ``materialize()``.)  A later fold replays the state as
    a prefix of the stream (each live element as its insert; each tombstoned one as an
    insert of a private value that is then deleted, so no later event can touch it) and
    keeps the existing ``Elem`` objects: a later ``delete`` sets ``tombstone`` on them in
    place, as crdt.py:40-43 does.  A state the caller put out of key order replays with
    each element keyed by the running maximum of the keys before it (``_effective_keys``):
    the same insert slots as crdt.py:48-57's scan of the list as it stands."""

    def __init__(self) -> None:
        self._events: List[Event] = []
        self._list: "List[Elem] | None" = None  # the state, once read or assigned

    @property
    def list(self) -> List[Elem]:
        if self._list is None or self._events:
            out = self._fold()
            if self._list is None:
                self._list = out
            else:  # the caller's list object is the state (crdt.py:27, 31, 36): fold into it
                self._list[:] = out
            self._events = []
        return self._list

    @list.setter
    def list(self, value: List[Elem]) -> None:
        self._list = value
        self._events = []

    def _fold(self) -> List[Elem]:
        base = self._list or []
        if not base:
            return replay_lists([self._events])[0]
        events = self._events
        while True:
            eff, ordered = _effective_keys(base)
            j = -1 if ordered else next((i for i, ev in enumerate(events) if ev[0] == MOVE), -1)
            if j < 0:
                return _replay_onto(base, eff, events)
            # A list out of key order whose events hold a move: the move's pop can lower
            # the effective keys after it, so the events are replayed up to it, then its pop
            # alone (its insert dropped), and its insert opens the next round on the new list.
            if j:
                base = _replay_onto(base, eff, events[:j])
                eff, _ = _effective_keys(base)
            _, key, value = events[j]
            base = _replay_onto(base, eff, [events[j]], drop_new=True)
            events = [(INSERT, key, value)] + list(events[j + 1:])
    def insert(self, key: Key, value: str) -> None:
        self._events.append((INSERT, key, value))

    def move(self, value: str, key: Key) -> None:
        self._events.append((MOVE, key, value))

    def delete(self, value: str) -> None:
        self._events.append((DELETE, None, value))

    def materialize(self) -> List[str]:
        if self._list is None:
            return replay([self._events])[0]
        return [e.value for e in self.list if not e.tombstone]


def _effective_keys(base: Sequence[Elem]) -> Tuple[List[Key], bool]:
    """Each element's insert key for the replay of a list state, and whether the list is
    in key order.  An insert goes before the first element, in list order, whose key is
    strictly greater (crdt.py:48-57): the first element whose running maximum of keys
    is greater.  So the state replays as inserts keyed by that running maximum -- the
    list's own keys when it is in key order (what insert() and move() keep); the
    running maximum makes a caller-reordered list a key-ordered one with the same
    insert slots, and a new element's maximum is its own key.  Inserts and deletes leave
    the other elements' maxima unchanged; a move's pop may lower them (RGA._fold)."""
    eff: List[Key] = []
    ordered = True
    top = None
    for e in base:
        k = (e.key.anchor, e.key.t, e.key.author, e.key.opid)
        if top is None or k >= top:
            top = k
            eff.append(e.key)
        else:  # (below the running maximum: inserts see the maximum here)
            ordered = False
            eff.append(eff[-1])
    return eff, ordered


def _replay_onto(base: Sequence[Elem], eff: Sequence[Key], events: Sequence[Event],
                 drop_new: bool = False) -> List[Elem]:
    """The list state `base` (insert keys `eff`) followed by `events`, replayed on the
    GPU.  Each live element replays as its insert, each tombstoned one as an insert of
    a private value that is then deleted (no later event can touch it); the existing
    Elem objects are kept (a delete tombstones them in place, crdt.py:40-43), every
    event-created element is a new Elem.  drop_new: leave the event-created elements
    out (a move's pop replayed alone)."""
    stream: List[Event] = []
    origin: List[int] = []  # stream index -> base index (-1: a later event)
    for i, e in enumerate(base):
        if e.tombstone:
            tag = object()  # equal to nothing else: no later move/delete reaches it
            stream.append((INSERT, eff[i], tag))
            stream.append((DELETE, None, tag))
            origin += [i, -1]
        else:
            stream.append((INSERT, eff[i], e.value))
            origin.append(i)
    nb = len(stream)
    stream += list(events)
    src, tomb = _replay_list_src(stream)
    out: List[Elem] = []
    for s, tb in zip(src, tomb):
        if s < nb:
            e = base[origin[s]]
            if tb:
                e.tombstone = True
        elif drop_new:
            continue
        else:
            _, key, value = stream[s]
            e = Elem(key, value, bool(tb))
        out.append(e)
    return out


def _replay_list_src(stream: Sequence[Event]) -> Tuple[List[int], List[int]]:
    """One stream in list mode on the GPU: (creating event index, tombstone) per element
    of the final list, in list order."""
    from ._lib import rga_replay_device  # the HIP library; raises if missing
    batch = marshal_streams([stream])
    _, src, offsets, tomb = rga_replay_device(batch, tombstones=True, grouped=True)
    n = int(offsets[1])
    return src[:n].tolist(), tomb[:n].tolist()
