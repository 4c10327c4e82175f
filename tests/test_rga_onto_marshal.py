"""crdt.marshal_onto without a GPU: every base is stored once, base_off / own_off / job_base
are what smx_rga_onto specifies (the bases before the own events), bases and own streams share
one id domain, and the CPU oracle on the expanded batch gives, job by job, what it gives on
crdt.marshal_streams of the concatenated streams (compared by value objects: the two marshals
intern in different orders)."""
import random

import numpy as np

from oracle import oracle
from semantic_merge_amd import crdt
from semantic_merge_amd.crdt import DELETE, INSERT, MOVE, Key

import _rga_onto as onto
import _rga_shapes as shapes


def _stream(rng, n, values, anchors=("a", "b"), authors=("x", "y"), ts=(1, 2, 3)):
    out = []
    for _ in range(n):
        kind = rng.choice((INSERT, INSERT, MOVE, DELETE))
        v = rng.choice(values)
        key = None if kind == DELETE else Key(rng.choice(anchors), rng.choice(ts), rng.choice(authors),
                                              "%032x" % rng.getrandbits(12))
        out.append((kind, key, v))
    return out


def _case(seed=5, ts=(1, 2, 3)):
    rng = random.Random(seed)
    values = ["v%d" % i for i in range(6)] + [7, (1, 2), 2.5]
    bases = [_stream(rng, n, values, ts=ts) for n in (12, 0, 30, 5)]
    jobs = [(2, _stream(rng, 9, values, ts=ts)), (None, _stream(rng, 7, values, ts=ts)), (0, []),
            (0, _stream(rng, 20, values, ts=ts)), (1, _stream(rng, 4, values, ts=ts)), (None, []),
            (2, _stream(rng, 15, values, ts=ts)), (0, _stream(rng, 3, values, ts=ts))]  # (base 3: named by no job)
    return bases, jobs


def test_bases_are_stored_once_and_before_the_own_events():
    bases, jobs = _case()
    b = crdt.marshal_onto(bases, jobs)
    nb, nj = len(bases), len(jobs)
    assert (b.n_bases, b.n_jobs) == (nb, nj)
    assert b.n == sum(map(len, bases)) + sum(len(own) for _, own in jobs)  # not once per job
    assert b.base_off.dtype == np.int64 and b.own_off.dtype == np.int64 and b.job_base.dtype == np.int32
    assert b.base_off.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in bases])]).tolist()
    assert b.own_off.tolist() == (b.base_off[-1] + np.concatenate([[0], np.cumsum([len(o) for _, o in jobs])])).tolist()
    assert b.base_off[-1] <= b.own_off[0] and b.own_off[-1] == b.n
    assert b.job_base.tolist() == [-1 if base is None else base for base, _ in jobs]
    for col, dt in ((b.op, np.uint8), (b.value, np.uint32), (b.anchor, np.uint32), (b.t, np.int64),
                    (b.author, np.uint32), (b.opid_hi, np.uint64), (b.opid_lo, np.uint64)):
        assert col.dtype == dt and col.shape == (b.n,)
    events = [ev for s in bases for ev in s] + [ev for _, own in jobs for ev in own]
    assert b.op.tolist() == [ev[0] for ev in events] and b.values == [ev[2] for ev in events]
    assert b.n_out == sum((len(bases[base]) if base is not None else 0) + len(own) for base, own in jobs)
    idx, starts = crdt.job_columns(b)
    assert starts.tolist() == np.concatenate([[0], np.cumsum(b.job_len)]).tolist() and idx.size == b.n_out
    for j, (base, own) in enumerate(jobs):
        want = (bases[base] if base is not None else []) + list(own)
        assert [events[c] for c in idx[starts[j]:starts[j + 1]]] == want


def test_one_id_domain_across_bases_and_own_streams():
    bases, jobs = _case()
    b = crdt.marshal_onto(bases, jobs)
    events = [ev for s in bases for ev in s] + [ev for _, own in jobs for ev in own]
    nbase = int(b.base_off[-1])
    for name, col, of in (("value", b.value, lambda ev: ev[2]),
                          ("anchor", b.anchor, lambda ev: ev[1].anchor if ev[1] else ""),
                          ("author", b.author, lambda ev: ev[1].author if ev[1] else "")):
        ids = {}
        for c, ev in enumerate(events):
            k = (type(of(ev)).__name__, of(ev))
            assert ids.setdefault(k, int(col[c])) == int(col[c]), f"{name} {k}: two ids"
        assert len(set(ids.values())) == len(ids), f"{name}: two objects share an id"
        in_base = {k for c, k in enumerate((type(of(ev)).__name__, of(ev)) for ev in events) if c < nbase}
        in_own = {k for c, k in enumerate((type(of(ev)).__name__, of(ev)) for ev in events) if c >= nbase}
        assert in_base & in_own, f"{name}: the case shares none between a base and an own stream"
    a_rank = {a: int(b.anchor[c]) for c, ev in enumerate(events) if ev[1] for a in [ev[1].anchor]}
    assert sorted(a_rank, key=a_rank.get) == sorted(a_rank)  # order-preserving over the whole call


def _by_job_values(batch_values, vals_src, offs, tomb, col_of=None):
    src = vals_src if col_of is None else col_of[vals_src]
    return [[(batch_values[s], bool(tb)) for s, tb in zip(src[offs[j]:offs[j + 1]], tomb[offs[j]:offs[j + 1]])]
            for j in range(len(offs) - 1)]


def test_expanded_batch_equals_concatenated_streams():
    for ts in ((1, 2, 3), (0.5, 1, 2.25)):  # int t; a non-int t: marshal_streams' rank path
        bases, jobs = _case(seed=9, ts=ts)
        b = crdt.marshal_onto(bases, jobs)
        ex, idx = onto.expand(b)
        _, src, offs, tomb = oracle.rga(*shapes.args(ex), tombstones=True)
        got = _by_job_values(b.values, src, offs, tomb, idx)
        ref = crdt.marshal_streams([(bases[base] if base is not None else []) + list(own) for base, own in jobs])
        _, rsrc, roffs, rtomb = oracle.rga(*shapes.args(ref), tombstones=True)
        want = _by_job_values(ref.values, rsrc, roffs, rtomb)
        assert got == want
        assert any(tb for job in want for _, tb in job) and any(not tb for job in want for _, tb in job)


def test_marshal_onto_rejects_a_base_out_of_range():
    bases, jobs = _case()
    for bad in (len(bases), -1):
        try:
            crdt.marshal_onto(bases, jobs + [(bad, [])])
        except IndexError:
            continue
        raise AssertionError(f"base {bad} accepted")


def test_marshal_streams_is_unchanged():
    """marshal_streams and marshal_onto share their column builder: a batch with no bases is
    marshal_streams' batch, column by column."""
    bases, jobs = _case()
    streams = [own for _, own in jobs]
    a = crdt.marshal_streams(streams)
    b = crdt.marshal_onto([], [(None, s) for s in streams])
    assert a.n_lists == len(streams) and a.list_id.tolist() == np.repeat(np.arange(len(streams)),
                                                                         [len(s) for s in streams]).tolist()
    for name in ("op", "value", "anchor", "t", "author", "opid_hi", "opid_lo"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.values == b.values and b.base_off.tolist() == [0] and b.n_out == a.n
