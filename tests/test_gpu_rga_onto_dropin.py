"""crdt.replay_onto / replay_lists_onto on Key events against the repository's sequential
Python RGA (oracle/rga_list_ref.py) run on each job's base events followed by its own: a dozen
small jobs over a few bases, values of non-string types (interned by _EqClasses, as replay
does) and, in a second case, a non-int t (marshal_streams' rank path)."""
import random

import pytest

from oracle.rga_list_ref import ListRga
from semantic_merge_amd import crdt
from semantic_merge_amd.crdt import DELETE, INSERT, MOVE, Elem, Key

pytestmark = pytest.mark.gpu

VALUES = ["import os", "import sys", "def f", "x = 1", 7, 7.5, (1, "a"), None, ("t",), "class C"]


def _stream(rng, n, ts):
    out = []
    for _ in range(n):
        kind = rng.choice((INSERT, INSERT, INSERT, MOVE, DELETE))
        v = rng.choice(VALUES)
        key = None if kind == DELETE else Key(rng.choice(("", "head", "tail")), rng.choice(ts),
                                              rng.choice(("ann", "bob")), "%032x" % rng.getrandbits(6))
        out.append((kind, key, v))
    return out


def _case(seed, ts):
    rng = random.Random(seed)
    bases = [_stream(rng, n, ts) for n in (25, 0, 8, 40)]
    jobs = [(3, _stream(rng, 12, ts)), (0, _stream(rng, 30, ts)), (None, _stream(rng, 9, ts)), (0, []),
            (2, _stream(rng, 1, ts)), (1, _stream(rng, 6, ts)), (0, _stream(rng, 14, ts)), (None, []),
            (3, _stream(rng, 45, ts)), (2, _stream(rng, 20, ts)), (0, _stream(rng, 3, ts)), (3, []),
            (1, [])]
    return bases, jobs


def _reference(events):
    r = ListRga()
    for kind, key, value in events:
        if kind == INSERT:
            r.insert((key.anchor, key.t, key.author, key.opid), value)
        elif kind == MOVE:
            r.move(value, (key.anchor, key.t, key.author, key.opid))
        else:
            r.delete(value)
    return r.state()


@pytest.mark.parametrize("ts", [(1, 2, 3, 10 ** 12, -5), (0.5, 1, 2.25, -3.0)], ids=["int_t", "ranked_t"])
def test_replay_onto_matches_the_sequential_rga(ts):
    bases, jobs = _case(17, ts)
    assert len(jobs) >= 12
    lists = crdt.replay_lists_onto(bases, jobs)
    mats = crdt.replay_onto(bases, jobs)
    assert len(lists) == len(mats) == len(jobs)
    tombstoned = 0
    for j, (b, own) in enumerate(jobs):
        events = (bases[b] if b is not None else []) + list(own)
        state = _reference(events)
        got = [((e.key.anchor, e.key.t, e.key.author, e.key.opid), e.value, e.tombstone) for e in lists[j]]
        assert all(isinstance(e, Elem) for e in lists[j])
        assert [(k, type(v), v, tb) for k, v, tb in got] == [(k, type(v), v, tb) for k, v, tb in state], f"job {j}"
        live = [v for _, v, tb in state if not tb]
        assert [(type(v), v) for v in mats[j]] == [(type(v), v) for v in live], f"job {j}"
        tombstoned += sum(tb for _, _, tb in state)
    assert tombstoned > 0
    # what the parent commit offers for the same jobs: replay of the concatenated streams
    assert mats == crdt.replay([(bases[b] if b is not None else []) + list(own) for b, own in jobs])


def test_replay_onto_without_jobs_or_bases():
    assert crdt.replay_onto([], []) == [] and crdt.replay_lists_onto([[(INSERT, Key("", 1, "a", "x"), "v")]], []) == []
    own = [(INSERT, Key("", 1, "a", "x"), "v"), (INSERT, Key("", 0, "a", "y"), 3)]
    assert crdt.replay_onto([], [(None, own), (None, [])]) == [[3, "v"], []]
