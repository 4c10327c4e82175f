"""The CPU RGA oracle (oracle/crdt_ref.c) reproduces the reference RGA's outputs."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd.crdt import DELETE, INSERT, MOVE, Key, marshal_streams

from _util import load

OPS = {"insert": INSERT, "move": MOVE, "delete": DELETE}


def to_streams(cases):
    streams = []
    for case in cases:
        s = []
        for ev in case["events"]:
            if ev[0] == "delete":
                s.append((DELETE, None, ev[1]))
            else:
                s.append((OPS[ev[0]], Key(*ev[2]), ev[1]))
        streams.append(s)
    return streams


def test_rga_oracle_matches_reference():
    cases = load("rga_cases.json")
    b = marshal_streams(to_streams(cases))
    vals, src, offs = oracle.rga(b.n_lists, b.list_id, b.op, b.value, b.anchor, b.t,
                                 b.author, b.opid_hi, b.opid_lo)
    srcl, offl = src.tolist(), offs.tolist()
    for i, case in enumerate(cases):
        got = [b.values[s] for s in srcl[offl[i]:offl[i + 1]]]
        assert got == case["out"], f"rga case {i}"


def _list_ref_script(steps):
    """tools/make_golden.py's RGA mutation scripts on oracle/rga_list_ref.py."""
    from oracle.rga_list_ref import ListRga
    r, held, rec, unordered = ListRga(), None, [], 0
    for st in steps:
        op = st[0]
        if op == "insert":
            r.insert(tuple(st[2]), st[1])
        elif op == "move":
            r.move(st[1], tuple(st[2]))
        elif op == "delete":
            r.delete(st[1])
        elif op == "read":
            rec.append([[list(k), v, tb] for k, v, tb in r.state()])
            ks = [row[0] for row in r.rows]
            unordered += any(b < a for a, b in zip(ks, ks[1:]))
        elif op == "materialize":
            rec.append([v for _, v, tb in r.state() if not tb])
        elif op == "append":
            r.rows.append([tuple(st[1]), st[2], st[3]])
        elif op == "pop":
            r.rows.pop(st[1])
        elif op == "set_tomb":
            r.rows[st[1]][2] = st[2]
        elif op == "assign":
            r.rows = [[tuple(k), v, tb] for k, v, tb in st[1]]
        elif op == "hold":
            held = r.rows[st[1]]
        elif op == "held":
            rec.append(None if held is None else held[2])
    return rec, unordered


def test_list_ref_matches_reference_mutation_scripts():
    """oracle/rga_list_ref.py (the list-state checker of the GPU RGA class) reproduces
    the reference RGA's results on the 300 mutation scripts (appends, pops, tombstone
    flips, assignments, held elements).  Those scripts keep their lists in key order, so
    for states out of key order the checker rests on its line-by-line restatement of
    crdt.py:29-57 (no reference output covers them)."""
    for i, case in enumerate(load("rga_mutation_cases.json")):
        rec, _ = _list_ref_script(case["steps"])
        assert rec == case["out"], f"mutation script {i}"


def test_effective_keys_give_the_scan_slot():
    """crdt._effective_keys: on a list in any order, the slot of crdt.py:48-57's scan
    (before the first strictly greater key) is the upper bound of the new key among
    the running-maximum keys -- the slot the device replay of a key-ordered list takes."""
    import bisect
    import random
    from semantic_merge_amd.crdt import Elem, _effective_keys
    rnd = random.Random(5)
    tup = lambda k: (k.anchor, k.t, k.author, k.opid)
    for _ in range(500):
        base = [Elem(Key(rnd.choice("abc"), rnd.randrange(3), "u", "o"), "v") for _ in range(rnd.randrange(8))]
        eff, ordered = _effective_keys(base)
        ks = [tup(e.key) for e in base]
        assert ordered == all(a <= b for a, b in zip(ks, ks[1:]))
        assert [tup(k) for k in eff] == sorted(tup(k) for k in eff)  # non-decreasing
        for _ in range(5):
            k = (rnd.choice("abcd"), rnd.randrange(4), "u", "o")
            scan = next((i for i, x in enumerate(ks) if k < x), len(ks))
            assert scan == bisect.bisect_right([tup(x) for x in eff], k)


def test_rga_oracle_list_mode_matches_reference():
    """The oracle's list mode (out_tomb given) is the reference's own RGA.list after each
    golden stream: keys, values and tombstones of every element, in list order."""
    cases = load("rga_cases.json")
    want = load("rga_list_cases.json")
    streams = to_streams(cases)
    b = marshal_streams(streams)
    vals, src, offs, tomb = oracle.rga(b.n_lists, b.list_id, b.op, b.value, b.anchor, b.t,
                                       b.author, b.opid_hi, b.opid_lo, tombstones=True)
    assert len(vals) == len(src) == len(tomb) == offs[-1]
    assert tomb.sum() > 100 and (~tomb).sum() > 100
    events = [ev for s in streams for ev in s]
    srcl, tl, offl = src.tolist(), tomb.tolist(), offs.tolist()
    for i, w in enumerate(want):
        got = []
        for s, tb in zip(srcl[offl[i]:offl[i + 1]], tl[offl[i]:offl[i + 1]]):
            _, k, v = events[s]
            got.append([[k.anchor, k.t, k.author, k.opid], v, tb])
        assert got == w, f"rga list case {i}"
    # materialize mode is the same state without the tombstoned elements
    mv, ms, mo = oracle.rga(b.n_lists, b.list_id, b.op, b.value, b.anchor, b.t, b.author, b.opid_hi, b.opid_lo)
    assert ms.tolist() == [s for s, tb in zip(srcl, tl) if not tb]
    assert mv.tolist() == [v for v, tb in zip(vals.tolist(), tl) if not tb]
    assert mo.tolist() == [0] + np.cumsum([sum(1 for tb in tl[offl[i]:offl[i + 1]] if not tb)
                                           for i in range(b.n_lists)]).tolist()


class _Val:
    """A value that compares by its id and remembers the event that carried it."""
    __slots__ = ("v", "i")

    def __init__(self, v, i):
        self.v, self.i = v, i

    def __eq__(self, other):
        return self.v == other.v

    __hash__ = None


@pytest.mark.parametrize("regime", ["narrow", "wide"])
def test_rga_oracle_list_mode_matches_list_ref_on_ties(regime):
    """Past the golden streams' 40 events: the oracle's list state equals the pure-Python
    restatement oracle/rga_list_ref.py on the tie-heavy batch (lists of 0 to 5000 events,
    keys tied at every level), list by list: creating events, values and tombstones."""
    from oracle.rga_list_ref import ListRga
    import _rga_shapes as shapes
    b = shapes.tie_batch(regime=regime)
    vals, src, offs, tomb = oracle.rga(*shapes.args(b), tombstones=True)
    shapes.assert_ties(b, src, offs)
    refs = [ListRga() for _ in range(b.n_lists)]
    cols = [c.tolist() for c in (b.list_id, b.op, b.value, b.anchor, b.t, b.author, b.opid_hi, b.opid_lo)]
    for i, (l, op, v, an, t, au, hi, lo) in enumerate(zip(*cols)):
        if op == INSERT:
            refs[l].insert((an, t, au, (hi, lo)), _Val(v, i))
        elif op == MOVE:
            refs[l].move(_Val(v, i), (an, t, au, (hi, lo)))
        else:
            refs[l].delete(_Val(v, i))
    assert tomb.any() and not tomb.all()
    for l, ref in enumerate(refs):
        a, e = int(offs[l]), int(offs[l + 1])
        st = ref.state()
        assert src[a:e].tolist() == [v.i for _, v, _ in st], f"list {l}"
        assert vals[a:e].tolist() == [v.v for _, v, _ in st], f"list {l}"
        assert tomb[a:e].tolist() == [tb for _, _, tb in st], f"list {l}"
    assert offs[-1] == len(src)
