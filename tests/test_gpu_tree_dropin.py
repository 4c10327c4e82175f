"""compose_tree against the reference's own results (tests/golden/train_cases.json) and the host
loop: every golden train becomes a root path of a tree, the cases of a group joined in one tree
that shares a prefix wherever two trains start with the same logs; the leaves must equal the
golden ops and conflicts as dicts, and with want="all" every inner node the host loop over
compose_oplogs.  Then a tree with a node the device reports as -2, whose subtree is computed by
the host loop, the argument checks, `want` as indices, and inputs left as they were."""
import json

import pytest

from semantic_merge_amd import compose_tree
from semantic_merge_amd import compose as compose_mod

import _train
from _util import load, to_ops

pytestmark = pytest.mark.gpu
GROUP = 30


@pytest.fixture(scope="module")
def cases():
    return [_train.golden_case(c) for c in load("train_cases.json")]


def dicts(ops):
    return None if ops is None else [o.to_dict() for o in ops]


def joined(group):
    """The cases of `group` as one tree: (logs, nodes, ends, extra).  Logs of equal content are
    pooled once, the trains are inserted into a trie, so that trains that start with the same
    logs share those nodes; ends[c]: the nodes of case c's train, root first.  Each train of two
    logs or more comes a second time with its last two logs swapped: a sibling path under the
    shared prefix, whose nodes are `extra`."""
    logs, where, nodes, child, ends, extra = [], {}, [], {}, [], []

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
        train = [own[l] for l in case["train"]]
        ends.append(walk(train))
        if len(train) >= 2:
            extra += walk(train[:-2] + [train[-1], train[-2]])[-2:]
    return logs, nodes, ends, extra


def test_golden_trains_as_paths(cases):
    shared = evicted = 0
    for g0 in range(0, len(cases), GROUP):
        group = cases[g0: g0 + GROUP]
        logs, nodes, ends, extra = joined(group)
        shared += sum(len(e) for e in ends) - len({n for e in ends for n in e})
        before = [[o.to_dict() for o in log] for log in logs]
        parents = {p for p, _ in nodes}
        got = compose_tree(logs, nodes)
        assert [[o.to_dict() for o in log] for log in logs] == before, f"group {g0}: inputs mutated"
        assert len(got) == len(nodes)
        for n, (ops, _) in enumerate(got):
            assert (ops is None) == (n in parents), f"group {g0}: node {n}: ops for the leaves alone"
        for c, (case, path) in enumerate(zip(group, ends)):
            if not path:
                continue
            steps = [[x.to_dict() for x in got[n][1]] for n in path]
            assert steps == case["steps"], f"case {g0 + c}: conflicts differ from the reference's"
            evicted += sum(1 for s in steps if s)
            if path[-1] not in parents:
                assert dicts(got[path[-1]][0]) == case["out"], f"case {g0 + c}: the leaf's ops differ from the reference's"
    assert shared > 0, "no two golden trains share a prefix"
    assert evicted > 50


def test_every_node_equals_the_host_loop(cases):
    logs, nodes, ends, extra = joined(cases[:GROUP])
    assert extra
    got = compose_tree(logs, nodes, want="all")
    for c, (case, path) in enumerate(zip(cases[:GROUP], ends)):
        if path:
            assert dicts(got[path[-1]][0]) == case["out"], f"case {c}: the train's ops differ from the reference's"
    for n in range(len(nodes)):
        path, up = [], n
        while up is not None:
            path.append(nodes[up][1])
            up = nodes[up][0]
        out, steps = compose_mod._train_on_host(logs, path[::-1])
        assert dicts(got[n][0]) == dicts(out), f"node {n}: ops differ from the host loop's"
        assert [x.to_dict() for x in got[n][1]] == [x.to_dict() for x in steps[-1]], f"node {n}: conflicts differ"


def test_a_subtree_through_the_host_path(cases, monkeypatch):
    """Two logs of more than 1024 ops on a path: the second node is reported as -2.  That node
    and the nodes below it, and only those, are run by the host loop, and equal it."""
    case = max(cases[:GROUP], key=lambda c: len(c["out"]))
    logs = [to_ops(x) for x in case["logs"]]
    big = [o for log in logs for o in log] * (1024 // max(sum(len(x) for x in logs), 1) + 1)
    assert 1024 < len(big) <= 2048 - max(len(x) for x in logs)
    L = len(logs)
    train = case["train"]
    nodes = [(n - 1 if n else None, l) for n, l in enumerate(train)]                  # the golden train
    nodes += [(None, L), (len(train), L + 1), (len(train) + 1, train[0]), (len(train), train[0])]
    calls = []
    real = compose_mod._train_on_host
    monkeypatch.setattr(compose_mod, "_train_on_host", lambda *a: calls.append(a[1]) or real(*a))
    got = compose_tree(logs + [big, big], nodes, want="all")
    assert sorted(calls) == sorted([[L, L + 1], [L, L + 1, train[0]]]), "exactly the -2 node and its child"
    k = len(train)
    assert dicts(got[k - 1][0]) == case["out"]
    assert [[x.to_dict() for x in got[n][1]] for n in range(k)] == case["steps"]
    for n, path in ((k, [L]), (k + 1, [L, L + 1]), (k + 2, [L, L + 1, train[0]]), (k + 3, [L, train[0]])):
        out, steps = real(logs + [big, big], path)
        assert dicts(got[n][0]) == dicts(out), f"node {n}"
        assert [x.to_dict() for x in got[n][1]] == [x.to_dict() for x in steps[-1]], f"node {n}"


def test_want_and_arguments(cases):
    case = next(c for c in cases if len(c["train"]) >= 4)
    logs = [to_ops(x) for x in case["logs"]]
    nodes = [(n - 1 if n else None, l) for n, l in enumerate(case["train"])]
    full = compose_tree(logs, nodes, want="all")
    some = compose_tree(logs, nodes, want=[1, 3])
    for n in range(len(nodes)):
        assert dicts(some[n][0]) == (dicts(full[n][0]) if n in (1, 3) else None)
        assert [x.to_dict() for x in some[n][1]] == [x.to_dict() for x in full[n][1]]
    assert [dicts(r[0]) is not None for r in compose_tree(logs, nodes)] == [False] * (len(nodes) - 1) + [True]
    assert compose_tree(logs, []) == [] and compose_tree([], []) == []
    with pytest.raises(ValueError):
        compose_tree(logs, [(0, 0)])
    with pytest.raises(ValueError):
        compose_tree(logs, nodes, want="inner")
    for bad in ([(None, len(logs))], [(None, -1)], [(None, 0), (2, 0)]):
        with pytest.raises(IndexError):
            compose_tree(logs, bad)
    with pytest.raises(IndexError):
        compose_tree(logs, nodes, want=[len(nodes)])
