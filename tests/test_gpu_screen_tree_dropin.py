"""screen_tree against the reference's own results (tests/golden/train_cases.json) and
screen_train: every golden train becomes a root path of a tree, the cases of a group joined in one
tree that shares a prefix wherever two trains start with the same logs; per node the conflicts
equal screen_train's last step on the root path, and on the golden paths the positions of the ops
in the golden steps.  Then a tree with a node that compose_tree reports as -2, answered here with
no host loop, the argument checks, empty inputs, and inputs left as they were."""
import pytest

from semantic_merge_amd import compose as compose_mod
from semantic_merge_amd import screen_train, screen_tree

import _screen_tree as T
import _train
from _util import load, to_ops

pytestmark = pytest.mark.gpu
GROUP = 30


@pytest.fixture(scope="module")
def golden():
    raw = load("train_cases.json")
    return raw, [_train.golden_case(c) for c in raw]


def last_steps(logs, nodes):
    """screen_train on every node's root path, spelled out: per node its last step."""
    return [tr[-1] for tr in screen_train(logs, [T.path_of(nodes, n) for n in range(len(nodes))])]


def test_golden_trains_as_paths(golden):
    raw, cases = golden
    shared = evicted = 0
    for g0 in range(0, len(cases), GROUP):
        logs, nodes, ends, owns = T.joined(cases[g0: g0 + GROUP])
        shared += sum(len(e) for e in ends) - len({n for e in ends for n in e})
        before = [[o.to_dict() for o in log] for log in logs]
        got = screen_tree(logs, nodes)
        assert [[o.to_dict() for o in log] for log in logs] == before, f"group {g0}: inputs mutated"
        assert len(got) == len(nodes)
        assert got == last_steps(logs, nodes), f"group {g0}: screen_train on the root paths differs"
        for c, (case, path, own) in enumerate(zip(raw[g0: g0 + GROUP], ends, owns)):
            for n, step in zip(path, case["steps"]):
                want = [((own[a[0]], a[1]), (own[b[0]], b[1])) for a, b in step]
                assert got[n] == want, f"case {g0 + c}: node {n}: the conflicts' ops differ from the reference's"
                evicted += bool(want)
    assert shared > 0, "no two golden trains share a prefix"
    assert evicted > 50


def test_a_node_compose_tree_sends_back(golden, monkeypatch):
    """Two logs of more than 1024 ops on a path: compose_tree reports the second node as -2 and
    runs it and its child by the host loop; screen_tree answers them itself."""
    raw, cases = golden
    case = max(cases[:GROUP], key=lambda c: len(c["out"]))
    logs = [to_ops(x) for x in case["logs"]]
    big = [o for log in logs for o in log] * (1024 // max(sum(len(x) for x in logs), 1) + 1)
    assert 1024 < len(big) <= 2048 - max(len(x) for x in logs)
    L, train = len(logs), case["train"]
    k = len(train)
    nodes = [(n - 1 if n else None, l) for n, l in enumerate(train)]                  # the golden train
    nodes += [(None, L), (k, L + 1), (k + 1, train[0]), (k, train[0])]
    all_logs = logs + [big, big]
    calls = []
    real = compose_mod._train_on_host
    monkeypatch.setattr(compose_mod, "_train_on_host", lambda *a: calls.append(a[1]) or real(*a))
    compose_mod.compose_tree(all_logs, nodes, want=[])
    assert sorted(calls) == sorted([[L, L + 1], [L, L + 1, train[0]]]), "compose_tree: the -2 node and its child"
    del calls[:]
    got = screen_tree(all_logs, nodes)
    assert not calls, "screen_tree went through the host loop"
    assert got == last_steps(all_logs, nodes)
    assert not calls
    for n in (k + 1, k + 2):   # as many conflicts as the host loop finds
        assert len(got[n]) == len(real(all_logs, T.path_of(nodes, n))[1][-1]), f"node {n}"


def test_arguments_and_empties(golden):
    raw, cases = golden
    case = next(c for c in cases if len(c["train"]) >= 4)
    logs = [to_ops(x) for x in case["logs"]]
    nodes = [(n - 1 if n else None, l) for n, l in enumerate(case["train"])]
    before = [[o.to_dict() for o in log] for log in logs]
    got = screen_tree(logs, nodes)
    assert got == screen_train(logs, [case["train"]])[0]
    assert [[o.to_dict() for o in log] for log in logs] == before
    assert screen_tree(logs, []) == [] and screen_tree([], []) == []
    assert screen_tree([[], []], [(None, 0), (0, 1), (None, 1)]) == [[], [], []]
    with pytest.raises(ValueError):
        screen_tree(logs, [(0, 0)])
    for bad in ([(None, len(logs))], [(None, -1)], [(None, 0), (2, 0)]):
        with pytest.raises(IndexError):
            screen_tree(logs, bad)
