"""The drop-in compose_train on the GPU against the reference's host loop with eviction
(tests/golden/train_cases.json): per train the ops the last landed step leaves and per step the
conflicts, as dicts; all the golden trains in few calls, one call with trains over shared logs,
one train forced through the host path (a step the device reports as -2), the argument checks,
and inputs left as they were."""
import pytest

from semantic_merge_amd import compose_train
from semantic_merge_amd import compose as compose_mod

import _train
from _util import load, to_ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return [_train.golden_case(c) for c in load("train_cases.json")]


def as_dicts(res):
    out, steps = res
    return [o.to_dict() for o in out], [[c.to_dict() for c in s] for s in steps]


def test_golden_trains(cases):
    evicted = 0
    for c, case in enumerate(cases):
        logs = [to_ops(x) for x in case["logs"]]
        before = [[o.to_dict() for o in log] for log in logs]
        trains = [case["train"], case["train"][:1], list(reversed(case["train"]))]
        got = compose_train(logs, trains)
        assert [[o.to_dict() for o in log] for log in logs] == before, f"case {c}: inputs mutated"
        assert len(got) == 3
        out, steps = as_dicts(got[0])
        assert out == case["out"], f"case {c}: the train's ops differ from the reference's"
        assert steps == case["steps"], f"case {c}: conflicts differ"
        assert as_dicts(got[1])[1] == [[]]
        evicted += sum(1 for s in steps if s)
        if case["train"] == list(range(len(logs))):
            assert as_dicts(compose_train(logs)[0]) == (out, steps)
    assert evicted > 50


def test_a_train_through_the_host_path(cases, monkeypatch):
    """A train that starts with two logs of more than 1024 ops holds a step the device reports as
    -2 (accumulator plus log over 2048 ops): that train, and only that one, is run by the host
    loop, and equals it."""
    case = max(cases, key=lambda c: len(c["out"]))
    logs = [to_ops(x) for x in case["logs"]]
    calls = []
    real = compose_mod._train_on_host
    monkeypatch.setattr(compose_mod, "_train_on_host", lambda *a: calls.append(1) or real(*a))
    big = [o for log in logs for o in log] * (2048 // max(sum(len(x) for x in logs), 1) + 1)
    got = compose_train(logs + [big, big], [case["train"], [len(logs), len(logs) + 1] + case["train"]])
    assert calls == [1], "exactly the second train holds a step of -2"
    assert as_dicts(got[0]) == (case["out"], case["steps"])
    want = real(logs + [big, big], [len(logs), len(logs) + 1] + case["train"])
    assert as_dicts(got[1]) == as_dicts(want)


def test_arguments(cases):
    logs = [to_ops(x) for x in cases[0]["logs"]]
    assert compose_train(logs, []) == []
    assert compose_train([], None) == [([], [])]
    with pytest.raises(IndexError):
        compose_train(logs, [[0, len(logs)]])
    with pytest.raises(IndexError):
        compose_train(logs, [[-1]])
