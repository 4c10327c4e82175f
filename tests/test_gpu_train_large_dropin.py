"""compose_train(logs, trains, large=True) on the GPU against the host loop it replaces
(_train_on_host: compose_oplogs with eviction), as dicts: the train of
test_a_train_through_the_host_path, whose second train holds a step over 2048 ops, and golden
trains behind a filler log that puts every step over the limit.  The host loop is not called,
inputs are left as they were, and large=True on trains that fit is large=False."""
import pytest

from semantic_merge_amd import compose as compose_mod
from semantic_merge_amd import compose_train

import _train
import _train_loop as TL
from _util import load, to_ops

pytestmark = pytest.mark.gpu

GOLDEN_EVERY = 10


@pytest.fixture(scope="module")
def cases():
    return [_train.golden_case(c) for c in load("train_cases.json")]


def as_dicts(res):
    out, steps = res
    return [o.to_dict() for o in out], [[c.to_dict() for c in s] for s in steps]


@pytest.fixture()
def host_calls(monkeypatch):
    """_train_on_host patched to count its calls: .seen has one entry per call, .real is the loop."""
    import types
    box = types.SimpleNamespace(seen=[], real=compose_mod._train_on_host)
    monkeypatch.setattr(compose_mod, "_train_on_host", lambda *a: box.seen.append(1) or box.real(*a))
    return box


def test_the_host_path_train_on_the_gpu(cases, host_calls):
    case = max(cases, key=lambda c: len(c["out"]))
    logs = [to_ops(x) for x in case["logs"]]
    big = [o for log in logs for o in log] * (2048 // max(sum(len(x) for x in logs), 1) + 1)
    every = logs + [big, big]
    trains = [case["train"], [len(logs), len(logs) + 1] + case["train"]]
    before = [[o.to_dict() for o in log] for log in every]
    got = compose_train(every, trains, large=True)
    assert host_calls.seen == [], "large=True keeps the train on the GPU"
    assert [[o.to_dict() for o in log] for log in every] == before, "inputs mutated"
    assert as_dicts(got[0]) == (case["out"], case["steps"])
    assert as_dicts(got[1]) == as_dicts(host_calls.real(every, trains[1]))
    # without the flag the second train, and only that one, goes through the host loop
    plain = compose_train(every, trains)
    assert host_calls.seen == [1]
    assert [as_dicts(r) for r in plain] == [as_dicts(r) for r in got]


def test_golden_trains_behind_a_filler(cases, host_calls):
    evicted = 0
    for c in range(0, len(cases), GOLDEN_EVERY):
        dicts, train = TL.fronted(cases[c], c)
        logs = [to_ops(x) for x in dicts]
        before = [[o.to_dict() for o in log] for log in logs]
        got = compose_train(logs, [train, cases[c]["train"]], large=True)
        assert host_calls.seen == [], f"case {c}: the host loop ran"
        assert [[o.to_dict() for o in log] for log in logs] == before, f"case {c}: inputs mutated"
        out, steps = as_dicts(got[0])
        assert (out, steps) == as_dicts(host_calls.real(logs, train)), f"case {c}: differs from the host loop"
        # the filler lands first and conflicts with nothing: behind it the reference's own train
        assert steps == [[]] + cases[c]["steps"], f"case {c}: conflicts differ from the reference's"
        assert len(out) == TL.FILLER_OPS + len(cases[c]["out"])
        assert as_dicts(got[1]) == (cases[c]["out"], cases[c]["steps"])
        evicted += sum(1 for s in steps if s)
    assert evicted >= 3


def test_large_on_trains_that_fit_is_the_plain_call(cases, host_calls):
    for c in (0, 7, 33):
        logs = [to_ops(x) for x in cases[c]["logs"]]
        trains = [cases[c]["train"], list(reversed(cases[c]["train"]))]
        assert [as_dicts(r) for r in compose_train(logs, trains, large=True)] == \
            [as_dicts(r) for r in compose_train(logs, trains)]
    assert host_calls.seen == []
    assert compose_train([], None, large=True) == [([], [])]
    assert compose_train([to_ops(x) for x in cases[0]["logs"]], [], large=True) == []
