"""One ComposeSession reused across every kind of call while its staging areas grow: each
result equals the same call's on a fresh session (which the neighbouring files hold against
the oracle), and a call of a size already seen allocates nothing."""
import numpy as np
import pytest

from semantic_merge_amd import synth
from semantic_merge_amd._lib import ComposeSession

import _cand
from _batch import ADV, branch, own_logs, shared_soa

pytestmark = pytest.mark.gpu


def merge(n, seed):
    return synth.lift_soa(synth.lift_logs(synth.LiftSpec(n, max(n // 10, 4), seed, **ADV)))


def same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def buffers(sess):
    """The addresses of both areas' four buffers and of the workspace."""
    return [t.data_ptr() for area in (sess.main, sess.aux) for t in (area.h_in, area.d_in, area.h_out, area.d_out)] \
        + [sess.ws.data_ptr()]


def test_one_session_across_every_call_kind_while_its_areas_grow():
    m40 = merge(40, 3)
    six = _cand.sparse_logs(6, 10, 21, lo=26, hi=35)       # 6 logs of about 30 ops, few symbols: conflicts
    twelve = _cand.sparse_logs(12, 16, 22, lo=280, hi=321)  # 12 logs of about 300 ops
    many = [merge(10, 4), merge(200, 5), merge(2048, 6)]
    four = [(0, 1), (4, 2), (1, 5), (3, 0)]
    n_sym = 12
    ssoa = shared_soa(branch(50, n_sym, 6, 0, **ADV), own_logs(n_sym, 300, [20, 35, 60]), n_sym)
    calls = [
        lambda s: s.compose(m40),
        lambda s: s.screen_all(six),
        lambda s: s.compose_many(many),
        lambda s: s.screen(six, four),
        lambda s: s.compose_shared(ssoa),
        lambda s: s.screen_all(twelve),
        lambda s: s.candidates(twelve, start_cap=1),
        lambda s: s.compose(m40),
    ]
    sess = ComposeSession()
    for step, call in enumerate(calls, 1):
        before = buffers(sess) if step > 2 else None
        got, want = call(sess), call(ComposeSession())
        assert same(got, want), f"step {step}: the reused session differs from a fresh one"
        if step == 2:
            assert sum(len(c) > 0 for c in got[1]) >= 2, "fewer than two conflicting pairs among the 6 logs"
        if step == 6:
            # the 12 logs' columns outgrow the main input (3582 ops of 33 bytes against the 2258 ops of
            # step 3) and their conflict capacities the auxiliary output (its 4096-byte floor until now);
            # conf_off for 66 pairs fits the auxiliary input's floor, the 66 pairs the main output
            grew = [a != b for a, b in zip(before, buffers(sess))]
            assert len(got[0]) > 0 and grew[0] and grew[1], "the main input area did not grow"
            assert grew[6] and grew[7], "the auxiliary output area did not grow"
            before = buffers(sess)
            assert same(call(sess), want) and buffers(sess) == before, "a size already seen allocated again"
        if step == 7:
            assert sess.last["retries"] == 1 and len(got) > 1
