"""screen_results, the one unpack of a screen's output bytes that ComposeSession.screen and
screen_all share, on a hand-built byte buffer: three pairs with capacities [2, 0, 1]."""
import numpy as np
import pytest

from semantic_merge_amd._lib import SmxError
from semantic_merge_amd._session import screen_results

CONF_AT, COUNTS_AT = 256, 512
CONF_OFF = np.array([0, 2, 2, 3], np.int64)          # capacities 2, 0, 1
PAIRS = np.array([[0, 3], [4, 1], [2, 5]], np.int32)  # (log i, log j) of pair 0, 1, 2
CONF = np.array([[10, 11], [12, 13], [14, 15]], np.int32)


def _buffer(counts):
    hout = np.full(1024, 0xEE, np.uint8)
    hout[CONF_AT: CONF_AT + CONF.nbytes] = CONF.view(np.uint8).reshape(-1)
    c = np.asarray(counts, np.int64)
    hout[COUNTS_AT: COUNTS_AT + c.nbytes] = c.view(np.uint8)
    return hout


def test_full_counts_return_every_slice_as_a_copy():
    hout = _buffer([2, 0, 1])
    res = screen_results(hout, CONF_AT, COUNTS_AT, CONF_OFF, PAIRS)
    assert len(res) == 3 and all(r.dtype == np.int32 and r.ndim == 2 and r.shape[1] == 2 for r in res)
    assert np.array_equal(res[0], CONF[:2]) and res[1].shape == (0, 2) and np.array_equal(res[2], CONF[2:])
    hout[:] = 0  # copies, not views: the staging bytes may be overwritten at once
    assert np.array_equal(res[0], CONF[:2]) and np.array_equal(res[2], CONF[2:])
    assert not any(np.shares_memory(r, hout) for r in res)


def test_fewer_conflicts_than_the_capacity():
    res = screen_results(_buffer([1, 0, 0]), CONF_AT, COUNTS_AT, CONF_OFF, PAIRS)
    assert np.array_equal(res[0], CONF[:1]) and res[1].shape == (0, 2) and res[2].shape == (0, 2)


@pytest.mark.parametrize("p", [0, 1, 2])
def test_a_pair_sent_back_is_none_and_the_others_intact(p):
    counts = [2, 0, 1]
    counts[p] = -2
    res = screen_results(_buffer(counts), CONF_AT, COUNTS_AT, CONF_OFF, PAIRS)
    want = [CONF[:2], CONF[:0], CONF[2:]]
    for i in range(3):
        if i == p:
            assert res[i] is None
        else:
            assert np.array_equal(res[i], want[i])


def test_an_invalid_pair_raises_naming_the_pair_and_both_logs():
    with pytest.raises(SmxError, match=r"pair 1 \(logs 4, 1\): invalid input") as e:
        screen_results(_buffer([2, -1, 1]), CONF_AT, COUNTS_AT, CONF_OFF, PAIRS)
    assert e.value.code == -1


def test_a_count_over_the_capacity_raises_naming_the_pair():
    with pytest.raises(SmxError, match=r"pair 2: 2 conflicts exceed its capacity") as e:
        screen_results(_buffer([2, 0, 2]), CONF_AT, COUNTS_AT, CONF_OFF, PAIRS)
    assert e.value.code == -2
