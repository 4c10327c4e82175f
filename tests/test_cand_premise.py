"""The fact smx_screen_candidates rests on, pinned against the CPU oracle: a DivergentRename
needs a rename in each log on the same symbol with different names (compose.py:60-70, 88-98), so
a pair of logs without such a symbol has no conflicts in either orientation.  The converse
does not hold: the rule is a prefilter in front of the exact screen, not the answer."""
import numpy as np

from oracle import oracle

import _cand
from _screen import make_log

RENAME = _cand.RENAME
N_LOGS, SPACE = 30, 120


def conflicts(lsoa, i, j):
    return len(oracle.compose(lsoa.pair(i, j))[4]), len(oracle.compose(lsoa.pair(j, i))[4])


def test_non_candidates_have_no_conflicts_and_conflicts_are_candidates():
    lsoa = _cand.sparse_logs(N_LOGS, SPACE, 7)
    pairs, info = _cand.candidates(lsoa)
    assert (info >= 0).all()
    cand = set(map(tuple, pairs.tolist()))
    assert list(map(tuple, pairs.tolist())) == sorted(cand) and all(i < j for i, j in cand)
    total = N_LOGS * (N_LOGS - 1) // 2
    quiet = 0  # candidates without a conflict in either orientation
    for i in range(N_LOGS):
        for j in range(i + 1, N_LOGS):
            ab, ba = conflicts(lsoa, i, j)
            if (i, j) not in cand:
                assert ab == 0 and ba == 0, f"pair ({i}, {j}) is no candidate but conflicts"
            else:
                quiet += ab == 0 and ba == 0
            if ab or ba:
                assert (i, j) in cand, f"pair ({i}, {j}) conflicts but is no candidate"
    # the inputs: pairs on both sides of the rule, and the rule a strict superset of the answer
    assert 4 * (total - len(cand)) >= total, f"{total - len(cand)} of {total} pairs are non-candidates"
    assert 4 * len(cand) >= total, f"{len(cand)} of {total} pairs are candidates"
    assert quiet >= 1, "every candidate conflicts: the inputs do not show the filter to be a superset"


def ren(sym_v0, ts0=1000):
    """A log of renames (sym, v0), one per millisecond."""
    n = len(sym_v0)
    return make_log([RENAME] * n, ts0 + np.arange(n), np.arange(n) + 1, np.arange(n) + 1,
                    [s for s, _ in sym_v0], [v for _, v in sym_v0])


def test_constructed_cases():
    # two logs renaming s to the same name: no candidate, no conflict
    same = _cand.logs_soa([ren([(2, 7)]), ren([(2, 7)], 2000)], 4)
    assert _cand.candidates(same)[0].tolist() == []
    assert conflicts(same, 0, 1) == (0, 0)
    # s to x and then to y, against s to x: a candidate (and the oracle finds the conflict)
    twice = _cand.logs_soa([ren([(2, 7), (2, 8)]), ren([(2, 7)], 1001)], 4)
    assert _cand.candidates(twice)[0].tolist() == [[0, 1]]
    assert sum(conflicts(twice, 0, 1)) > 0
    # other symbols do not matter, and neither does which log comes first
    other = _cand.logs_soa([ren([(1, 7), (3, 9)]), ren([(2, 8), (0, 9)])], 4)
    assert _cand.candidates(other)[0].tolist() == []
    assert conflicts(other, 0, 1) == (0, 0)
