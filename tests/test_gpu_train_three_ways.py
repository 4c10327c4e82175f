"""The step of a merge train is stated once (csrc/smx_train.h) and run by three forms: one small
train goes through smx_compose_train, through smx_compose_tree as a one-path tree, and through the
host loop of smx_train_stage, smx_compose and smx_train_land.  All three give the same lengths,
outcomes and conflict records step by step and the same final accumulator, and these are the
column-level oracle's (tests/_train.py).  The train: four logs of 40, 25, 25 and 3 ops over 16
symbols with a log index outside the logs in the middle; two steps land, one conflicts, and a move
whose gathered file is the empty string takes v1_alt.  Then train against tree on two logs of
1100 ops: the second step does not fit and is a -2 in both."""
import dataclasses

import numpy as np
import pytest

import _train
import _train_loop as TL
import _tree
from _batch import ADV, MOVE, branch, none_moves
from _pairs import logs_soa

pytestmark = pytest.mark.gpu

N_SYM = 16
SEED = 26


def small_case():
    """(LogsSoA, train, v1_alt, empty_str): a log of moves without values, two logs whose renames
    diverge, a short one; every other move with a file carries the id that stands for the empty
    string."""
    logs = [none_moves(branch(40, N_SYM, SEED, 1, **ADV), 3), branch(25, N_SYM, SEED + 1, 0, **ADV),
            branch(25, N_SYM, SEED + 1, 1, **ADV), branch(3, N_SYM, SEED + 2, 0, **ADV)]
    pool = logs_soa(logs, N_SYM)
    mv = np.flatnonzero((np.asarray(pool.kind) == MOVE) & (np.asarray(pool.v1) >= 0))
    ids = np.unique(np.asarray(pool.v1)[mv])
    empty = int(ids[0])
    v1 = np.array(pool.v1)
    v1[mv[::2]] = empty
    pool = dataclasses.replace(pool, v1=v1)
    alt = np.random.default_rng(3).choice(np.concatenate([ids[1:], [-1]]), pool.n_total).astype(np.int32)
    return pool, [0, 1, len(logs), 2, 3], alt, empty


def same_steps(label, got, want):
    assert len(got) == len(want), f"{label}: {len(got)} steps, not {len(want)}"
    for g, (a, b) in enumerate(zip(got, want)):
        assert tuple(a[:2]) == tuple(b[:2]), f"{label}: step {g}: (length, outcome) {a[:2]}, not {b[:2]}"
        assert np.array_equal(a[2], b[2]), f"{label}: step {g}: conflict records differ"


def same_acc(label, got, want):
    for name, a, b in zip(_train.RES, got, want):
        assert np.array_equal(a, b), f"{label}: {name} differs: {a[:8]} vs {b[:8]} ({len(a)}, {len(b)})"


def path_steps(res):
    """A one-path DeviceTree's results as a train's steps: (length, outcome, records) per node."""
    assert all(r != -1 for r in res), "a node failed structurally"
    return [(r[5], r[6], r[7]) for r in res]


def test_one_small_train_three_ways():
    pool, train, alt, empty = small_case()
    kw = dict(v1_alt=alt, empty_str=empty)
    trace = []
    want = _train.run_train(pool, train, trace=trace, **kw)
    outcomes = [oc for _, oc, _ in want[5]]
    assert outcomes[0] == 0 and outcomes[1] == 0 and outcomes[2] == -1 and outcomes[3] > 0 and outcomes[4] == 0, outcomes
    assert any(TL.staged_values(pool, tr, alt, empty)[2].any() for tr in trace), "no move takes v1_alt"
    assert any((want[f] != _train.NONE).any() for f in (1, 2)), "no entry carries an accumulated value"

    dt, raw = _train.run(pool, [train], **kw)
    by_train = dt.results(raw)[0]
    dn, raw = _tree.run(pool, [(None if g == 0 else g - 1, l) for g, l in enumerate(train)], **kw)
    by_tree = dn.results(raw)
    dl, raw = TL.run(pool, train, **kw)
    by_loop = dl.results(raw)

    # each against the oracle
    same_steps("train", by_train[5], want[5])
    same_steps("tree", path_steps(by_tree), want[5])
    same_steps("loop", by_loop[5], want[5])
    same_acc("train", by_train[:4], want[:4])
    same_acc("tree", by_tree[-1][:4], want[:4])
    same_acc("loop", by_loop[:4], want[:4])
    assert by_train[4] == by_loop[4] == want[4] == 3
    # and against each other
    same_steps("tree against train", path_steps(by_tree), by_train[5])
    same_steps("loop against train", by_loop[5], by_train[5])
    same_acc("tree against train", by_tree[-1][:4], by_train[:4])
    same_acc("loop against train", by_loop[:4], by_train[:4])
    # the tree keeps every landed node's accumulator: the last one that landed is the train's
    assert by_tree[-1][4] == len(train) - 1 and by_tree[3][4] == 1 and by_tree[2][4] == 1


def test_a_step_that_does_not_fit_in_train_and_tree():
    pool = logs_soa([_tree.clean(1100, 21), _tree.clean(1100, 22)], _tree.N_SYM)
    train = [0, 1]
    want = _train.run_train(pool, train)
    assert [(n, oc) for n, oc, _ in want[5]] == [(1100, 0), (1100, -2)]
    dt, raw = _train.run(pool, [train])
    by_train = dt.results(raw)[0]
    dn, raw = _tree.run(pool, [(None, 0), (0, 1)])
    by_tree = dn.results(raw)
    same_steps("train", by_train[5], want[5])
    same_steps("tree against train", path_steps(by_tree), by_train[5])
    same_acc("train", by_train[:4], want[:4])
    same_acc("tree against train", by_tree[-1][:4], by_train[:4])
    assert by_tree[-1][4] == 0 and by_train[4] == 1
