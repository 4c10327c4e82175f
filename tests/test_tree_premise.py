"""The premise of smx_compose_tree on the oracle alone, and the host's level-order function.
The premise: a node's result depends on its parent's accumulator and its own log only, so
carrying the state from parent to child, node by node, gives at every node of a tree what
`_train.run_train` gives on the node's whole root path; a node that does not land leaves its
parent's state to its children.  tree_levels: the permutation into level order, level_off, the
way back, and the errors of a malformed tree."""
import numpy as np
import pytest

from semantic_merge_amd._session import tree_levels

import _train
import _tree
from _tree import IX, SEEDS, random_nodes


@pytest.fixture(scope="module")
def pool():
    return _tree.make_pool()


@pytest.mark.parametrize("seed", SEEDS)
def test_carried_state_equals_the_whole_path(pool, seed):
    nodes = random_nodes(seed)
    empty = tuple(np.zeros(0, np.int32) for _ in range(4))
    state, outcome, below_conflict, conflicting_with_landed_child = {}, {}, {}, False
    for n, (p, l) in enumerate(nodes):
        state[n], step = _tree.carry_step(pool, empty if p is None else state[p], l)
        path = []
        up = n
        while up is not None:
            path.append(nodes[up][1])
            up = nodes[up][0]
        w = _train.run_train(pool, path[::-1])
        for g, r in zip(state[n], w[:4]):
            assert np.array_equal(g, r), (seed, n)
        assert step[:2] == w[5][-1][:2] and np.array_equal(step[2], w[5][-1][2]), (seed, n)
        below_conflict[n] = p is not None and (below_conflict[p] or outcome[p] > 0)
        outcome[n] = step[1]
        if step[1] != 0:  # it did not land: the parent's state, the very arrays
            assert state[n] is (empty if p is None else state[p])
        elif below_conflict[n] and len(pool.log_off) and l != IX["empty"]:
            conflicting_with_landed_child = True
    assert conflicting_with_landed_child, "no conflicting node with a landed descendant: the seed shows nothing"


def test_level_order():
    parents = [None, None, 0, 1, 0, 2, None, 5, 3]
    order, level_off, back = tree_levels(parents)
    assert order.tolist() == [0, 1, 6, 2, 3, 4, 5, 8, 7]
    assert level_off.tolist() == [0, 3, 6, 8, 9] and level_off.dtype == np.int64
    assert sorted(order.tolist()) == list(range(9))
    assert back[order].tolist() == list(range(9)) and order[back].tolist() == list(range(9))
    depth = np.searchsorted(level_off, back, "right") - 1
    for n, p in enumerate(parents):
        assert depth[n] == (0 if p is None else depth[p] + 1)
    # -1 names a root too; a star, a path, no node
    assert tree_levels([-1, None, -1])[1].tolist() == [0, 3]
    assert tree_levels([None, 0, 1, 2])[1].tolist() == [0, 1, 2, 3, 4]
    order, level_off, back = tree_levels([])
    assert len(order) == 0 and level_off.tolist() == [0] and len(back) == 0
    for seed in range(5):
        nodes = random_nodes(seed)
        order, level_off, back = tree_levels([p for p, _ in nodes])
        assert len(level_off) - 1 <= 6 and back[order].tolist() == list(range(len(nodes)))
        assert (np.diff(level_off) > 0).all()


def test_level_order_errors():
    for parents in ([0], [None, 1], [None, 2, 1], [1, None]):
        with pytest.raises(ValueError):
            tree_levels(parents)
    for parents in ([None, 5], [-2], [None, None, 3]):
        with pytest.raises(IndexError):
            tree_levels(parents)
