"""The fact smx_screen rests on, pinned against the CPU oracle: the conflict list of a
composition is a function of the two logs' renames alone (T is ordered by precedence first, and
the DivergentRename test fires only between two renames), so dropping every other op changes
nothing but the indices.  And marshal_logs: any two of its logs form the same merge as
marshal(logs[i], logs[j])."""
import numpy as np

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd.marshal import marshal, marshal_logs

from _shapes import pick
from _util import to_ops

RENAME = synth.KIND_RANK["renameSymbol"]
ADV = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)


def renames_only(soa):
    """(the SoA of soa's renames alone, the kept indices of A, those of B)."""
    ka, kb = soa.kind[:soa.n_a] == RENAME, soa.kind[soa.n_a:] == RENAME
    return pick(soa, ka, kb), np.flatnonzero(ka), np.flatnonzero(kb)


def pairs30():
    out = []
    for i in range(30):
        kw = [ADV, dict(ADV, shuffle=True), dict(ADV, ops_per_ms=4096), dict(ADV, ops_per_ms=4096, shuffle=True),
              dict(divergent=0.5), dict(ADV, ops_per_ms=1)][i % 6]
        soa = synth.lift_soa(synth.lift_logs(synth.LiftSpec(60 + 37 * i, 6 + i % 7, 900 + i, **kw)))
        if i in (7, 19):    # an empty side
            a, b = np.ones(soa.n_a, bool), np.ones(soa.n_b, bool)
            soa = pick(soa, a & (i != 7), b & (i != 19))
        out.append(soa)
    return out


def test_conflicts_are_a_function_of_the_renames():
    with_conflicts = 0
    for i, soa in enumerate(pairs30()):
        full = oracle.compose(soa)[4]
        ren, ia, ib = renames_only(soa)
        assert (ren.kind == RENAME).all() and ren.n <= soa.n
        got = oracle.compose(ren)[4]
        mapped = np.stack([ia[got[:, 0]], soa.n_a + ib[got[:, 1] - ren.n_a]], axis=1) if len(got) else got
        assert np.array_equal(mapped, full), f"pair {i}: the renames alone give other conflicts"
        with_conflicts += len(full) > 0
    assert with_conflicts >= 10, "the equality is vacuous: too few pairs have conflicts"


def test_marshal_logs_pairs_compose_as_marshal():
    def logs(n, seed, **kw):
        return [to_ops(d) for d in synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(n, 9, seed, **kw)))]

    ops = logs(160, 1, **ADV) + logs(90, 2, **dict(ADV, shuffle=True)) + [[]] + logs(40, 3)
    before = [[id(o) for o in log] for log in ops]
    lsoa = marshal_logs(ops)
    assert lsoa.n_logs == len(ops) and lsoa.n_total == sum(len(x) for x in ops)
    assert lsoa.log_off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in ops])]).tolist()
    some = 0
    for i in range(len(ops)):
        for j in range(len(ops)):
            pair = lsoa.pair(i, j)
            assert (pair.n_a, pair.n_b) == (len(ops[i]), len(ops[j]))
            want = oracle.compose(marshal(ops[i], ops[j]))[4]
            assert np.array_equal(oracle.compose(pair)[4], want), (i, j)
            some += len(want) > 0
    assert some > 0
    assert before == [[id(o) for o in log] for log in ops]
