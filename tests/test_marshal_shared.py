"""marshal_shared on the CPU: one pass over a shared log and its branch logs, one symbol /
string / equality-class table and one timestamp and id encoding for the batch.  Every merge
cut out of the batch (SharedSoA.merge) composes, through the CPU oracle, to the same JSON as
the same pair marshalled alone."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import marshal as M
from semantic_merge_amd import synth
from semantic_merge_amd.materialize import materialize_conflicts, materialize_ops

from _util import jline, load, run_backend, to_ops

PER_BATCH = 8


@pytest.fixture(scope="module")
def cases():
    return load("compose_cases.json")


def batch_json(ssoa, shared, branches, m, shared_is_b):
    soa = ssoa.merge(m, shared_is_b)
    order, addr, file, ctx, pairs = oracle.compose(soa)
    ops = branches[m] + shared if shared_is_b else shared + branches[m]
    out = materialize_ops(ops, soa.kind, ssoa.strings, order, addr, file, ctx)
    conf = materialize_conflicts(ops, np.asarray(pairs).reshape(-1, 2))
    return jline([o.to_dict() for o in out]), jline([c.to_dict() for c in conf])


def alone_json(a, b):
    out, conf = run_backend(oracle.compose, a, b)
    return jline(out), jline(conf)


@pytest.mark.parametrize("shared_is_b", [False, True])
def test_golden_batches_equal_pairs_marshalled_alone(cases, shared_is_b):
    n = len(cases)
    conflicts = 0
    for i in range(0, n, 7):  # case i's A against the B logs of 8 other cases
        others = [(i + 1 + 13 * k) % n for k in range(PER_BATCH)]
        assert i not in others
        a = cases[i]["A"]
        shared, branches = to_ops(a), [to_ops(cases[j]["B"]) for j in others]
        ssoa = M.marshal_shared(shared, branches)
        assert ssoa.n_shared == len(shared) and ssoa.n_merges == PER_BATCH
        assert ssoa.off.tolist() == np.cumsum([len(shared)] + [len(b) for b in branches]).tolist()
        assert int(ssoa.sym.max(initial=0)) < ssoa.n_sym
        for m, j in enumerate(others):
            got = batch_json(ssoa, shared, branches, m, shared_is_b)
            want = alone_json(cases[j]["B"], a) if shared_is_b else alone_json(a, cases[j]["B"])
            assert got[0] == want[0], f"case {i} x {j}: composed ops differ"
            assert got[1] == want[1], f"case {i} x {j}: conflicts differ"
            conflicts += got[1] != "[]"
    assert conflicts > 0


def test_shared_log_is_marshalled_once(cases):
    a, bs = to_ops(cases[5]["A"]), [to_ops(cases[j]["B"]) for j in (6, 7, 8)]
    ssoa = M.marshal_shared(a, bs)
    assert ssoa.n_total == len(a) + sum(len(b) for b in bs)
    for c in M._COLS:
        assert len(getattr(ssoa, c)) == ssoa.n_total
    # written into the caller's columns when given
    cols = {"kind": np.empty(ssoa.n_total, np.uint8), "sym": np.empty(ssoa.n_total, np.uint32),
            "v0": np.empty(ssoa.n_total, np.int32), "v1": np.empty(ssoa.n_total, np.int32),
            **{c: np.empty(ssoa.n_total, np.uint64) for c in ("ts", "oid_hi", "oid_lo")}}
    again = M.marshal_shared(a, bs, cols)
    for c in ("kind", "sym", "v0", "v1"):
        assert getattr(again, c) is cols[c]
        assert np.array_equal(getattr(again, c), getattr(ssoa, c)), c
    empty = M.marshal_shared([], [])
    assert empty.n_merges == 0 and empty.n_total == 0 and empty.off.tolist() == [0]


@pytest.mark.parametrize("shared_is_b", [False, True])
def test_rank_fallbacks_from_one_branch_only(shared_is_b):
    """Non-ISO timestamps and long ids in one branch only: alone, the other pairs take the
    ISO and UUID encodings; in the batch every op takes the dense ranks over the union."""
    spec = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    sh, _ = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(120, 6, 1, **spec)))
    plain = [synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 6, 10 + n, **spec)))[1] for n in (40, 90)]
    odd = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(140, 6, 3, **spec)))[1]
    stamps = ["", "yesterday", "2024-13-99 noon", "1970-01-01T00:00:00Z", "2024-01-01T00:00:00.5Z", "été"]
    for k, d in enumerate(odd):
        d["provenance"]["timestamp"] = stamps[k % len(stamps)]
        d["id"] = f"an-identifier-of-more-than-fifteen-bytes-{(k * 7919) % 140:04d}"
    dicts = [plain[0], odd, plain[1]]
    shared, branches = to_ops(sh), [to_ops(b) for b in dicts]
    alone = M.marshal(shared, branches[0])
    assert (alone.ts_mode, alone.id_mode) == (M.TS_ISO, M.ID_UUID)
    ssoa = M.marshal_shared(shared, branches)
    assert (ssoa.ts_mode, ssoa.id_mode) == (M.TS_RANK, M.ID_RANK)
    conflicts = 0
    for m, b in enumerate(dicts):
        got = batch_json(ssoa, shared, branches, m, shared_is_b)
        want = alone_json(b, sh) if shared_is_b else alone_json(sh, b)
        assert got == want, f"merge {m}"
        conflicts += got[1] != "[]"
    assert conflicts > 0


def test_same_exceptions_as_marshal(cases):
    a, b = to_ops(cases[0]["A"]), to_ops(cases[1]["B"])
    bad = to_ops(cases[2]["B"]) + [object()]
    with pytest.raises(Exception) as one:
        M.marshal_native(a, bad)
    with pytest.raises(type(one.value)):
        M.marshal_shared(a, [b, bad])
