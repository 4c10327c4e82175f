"""The premise of smx_compose_pairs on the CPU: marshalling a group of logs once, with one symbol
/ string / equality-class table and one timestamp and id encoding for all of them
(marshal_logs), does not change any pair's result.  Every golden case's two logs, cut out of a
group as LogsSoA.pair(i, j), compose through the CPU oracle to the case's golden output; the
dense-rank timestamp and id fallbacks rank over the union of the logs and keep every pair's
order too."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import marshal as M
from semantic_merge_amd import synth
from semantic_merge_amd.materialize import materialize_conflicts, materialize_ops

from _util import jline, load, run_backend, to_ops

PER_GROUP = 6  # golden cases per group: 12 logs marshalled together


@pytest.fixture(scope="module")
def cases():
    return load("compose_cases.json")


def pair_json(lsoa, logs, i, j):
    """The composed ops and the conflicts of (log i, log j) of a group, as JSON lines."""
    soa = lsoa.pair(i, j)
    order, addr, file, ctx, pairs = oracle.compose(soa)
    ops = logs[i] + logs[j]
    out = materialize_ops(ops, soa.kind, lsoa.strings, order, addr, file, ctx)
    conf = materialize_conflicts(ops, np.asarray(pairs).reshape(-1, 2))
    return jline([o.to_dict() for o in out]), jline([c.to_dict() for c in conf])


def test_golden_pairs_out_of_a_common_id_domain(cases):
    n = len(cases)
    assert n >= PER_GROUP
    conflicts = 0
    for g0 in range(0, n, PER_GROUP):
        group = [(g0 + k) % n for k in range(PER_GROUP)]
        logs = [to_ops(cases[c][side]) for c in group for side in ("A", "B")]
        lsoa = M.marshal_logs(logs)
        assert lsoa.n_logs == 2 * PER_GROUP
        assert lsoa.log_off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in logs])]).tolist()
        assert int(lsoa.sym.max(initial=0)) < lsoa.n_sym
        for k, c in enumerate(group):
            out, conf = pair_json(lsoa, logs, 2 * k, 2 * k + 1)
            assert out == jline(cases[c]["out"]), f"case {c}: composed ops differ from the golden output"
            assert conf == jline(cases[c]["conflicts"]), f"case {c}: conflicts differ from the golden output"
            conflicts += conf != "[]"
        # a pair across two cases, in both orientations, and a self pair: as the pair marshalled alone
        a, b = group[0], group[PER_GROUP // 2]
        for (i, j), (x, y) in (((0, PER_GROUP + 1), (cases[a]["A"], cases[b]["B"])),
                               ((PER_GROUP + 1, 0), (cases[b]["B"], cases[a]["A"])),
                               ((1, 1), (cases[a]["B"], cases[a]["B"]))):
            wo, wc = run_backend(oracle.compose, x, y)
            assert pair_json(lsoa, logs, i, j) == (jline(wo), jline(wc)), f"group at {g0}: pair ({i}, {j})"
    assert conflicts > 0


def test_rank_fallbacks_rank_over_the_union():
    """Non-ISO timestamps and long ids in one log only: alone, the other pairs take the ISO and
    UUID encodings; in the group every op takes the dense ranks over the union of the logs."""
    spec = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
    dicts = [synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, 6, 10 + n, **spec)))[s]
             for n, s in ((60, 0), (40, 1), (90, 1))]
    odd = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(140, 6, 3, **spec)))[1]
    stamps = ["", "yesterday", "2024-13-99 noon", "1970-01-01T00:00:00Z", "2024-01-01T00:00:00.5Z", "été"]
    for k, d in enumerate(odd):
        d["provenance"]["timestamp"] = stamps[k % len(stamps)]
        d["id"] = f"an-identifier-of-more-than-fifteen-bytes-{(k * 7919) % 140:04d}"
    dicts.insert(2, odd)
    logs = [to_ops(d) for d in dicts]
    alone = M.marshal(logs[0], logs[1])
    assert (alone.ts_mode, alone.id_mode) == (M.TS_ISO, M.ID_UUID)
    lsoa = M.marshal_logs(logs)
    assert (lsoa.ts_mode, lsoa.id_mode) == (M.TS_RANK, M.ID_RANK)
    conflicts = 0
    for i in range(len(logs)):
        for j in range(len(logs)):
            wo, wc = run_backend(oracle.compose, dicts[i], dicts[j])
            got = pair_json(lsoa, logs, i, j)
            assert got == (jline(wo), jline(wc)), f"pair ({i}, {j})"
            conflicts += got[1] != "[]"
    assert conflicts > 0
