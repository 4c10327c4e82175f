"""GPU parity of smx_compose_pairs with SMX_BATCH_LARGE: pairs of more than 2048 ops run inside
the batch through compose_large, in the workspace slice at the pair's result offset, between
small pairs; a large self pair, a walk of several rounds, failed pairs between large ones, grid
caps, and one workspace reused across flags.  Every pair is checked against the CPU oracle on
that pair alone, and every output word outside the pairs' results against the canary."""
import dataclasses

import numpy as np
import pytest

from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import DeviceBatch, compose_pairs_soa, session

from _batch import ADV, branch, none_moves
from _pairs import FILL, check, gap_log, logs_soa, ref, run, same_bytes
from _util import _eq_soa as _eq

pytestmark = pytest.mark.gpu

LARGE = _abi.BATCH_LARGE
RENAME = synth.KIND_RANK["renameSymbol"]


@pytest.fixture(scope="module")
def batch():
    """Logs of 30 to 3000 ops; pairs of 2049, 4097 and 5000 ops between small ones, large pairs
    in both orientations, a large self pair, and a pair of two logs of more than 1024 renames."""
    n_sym = 40
    adv = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
    logs = [branch(1000, n_sym, 1, 0, **adv),                    # 0
            branch(1049, n_sym, 2, 1, **adv),                    # 1: 1000 + 1049 = 2049
            branch(120, n_sym, 3, 1, **ADV),                     # 2
            none_moves(branch(2048, n_sym, 4, 0, ops_per_ms=3), 5),   # 3
            branch(2049, n_sym, 5, 1, shuffle=True, mix=synth.ADVERSARIAL_MIX),  # 4: 2048 + 2049 = 4096 + 1
            gap_log(100),                                        # 5: held by no pair
            branch(30, n_sym, 6, 0, **ADV),                      # 6
            branch(3000, n_sym, 7, 0, **ADV),                    # 7
            branch(2000, n_sym, 8, 1, ops_per_ms=4096, mix=synth.ADVERSARIAL_MIX),  # 8: 3000 + 2000 = 5000
            branch(3000, n_sym, 9, 1, **ADV)]                    # 9
    lsoa = logs_soa(logs, n_sym)
    pairs = [(2, 6), (0, 1), (6, 2), (3, 4), (2, 2), (7, 8), (1, 0), (6, 0), (7, 7), (4, 3), (9, 7), (7, 9), (0, 2)]
    lens = np.diff(lsoa.log_off)
    assert sorted({int(lens[i] + lens[j]) for i, j in pairs} & {2049, 4097, 5000}) == [2049, 4097, 5000]
    ren = [int((lsoa.kind[lsoa.log_off[l]: lsoa.log_off[l + 1]] == RENAME).sum()) for l in (7, 9)]
    assert min(ren) > 1024  # the walk of (7, 9), (9, 7) and (7, 7) takes several rounds
    assert len(ref(lsoa, 7, 9)[4]) > 64 and len(ref(lsoa, 0, 1)[4]) > 0
    return lsoa, pairs


def test_large_pairs_between_small_ones(batch):
    lsoa, pairs = batch
    lens = np.diff(lsoa.log_off)
    big = [p for p, (i, j) in enumerate(pairs) if lens[i] + lens[j] > _abi.BATCH_MAX_OPS]
    assert len(big) == 8
    db, raw, res = run(lsoa, pairs, flags=LARGE)
    check(db, raw, "SMX_BATCH_LARGE")
    assert (raw["counts"] != -2).all()
    # without the flag the same pairs are sent back, untouched, and the small ones are the same
    db0, raw0, res0 = run(lsoa, pairs)
    check(db0, raw0, "flags 0", sent_back=big)
    same_bytes([r for p, r in enumerate(res) if p not in big], [r for p, r in enumerate(res0) if p not in big],
               "the small pairs under either flags")
    # bit-equal to smx_compose_batch_ex on the repeated layout
    rep = DeviceBatch([lsoa.pair(i, j) for i, j in pairs], n_sym=lsoa.n_sym, fill=FILL, flags=LARGE)
    rep.run()
    same_bytes(res, rep.results(), "smx_compose_pairs vs smx_compose_batch_ex on the repeated layout")


def test_grid_caps_and_workspace_reuse(batch):
    lsoa, pairs = batch
    raws = {}
    for cap in (0, 1):  # one workgroup runs large pair after large pair, and small after small
        db, raws[cap], _ = run(lsoa, pairs, flags=LARGE, grid_cap=cap)
        check(db, raws[cap], f"grid_cap {cap}")
    for name, a in raws[0].items():
        assert a.tobytes() == raws[1][name].tobytes(), f"grid_cap 1: {name} differs from grid_cap 0"
    # one workspace: flags 0, then SMX_BATCH_LARGE, then 0 again
    db = run(lsoa, pairs, flags=LARGE)[0]
    seen = {}
    for step, flags in enumerate((0, LARGE, 0)):
        for name in db._OUT:
            getattr(db, name).fill_(FILL)
        db.flags = flags
        db.run()
        seen[step] = db.raw()
    for name, a in raws[0].items():
        assert a.tobytes() == seen[1][name].tobytes(), f"reused workspace, SMX_BATCH_LARGE: {name}"
        assert seen[0][name].tobytes() == seen[2][name].tobytes(), f"reused workspace, flags 0 twice: {name}"
    lens = np.diff(lsoa.log_off)
    check(db, seen[2], "reused workspace, flags 0",
          sent_back=[p for p, (i, j) in enumerate(pairs) if lens[i] + lens[j] > _abi.BATCH_MAX_OPS])


def test_failed_pairs_between_large_ones(batch):
    good, pairs = batch
    # an invalid kind in the last tile of log 7, a symbol = n_sym in log 4
    bad = dataclasses.replace(good, kind=good.kind.copy(), sym=good.sym.copy())
    bad.kind[int(bad.log_off[8]) - 1] = 18
    bad.sym[int(bad.log_off[4]) + 2048] = good.n_sym
    db, raw, _ = run(bad, pairs, flags=LARGE)
    check(db, raw, "kind = 18, sym = n_sym", failed=[p for p, (i, j) in enumerate(pairs) if {i, j} & {7, 4}])
    # a large pair's region one entry too short; a large pair whose region starts below an earlier entry
    lens = np.diff(good.log_off)
    room = np.asarray([lens[i] + lens[j] for i, j in pairs], np.int64)
    short = room.copy()
    short[5] -= 1
    db, raw, _ = run(good, pairs, flags=LARGE, res_off=np.concatenate([[0], np.cumsum(short)]))
    check(db, raw, "res_off one entry too short", failed=(5,))
    low = np.concatenate([[0], np.cumsum(room)])
    low[4] = low[3] - 1
    db, raw, _ = run(good, pairs, flags=LARGE, res_off=low)
    check(db, raw, "res_off below an earlier entry", failed=(3, 4))


def test_conflict_truncation_of_a_large_pair(batch):
    lsoa, _ = batch
    pairs = [(2, 6), (7, 9), (0, 2)]
    n_conf = len(ref(lsoa, 7, 9)[4])
    for cap in (0, n_conf - 1):
        db, raw, res = run(lsoa, pairs, flags=LARGE, conflict_caps=[30, cap, 120])
        check(db, raw, f"capacity {cap}", truncated=(1,))
        assert int(raw["counts"][3]) == n_conf and len(res[1][4]) == cap


def test_session_large(batch):
    lsoa, pairs = batch
    got = compose_pairs_soa(lsoa, pairs, large=True)
    last = session().last
    assert (last["routed"], last["large"]) == (0, 8)
    for (i, j), g in zip(pairs, got):
        _eq(g, ref(lsoa, i, j), f"compose_pairs_soa(large=True): pair ({i}, {j})")
    got = compose_pairs_soa(lsoa, pairs, large=True, large_max=4097)  # the pairs of 5000 and 6000 ops go through compose()
    last = session().last
    assert (last["routed"], last["large"]) == (4, 4)
    for (i, j), g in zip(pairs, got):
        _eq(g, ref(lsoa, i, j), f"compose_pairs_soa(large_max=4097): pair ({i}, {j})")
