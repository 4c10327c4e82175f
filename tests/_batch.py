"""What the GPU tests of the three batched composes share (test_gpu_batch*.py, test_gpu_shared.py,
test_gpu_pairs*.py and the tests of the screens that reuse their logs): synthetic merges and
branch logs, the oracle's answer computed once per merge, and the checks of a DeviceBatch run."""
import numpy as np

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, SharedSoA

from _shapes import pick
from _util import _eq_soa as _eq

FILL = 0x5A5A5A5A  # what every output word holds before a run that checks the unwritten ones
MOVE = synth.KIND_RANK["moveDecl"]
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")
GAP = {"kind": 0xFF, "sym": 0xFFFFFFFF, "v0": -1, "v1": -1}  # invalid: a kernel that read a gap would report -1
ADV = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)


def lift(n, n_sym, seed, **kw):
    return synth.lift_soa(synth.lift_logs(synth.LiftSpec(n, n_sym, seed, **kw)))


_ref = {}


def ref(soa):
    """oracle.compose(soa), computed once per SoA object."""
    got = _ref.get(id(soa))
    if got is None:
        got = _ref[id(soa)] = (soa, oracle.compose(soa))
    return got[1]


def none_moves(soa, seed, p=0.6):
    rng = np.random.default_rng(seed)
    mv = np.flatnonzero(soa.kind == MOVE)
    soa.v0[mv[rng.random(len(mv)) < p]] = -1
    soa.v1[mv[rng.random(len(mv)) < p]] = -1
    return soa


def check_all(got, soas, label):
    assert len(got) == len(soas)
    for m, (g, s) in enumerate(zip(got, soas)):
        assert not isinstance(g, int), f"{label}: merge {m} failed with counts {g}"
        _eq(g, ref(s), f"{label}: merge {m} ({s.n} ops, n_a {s.n_a})")


def check_unwritten(db, raw, soas, failed=()):
    """Nothing past a merge's composed ops or conflict pairs, nothing at all for a failed merge."""
    for m, s in enumerate(soas):
        o, c = int(db.off[m]), int(db.conf_off[m])
        cap = int(db.conf_off[m + 1]) - c
        k, nc = (0, 0) if m in failed else (int(x) for x in raw["counts"][2 * m: 2 * m + 2])
        for name in ("order", "addr", "file", "ctx"):
            assert (raw[name][o + k: o + s.n] == FILL).all(), f"merge {m}: {name} written past its {k} ops"
        assert (raw["conf"][2 * (c + min(nc, cap)): 2 * (c + cap)] == FILL).all(), f"merge {m}: conflicts past its pairs"
    assert (raw["conf"][2 * int(db.conf_off[-1]):] == FILL).all()


def branch(n, n_sym, seed, side, **kw):
    """One branch log of n ops (side 0: a lift log's A branch, 1: its B branch), as an SoA
    with the other branch empty."""
    soa = synth.lift_soa(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **kw)))
    a, b = np.ones(soa.n_a, bool), np.ones(soa.n_b, bool)
    return pick(soa, a, ~b) if side == 0 else pick(soa, ~a, b)


def own_logs(n_sym, seed0, sizes):
    """Own logs as test_gpu_batch.py's mixed40 has them: an adversarial mix with divergent renames
    against the shared log's renames, None-valued moves, a shuffled branch, dense ties."""
    out = []
    for i, n in enumerate(sizes):
        kw = [ADV, dict(ops_per_ms=3), dict(shuffle=True, mix=synth.ADVERSARIAL_MIX),
              dict(ops_per_ms=4096, mix=synth.ADVERSARIAL_MIX), dict()][i % 5]
        soa = branch(n, n_sym, seed0 + i, 1, **kw)
        out.append(none_moves(soa, i) if i % 5 == 1 else soa)
    return out


def shared_soa(shared, owns, n_sym, gap=0):
    """The SharedSoA of one shared branch log and the own logs, `gap` invalid entries
    between the shared log and the first own log."""
    parts = [shared] + list(owns)
    cols = []
    for c in COLS:
        arrs = [np.asarray(getattr(p, c)) for p in parts]
        if gap:
            arrs.insert(1, np.full(gap, GAP.get(c, 0), arrs[0].dtype))
        cols.append(np.concatenate(arrs))
    off = shared.n + gap + np.concatenate([[0], np.cumsum([o.n for o in owns], dtype=np.int64)]).astype(np.int64)
    return SharedSoA(shared.n, off, *cols, n_sym, [], TS_ISO, ID_UUID)
