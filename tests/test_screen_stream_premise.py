"""The one new fact the streamed screen (smx_screen_ex with SMX_SCREEN_LARGE, k_screen_stream)
rests on, pinned against the CPU oracle without hardware: the two-head walk over the two sorted
rename lists can be run on chunks of C renames per side -- ranked and merged inside the chunk
alone -- and restarted from the pair of heads at which a chunk ran out, and gives the conflict
list of the whole pair, in at most ceil(RA / C) + ceil(RB / C) rounds."""
import numpy as np

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, SoA, marshal

from _util import load, to_ops

RENAME = synth.KIND_RANK["renameSymbol"]
ADV = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.5, rename_overlap=1.0)
CHUNKS = (1, 2, 3, 7, 64)


def sorted_renames(soa, lo, n):
    """The renames of ops [lo, lo + n): (key, symbol, class, index in A || B) in (ts, id, index) order."""
    idx = [i for i in range(lo, lo + n) if soa.kind[i] == RENAME]
    idx.sort(key=lambda i: (int(soa.ts[i]), int(soa.oid_hi[i]), int(soa.oid_lo[i]), i))
    return [((int(soa.ts[i]), int(soa.oid_hi[i]), int(soa.oid_lo[i])), int(soa.sym[i]), int(soa.v0[i]), i) for i in idx]


def one_round(ca, cb):
    """The walk over one chunk of each side from its heads (0, 0), as the kernel runs it: every
    rename's merged position from its rank in the other chunk (A counts B keys strictly below,
    B counts A keys at or below), the heads compared by position.  Returns the conflicts and
    the heads at which a side ran out."""
    pos_a = [i + sum(b[0] < a[0] for b in cb) for i, a in enumerate(ca)]
    pos_b = [i + sum(a[0] <= b[0] for a in ca) for i, b in enumerate(cb)]
    assert sorted(pos_a + pos_b) == list(range(len(ca) + len(cb)))
    ia = ib = 0
    out = []
    while ia < len(ca) and ib < len(cb):
        a, b = ca[ia], cb[ib]
        if a[1] == b[1] and a[2] != b[2]:
            out.append((a[3], b[3]))
            ia, ib = ia + 1, ib + 1
        elif pos_a[ia] < pos_b[ib]:
            ia += 1
        else:
            ib += 1
    return out, ia, ib


def streamed_conflicts(soa, C):
    A, B = sorted_renames(soa, 0, soa.n_a), sorted_renames(soa, soa.n_a, soa.n_b)
    ia = ib = rounds = 0
    out = []
    while ia < len(A) and ib < len(B):
        got, da, db = one_round(A[ia: ia + C], B[ib: ib + C])
        assert da == len(A[ia: ia + C]) or db == len(B[ib: ib + C]), "a round ends with a chunk used up"
        out += got
        ia, ib, rounds = ia + da, ib + db, rounds + 1
    assert rounds <= -(-len(A) // C) + -(-len(B) // C)
    return np.asarray(out, np.int32).reshape(-1, 2), rounds


def check(soas, label, min_with=1):
    with_conflicts = many_rounds = 0
    for i, soa in enumerate(soas):
        want = oracle.compose(soa)[4]
        for C in CHUNKS:
            got, rounds = streamed_conflicts(soa, C)
            assert got.shape == want.shape and np.array_equal(got, want), f"{label} {i}, chunks of {C}"
            many_rounds += rounds >= 3
        with_conflicts += len(want) > 0
    assert with_conflicts >= min_with, "the equality is vacuous: too few pairs have conflicts"
    assert many_rounds > 0, "no pair took three rounds"


def test_golden_cases():
    cases = load("compose_cases.json")
    check([marshal(to_ops(c["A"]), to_ops(c["B"])) for c in cases[:300]], "compose_cases", min_with=40)


def test_synthetic_logs():
    kws = [ADV, dict(ADV, shuffle=True), dict(ADV, ops_per_ms=4096), dict(ADV, ops_per_ms=4096, shuffle=True)]
    check([synth.lift_soa(synth.lift_logs(synth.LiftSpec(200 + 90 * i, 5 + i, 700 + i, **kws[i % 4])))
           for i in range(8)], "lift logs", min_with=6)


def hot(na, nb, seed, tie=False):
    """Two logs whose every op renames one symbol, all names different: every pair of heads
    conflicts.  tie: B's keys are A's own, so that A goes first on every full-key tie."""
    rng = np.random.default_rng(seed)
    n = na + nb
    ts = np.concatenate([np.sort(rng.integers(1000, 1000 + n, na)), np.sort(rng.integers(1000, 1000 + n, nb))])
    hi, lo = rng.integers(0, 1 << 62, n), rng.integers(0, 1 << 62, n)
    if tie:
        m = min(na, nb)
        ts[na: na + m], hi[na: na + m], lo[na: na + m] = ts[:m], hi[:m], lo[:m]
    v0 = np.arange(n, dtype=np.int32)
    return SoA(na, nb, np.full(n, RENAME, np.uint8), ts.astype(np.uint64), hi.astype(np.uint64), lo.astype(np.uint64),
               np.full(n, 2, np.uint32), v0, v0.copy(), 4, [], TS_ISO, ID_UUID)


def test_hot_symbol():
    soas = [hot(40, 40, 1), hot(90, 17, 2), hot(5, 130, 3), hot(64, 64, 4, tie=True), hot(65, 129, 5, tie=True)]
    for soa in soas:
        assert len(oracle.compose(soa)[4]) == min(soa.n_a, soa.n_b)
    check(soas, "hot symbol", min_with=len(soas))
