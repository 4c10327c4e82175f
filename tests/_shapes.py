"""Branch shapes for the compose tests: unbalanced, empty and disjoint branch logs cut out
of a synthetic log (synth.lift_logs always splits its ops evenly over two branches that
cover the same timestamp range at the same density)."""
import numpy as np

from semantic_merge_amd import synth
from semantic_merge_amd.marshal import SoA

SHAPES = ("a_empty", "b_empty", "a_one", "b_one", "a_255", "b_257_tail", "a_before_b", "b_before_a",
          "a_sparse", "b_sparse", "a_burst", "odd_sizes", "a_head_3q", "b_mid_half")

_COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")


def pick(soa, keep_a, keep_b):
    """A new SoA holding the ops of `soa` that two boolean masks over branch A and branch B
    select; order inside each branch, n_sym and the strings are kept."""
    keep_a = np.asarray(keep_a, dtype=bool)
    keep_b = np.asarray(keep_b, dtype=bool)
    assert keep_a.shape == (soa.n_a,) and keep_b.shape == (soa.n_b,)
    keep = np.concatenate([keep_a, keep_b])
    cols = [np.ascontiguousarray(getattr(soa, c)[keep]) for c in _COLS]
    return SoA(int(keep_a.sum()), int(keep_b.sum()), *cols, soa.n_sym, soa.strings, soa.ts_mode, soa.id_mode)


def _span(n, lo, hi):
    m = np.zeros(n, bool)
    m[max(lo, 0):max(min(hi, n), 0)] = True
    return m


def branch_shapes(soa, seed, scale=1):
    """Yields (name, keep_a, keep_b), one per name in SHAPES.  scale divides the shapes'
    op counts (255, 257, 3000, 129), for a base much shorter than a window grid."""
    na, nb = soa.n_a, soa.n_b
    rng = np.random.default_rng(seed)
    all_a, all_b = np.ones(na, bool), np.ones(nb, bool)
    c255, c257, c3000, c129 = (max(c // scale, 1) for c in (255, 257, 3000, 129))
    yield "a_empty", np.zeros(na, bool), all_b
    yield "b_empty", all_a, np.zeros(nb, bool)
    yield "a_one", _span(na, na // 2, na // 2 + 1), all_b
    yield "b_one", all_a, _span(nb, nb // 2, nb // 2 + 1)
    yield "a_255", _span(na, 0, c255), all_b
    yield "b_257_tail", all_a, _span(nb, nb - c257, nb)
    yield "a_before_b", _span(na, 0, na // 2), _span(nb, nb // 2, nb)
    yield "b_before_a", _span(na, na // 2, na), _span(nb, 0, nb // 2)
    yield "a_sparse", rng.random(na) < 1 / 64, all_b
    yield "b_sparse", all_a, rng.random(nb) < 1 / 64
    yield "a_burst", _span(na, na // 3, na // 3 + c3000), rng.random(nb) < 0.5
    yield "odd_sizes", _span(na, 0, na - c129), _span(nb, 0, nb - 1)
    # a branch that runs out, or starts late and ends early, in the middle of the window grid
    # while the other goes on; where both have ops, the timestamp groups stay whole
    yield "a_head_3q", _span(na, 0, 3 * na // 4), all_b
    yield "b_mid_half", all_a, _span(nb, nb // 4, nb // 4 + nb // 2)


def shape(soa, name, seed=0, scale=1):
    """pick() of the shape `name`."""
    for nm, ka, kb in branch_shapes(soa, seed, scale):
        if nm == name:
            return pick(soa, ka, kb)
    raise KeyError(name)


def alternating_groups(spec, big, small):
    """spec's logs with timestamp groups of alternately `big` and `small` ops per branch
    (the same on both branches)."""
    soa = synth.lift_soa(synth.lift_logs(spec))
    for lo, m in ((0, soa.n_a), (soa.n_a, soa.n_b)):
        period = big + small
        k = np.arange(m)
        grp = 2 * (k // period) + ((k % period) >= big)
        soa.ts[lo:lo + m] = soa.ts[0] + grp.astype(np.uint64) * np.uint64(2)
    return soa


# Merges of at most 2048 ops for the small plan and the batch: the sizes' edges, ties, shuffled logs.
SPECS = [
    synth.LiftSpec(1, 1, 3),
    synth.LiftSpec(2, 1, 4),
    synth.LiftSpec(17, 3, 5, ops_per_ms=1),
    synth.LiftSpec(1000, 100, 6),
    synth.LiftSpec(1000, 20, 7, shuffle=True),
    synth.LiftSpec(2000, 30, 8, ops_per_ms=4096, mix=synth.ADVERSARIAL_MIX, rename_overlap=1.0),
    synth.LiftSpec(2047, 5, 9, ops_per_ms=1, mix=synth.ADVERSARIAL_MIX, divergent=0.5),
    synth.LiftSpec(2048, 2048, 10, shuffle=True, mix=synth.ADVERSARIAL_MIX),
    synth.LiftSpec(2048, 1, 12, ops_per_ms=1),
]
