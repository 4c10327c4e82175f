"""The two CPU references agree on unbalanced, empty and disjoint branch logs: the
pure-Python restatement (oracle/compose_ref.py) equals the C oracle (oracle/compose_ref.c)
on every branch shape of tests/_shapes.py.  The golden vectors pin the C oracle only at
0-40 ops per side; the GPU tests of these shapes compare with the C oracle alone."""
import functools

import numpy as np
import pytest

from oracle import compose_ref, oracle
from semantic_merge_amd import synth

from _shapes import SHAPES, pick, shape

CUT = 3000  # ops kept per branch: the pure-Python side stays fast

SPECS = {
    "lift": synth.LiftSpec(40_000, 400, 7),
    "adv": synth.LiftSpec(40_000, 200, 17, ops_per_ms=16, mix=synth.ADVERSARIAL_MIX, divergent=0.3),
}


@functools.lru_cache(maxsize=None)
def _base(name):
    soa = synth.lift_soa(synth.lift_logs(SPECS[name]))
    return pick(soa, np.arange(soa.n_a) < CUT, np.arange(soa.n_b) < CUT)


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("base", list(SPECS))
def test_python_restatement_matches_c_oracle_on_branch_shapes(base, name):
    soa = shape(_base(base), name, seed=5)
    assert soa.n <= 2 * CUT
    got, ref = compose_ref.compose(soa), oracle.compose(soa)
    for what, g, r in zip(("order", "addr", "file", "ctx", "conflicts"), got, ref):
        g, r = np.asarray(g), np.asarray(r)
        assert g.shape == r.shape, f"{base}/{name}: {what} shape {g.shape} vs {r.shape}"
        assert np.array_equal(g, r), f"{base}/{name}: {what} differs"
    if name in ("a_empty", "b_empty"):
        assert len(ref[4]) == 0 and len(ref[0]) == soa.n


def test_shapes_are_what_they_say():
    """pick keeps branch order and the sizes the shape names promise."""
    soa = _base("lift")
    na, nb = soa.n_a, soa.n_b
    want = {"a_empty": (0, nb), "b_empty": (na, 0), "a_one": (1, nb), "b_one": (na, 1), "a_255": (255, nb),
            "b_257_tail": (na, 257), "a_before_b": (na // 2, nb - nb // 2), "b_before_a": (na - na // 2, nb // 2),
            "odd_sizes": (na - 129, nb - 1), "a_head_3q": (3 * na // 4, nb), "b_mid_half": (na, nb // 2)}
    for name in SHAPES:
        s = shape(soa, name, seed=5)
        if name in want:
            assert (s.n_a, s.n_b) == want[name], name
        assert all(len(getattr(s, c)) == s.n for c in ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1"))
        assert s.n_sym == soa.n_sym
        for lo, m in ((0, s.n_a), (s.n_a, s.n_b)):  # a timestamp-ordered branch stays ordered
            b = s.ts[lo:lo + m]
            assert np.all(b[1:] >= b[:-1]), name
    s = shape(soa, "a_before_b", seed=5)
    assert s.ts[s.n_a - 1] <= s.ts[s.n_a]
    s = shape(soa, "a_burst", seed=5)
    assert s.n_a == na - na // 3 and np.array_equal(s.oid_lo[:s.n_a], soa.oid_lo[na // 3:na])
    s = shape(soa, "a_sparse", seed=5)
    assert 0 < s.n_a < na // 16 and s.n_b == nb
