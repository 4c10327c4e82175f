"""GPU parity of the presorted window kernel (k_window_f, smx_window.h) at the shapes where
its LDS counters can go wrong: the group counters that a wave adds up before its one atomic
per group (step 4), the bucket counters, one per word (steps 6-9), and the arrays that
later phases lay over them (rown over the bucket counters).

Every log is cut out of one synthetic base (tests/_shapes.pick) and then given the
timestamps, kinds or ids of its case.  The plan places a window boundary at every multiple
of its target (1792 ops, then 768, then 256 when a window overflows) and moves it back to
the start of the timestamp group it falls into, so a log of at most 1792 ops, or of one
timestamp group, is one window.  With the small plan off (smx_set_small_limit(0)) logs of
at most 2048 ops take the windows as well.  Each case is compared with the C oracle on
order, addr, file, ctx and the conflict pairs (their count is the array's shape), and the
plan is the expected one."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd._lib import DeviceCompose, set_small_limit
from semantic_merge_amd.ops import KIND_MOVE, KIND_RANK, KIND_RENAME, N_KINDS

from _shapes import pick
from _util import _eq_soa

pytestmark = pytest.mark.gpu

T0 = np.uint64(synth.BASE_MS)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _windows_only():
    """The small plan off for the module; the base log dropped at its end."""
    old = set_small_limit(0)
    yield
    set_small_limit(old)
    _cache.clear()


def _base():
    if "base" not in _cache:
        _cache["base"] = synth.lift_soa(synth.lift_logs(synth.LiftSpec(40_000, 300, 97)))
    return _cache["base"]


def _cut(na, nb, only_kind=None):
    """The first na ops of branch A and nb of branch B (of kind only_kind, if given)."""
    base = _base()
    ka, kb = np.ones(base.n_a, bool), np.ones(base.n_b, bool)
    if only_kind is not None:
        ka, kb = base.kind[:base.n_a] == only_kind, base.kind[base.n_a:] == only_kind
    ka &= np.cumsum(ka) <= na
    kb &= np.cumsum(kb) <= nb
    soa = pick(base, ka, kb)
    assert (soa.n_a, soa.n_b) == (na, nb)
    return soa


def _one_timestamp(soa):
    soa.ts[:] = T0
    return soa


def _check(soa, plan, label):
    for lo, m in ((0, soa.n_a), (soa.n_a, soa.n_b)):  # the presorted plans' precondition
        assert np.all(np.diff(soa.ts[lo:lo + m].astype(np.int64)) >= 0), label
    ref = oracle.compose(soa)
    dc = DeviceCompose(soa)
    dc.run()
    got = dc.results()
    _eq_soa(got, ref, f"{label} (plan {dc.last_plan()}, n_a={soa.n_a}, n_b={soa.n_b})")
    assert dc.last_plan() == plan, f"{label}: plan {dc.last_plan()}, expected {plan}"
    return ref


# ---------------------------------------------------------------------------
# window sizes at the packing and chunk edges


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 511, 512, 513])
def test_one_window_sizes(n):
    """One window of n ops over both branches, with the base's runs of 64 ops per branch."""
    _check(_cut(n // 2, n - n // 2), "presorted", f"one window of {n}")


@pytest.mark.parametrize("n", [2047, 2048])
def test_one_full_window(n):
    """n ops of one timestamp: the boundary at 1792 moves back to 0, the second window
    holds them all (six kinds, one run)."""
    _check(_one_timestamp(_cut(n // 2, n - n // 2)), "presorted", f"one window of {n}")


def test_two_windows_2048_and_1():
    """2048 ops of one timestamp and one later op: 2049 ops overflow the window at the
    targets 1792 and 768; at 256 the boundary at 2048 falls on the last op and stays."""
    soa = _one_timestamp(_cut(1024, 1025))
    soa.ts[-1] = T0 + np.uint64(1)
    _check(soa, "presorted", "windows of 2048 and 1")


# ---------------------------------------------------------------------------
# counter widths


@pytest.mark.parametrize("kind", [KIND_MOVE, KIND_RENAME, KIND_RANK["editStmtBlock"]], ids=["moves", "renames", "edits"])
def test_one_group_of_2048(kind):
    """One timestamp, one kind: a single (kind, run) group of 2048 ops, a count that needs
    twelve bits of its counter and that every wave adds 64 at a time."""
    assert np.any(_base().kind == kind)
    _check(_one_timestamp(_cut(1024, 1024, only_kind=kind)), "presorted", f"one group of 2048, kind {kind}")


def test_every_op_its_own_run():
    """2048 distinct timestamps (A even, B odd): every op is a run, every group has one op;
    1792 runs of six kinds are more groups than the counters hold, so the windows halve."""
    soa = _cut(1024, 1024)
    for side, (lo, m) in enumerate(((0, soa.n_a), (soa.n_a, soa.n_b))):
        soa.ts[lo:lo + m] = T0 + np.uint64(2) * np.arange(m, dtype=np.uint64) + np.uint64(side)
    _check(soa, "presorted", "2048 runs of one op")


@pytest.mark.parametrize("per_run", [3, 31, 33])
def test_waves_over_many_runs(per_run):
    """Runs of per_run ops per branch: a wave's 64 ops lie in three or more runs (the
    per-op count), in exactly two with the seam anywhere in the wave, or in one."""
    soa = _cut(800, 800)
    for lo, m in ((0, soa.n_a), (soa.n_a, soa.n_b)):
        soa.ts[lo:lo + m] = T0 + (np.arange(m) // per_run).astype(np.uint64)
    _check(soa, "presorted", f"runs of {per_run}")


# ---------------------------------------------------------------------------
# kinds


def _other_kinds(soa):
    return np.flatnonzero((soa.kind != KIND_MOVE) & (soa.kind != KIND_RENAME))


def test_all_18_kinds():
    """Every kind present in one window: the ops that are neither moves nor renames take
    the sixteen other kinds in turn (they output neither value, whatever their kind)."""
    soa = _cut(850, 850)
    oth = _other_kinds(soa)
    soa.kind[oth] = (2 + np.arange(len(oth)) % (N_KINDS - 2)).astype(np.uint8)
    assert len(np.unique(soa.kind)) == N_KINDS
    _check(soa, "presorted", "all 18 kinds")


def test_one_kind_only():
    """Renames only, over the base's runs: one dense kind, no kind bits in the wave's key."""
    _check(_cut(700, 700, only_kind=KIND_RENAME), "presorted", "renames only")


def test_lowest_and_highest_kind_only():
    """Moves (kind 0) and unknown-type ops (kind 17) only."""
    soa = _cut(850, 850)
    soa.kind[soa.kind != KIND_MOVE] = N_KINDS - 1
    assert set(np.unique(soa.kind).tolist()) == {KIND_MOVE, N_KINDS - 1}
    _check(soa, "presorted", "kinds 0 and 17 only")


# ---------------------------------------------------------------------------
# bucket collisions


def test_ids_equal_in_top_32_bits():
    """Every id of both branches has the same top 32 bits: each group's ops fall into one
    bucket with equal rank keys, and step 9 ranks them on the full ids."""
    soa = _cut(800, 800)
    soa.oid_hi[:] = (soa.oid_hi & np.uint64(0xFFFFFFFF)) | np.uint64(0x5EED5EED00000000)
    _check(soa, "presorted", "equal top 32 bits")


@pytest.mark.parametrize("word", [0, 0xFFFFFFFFFFFFFFFF], ids=["zeros", "ones"])
def test_ids_all_equal(word):
    """All ids 0, or all ones: every op of a group lands in the group's first (last)
    bucket, whose counter takes the whole group; equal ids are ordered by (side, index)."""
    soa = _cut(800, 800)
    soa.oid_hi[:] = np.uint64(word)
    soa.oid_lo[:] = np.uint64(word)
    _check(soa, "presorted", f"ids all {word:#x}")


@pytest.mark.parametrize("n", [1000, 2048])
def test_adjacent_buckets(n):
    """One group of n ops whose ids are spaced by 2^32 / n in their top 32 bits, in a random
    order: every bucket of the group takes exactly one op, so every bucket has occupied
    neighbours (the pairs that shared a word when the counters were packed)."""
    soa = _one_timestamp(_cut(n // 2, n // 2, only_kind=KIND_RENAME))
    step = (1 << 32) // n
    slot = np.random.default_rng(3).permutation(n).astype(np.uint64)
    soa.oid_hi[:] = ((slot * np.uint64(step) + np.uint64(step // 2)) << np.uint64(32)) | (soa.oid_hi & np.uint64(0xFFFFFFFF))
    _check(soa, "presorted", f"adjacent buckets, group of {n}")


# ---------------------------------------------------------------------------
# the wide instance


@pytest.mark.parametrize("n", [8192, 2049])
def test_wide_window(n):
    """One timestamp group of n ops, more than a 2048-op window holds: the wide (8192-op)
    windows take it, as they take config 5's groups."""
    base = synth.lift_soa(synth.lift_logs(synth.LiftSpec(2 * 4200, 100, 17, ops_per_ms=4096,
                                                         mix=synth.ADVERSARIAL_MIX, rename_overlap=0.30)))
    ka, kb = np.arange(base.n_a) < n // 2, np.arange(base.n_b) < n - n // 2
    soa = _one_timestamp(pick(base, ka, kb))
    assert soa.n == n
    _check(soa, "presorted-wide", f"wide window of {n}")


# ---------------------------------------------------------------------------
# one branch only


@pytest.mark.parametrize("side", ["a_only", "b_only"])
@pytest.mark.parametrize("n", [600, 2048])
def test_one_branch_windows(side, n):
    """Windows that hold ops of one branch only (the other branch is empty): 600 ops in
    runs of 64, and a full window of one timestamp."""
    soa = _cut(n, 0) if side == "a_only" else _cut(0, n)
    if n == 2048:
        _one_timestamp(soa)
    _check(soa, "presorted", f"{side}, {n} ops")
