"""GPU parity on unbalanced, empty and disjoint branch logs, and the corners of the C ABI.

Every other synthetic log of the suite splits its ops evenly over two branches of the same
timestamp range and density (synth.lift_logs), so the merge-path split (k_fpart), the
column scans and the windows' partial chunks only ever saw a0 ~ b0.  Here every branch
shape of tests/_shapes.py is cut out of a base log per order plan and compared with the
CPU oracle: windows that hold one branch only, a branch that runs out in the middle of the
window grid, branches shorter than a chunk or a window, empty branches above the small
plan.  The ABI tests (after the parity tests) pin smx_ops.b_gap > 0 through smx_compose, a
conflict_cap smaller than the number of conflicts, a workspace that is too small and
merges of zero and one ops, as include/smx.h describes them."""
import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd._lib import DeviceCompose, SmxError, compose_soa, set_small_limit

from _shapes import SHAPES, alternating_groups, pick, shape
from _util import _eq_soa

pytestmark = pytest.mark.gpu

ADV = synth.ADVERSARIAL_MIX
SPECS = {
    "lift": synth.LiftSpec(40_000, 400, 7),
    "adv": synth.LiftSpec(40_000, 200, 17, ops_per_ms=16, mix=ADV, divergent=0.3),
    "wide": synth.LiftSpec(80_000, 300, 17, ops_per_ms=4096, mix=ADV, rename_overlap=0.3),
    "seg": synth.LiftSpec(80_000, 300, 73, mix=ADV),     # (alternating groups of 4050 and 100 ops)
    "shuf": synth.LiftSpec(40_000, 400, 7, shuffle=True),
    "dup": synth.LiftSpec(40_000, 400, 7, shuffle=True),  # (a quarter of the ops share one oid_hi)
    "long": synth.LiftSpec(60_000, 200, 59, ops_per_ms=10_000),
    "small": synth.LiftSpec(2048, 40, 13, mix=ADV),
}
# the plan of each base's odd_sizes shape (nearly the balanced log, whose plan the other GPU
# tests establish); any other shape may legitimately take another plan than its base
PLAN = {"lift": "presorted", "adv": "presorted", "wide": "presorted-wide", "seg": "segmented", "shuf": "radix",
        "dup": "radix+oid_lo", "long": "radix", "small": "small"}
SCALE = {"small": 16}  # the shapes' op counts (255, 257, 3000, 129) on the 2048-op base
SEED = 5

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def _base(name):
    key = ("base", name)
    if key not in _cache:
        spec = SPECS[name]
        soa = alternating_groups(spec, 4050, 100) if name == "seg" else synth.lift_soa(synth.lift_logs(spec))
        if name == "dup":  # equal (timestamp, oid_hi) pairs inside each branch: the radix sort needs oid_lo too
            soa.oid_hi[np.random.default_rng(SEED).random(soa.n) < 0.25] = np.uint64(7)
        _cache[key] = soa
    return _cache[key]


def _case(base, name):
    """(the picked log, the oracle's result), computed once per module."""
    key = (base, name)
    if key not in _cache:
        soa = shape(_base(base), name, SEED, SCALE.get(base, 1))
        _cache[key] = (soa, oracle.compose(soa))
    return _cache[key]


@pytest.fixture
def windows():
    """smx_set_small_limit(0): merges of at most 2048 ops take the window plans too."""
    old = set_small_limit(0)
    yield
    set_small_limit(old)


def _check_plan(base, name, plan, mode):
    print(f"PLAN {mode} {base} {name} -> {plan}")
    if name == "odd_sizes":
        want = PLAN[base]
        ok = plan.startswith("radix") if want == "radix" else plan == want
        assert ok, f"{base}/{name} ({mode}): plan {plan}, expected {want}"


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("base", list(SPECS))
def test_branch_shapes_session(base, name):
    """Through compose_soa, the session path: smx_compose_async, then smx_compose_finish
    only when the counts ask for it."""
    soa, ref = _case(base, name)
    got = compose_soa(soa)
    plan = DeviceCompose.last_plan()
    _eq_soa(got, ref, f"{base}/{name} (session, plan {plan}, n_a={soa.n_a}, n_b={soa.n_b})")
    _check_plan(base, name, plan, "session")


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("base", ["lift", "small"])
def test_branch_shapes_window_plans(windows, base, name):
    """With the small plan off: every shape of the 2048-op base (empty, one-op and 16-op
    branches) goes through the window plans, as does whatever else shrinks that far."""
    soa, ref = _case(base, name)
    got = compose_soa(soa)
    plan = DeviceCompose.last_plan()
    _eq_soa(got, ref, f"{base}/{name} (small plan off, plan {plan}, n_a={soa.n_a}, n_b={soa.n_b})")
    assert plan != "small"
    if base != "small":
        _check_plan(base, name, plan, "windows")
    else:
        print(f"PLAN windows {base} {name} -> {plan}")


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("base", ["lift", "wide", "seg"])
def test_branch_shapes_synchronous(base, name):
    """Through DeviceCompose.run(), the synchronous smx_compose (verdict word, fallbacks
    inside the call)."""
    soa, ref = _case(base, name)
    dc = DeviceCompose(soa)
    dc.run()
    plan = dc.last_plan()
    _eq_soa(dc.results(), ref, f"{base}/{name} (synchronous, plan {plan}, n_a={soa.n_a}, n_b={soa.n_b})")
    _check_plan(base, name, plan, "sync")


@pytest.mark.parametrize("swap", [False, True], ids=["a_sorted_b_shuffled", "a_shuffled_b_sorted"])
def test_one_branch_shuffled(swap):
    """One branch from the timestamp-ordered `lift` base, the other from `shuf` (the same
    spec and seed: the same ops, each branch permuted): the generic plan takes it."""
    lift, shuf = _base("lift"), _base("shuf")
    assert lift.n_a == shuf.n_a and np.array_equal(np.sort(lift.oid_lo[:lift.n_a]), np.sort(shuf.oid_lo[:shuf.n_a]))
    first, second = (shuf, lift) if swap else (lift, shuf)
    a = pick(first, np.ones(first.n_a, bool), np.zeros(first.n_b, bool))
    b = pick(second, np.zeros(second.n_a, bool), np.ones(second.n_b, bool))
    cols = [np.concatenate([getattr(a, c), getattr(b, c)]) for c in ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")]
    soa = type(a)(a.n_a, b.n_b, *cols, a.n_sym, a.strings, a.ts_mode, a.id_mode)
    ref = oracle.compose(soa)
    got = compose_soa(soa)
    plan = DeviceCompose.last_plan()
    print(f"PLAN session mixed {'a_shuffled_b_sorted' if swap else 'a_sorted_b_shuffled'} -> {plan}")
    _eq_soa(got, ref, f"one branch shuffled (swap={swap}, plan {plan})")
    assert plan.startswith("radix"), plan


@pytest.mark.parametrize("name", ["a_sparse", "a_before_b"])
def test_branch_shapes_early_verdict(name):
    """The synchronous early verdict (merges from 4M ops: k_khist's long-group test, then
    the host picks the windows) on unbalanced logs.  The base is the c5-shaped spec of
    test_gpu_early_verdict_plans, at 8.5M ops so that the picked logs (a 1/64 of A against
    all of B: 4.3M ops; half of A before half of B: 4.25M) are still at or above the early
    verdict's size; synthesis and the oracle dominate the time."""
    key = ("base", "early")
    if key not in _cache:
        _cache[key] = synth.lift_soa(synth.lift_logs(synth.LiftSpec(8_500_000, 20_000, 79, ops_per_ms=4096, mix=ADV)))
    soa = shape(_cache[key], name, SEED)
    assert soa.n >= (1 << 22)
    dc = DeviceCompose(soa)
    dc.run()
    plan = dc.last_plan()
    print(f"PLAN sync early {name} -> {plan}")
    _eq_soa(dc.results(), oracle.compose(soa), f"early verdict, {name} (plan {plan}, n_a={soa.n_a}, n_b={soa.n_b})")
    if name == "a_before_b":
        _cache.pop(key)  # (the last case that uses it)


# ---------------------------------------------------------------------------
# the C ABI's corners (include/smx.h), through DeviceCompose's optional arguments


@pytest.mark.parametrize("b_gap", [1, 255, 4096])
@pytest.mark.parametrize("name", ["odd_sizes", "a_255", "a_empty"])
@pytest.mark.parametrize("base", ["lift", "wide", "small"])
def test_b_gap(base, name, b_gap):
    """Branch B's columns b_gap entries after A's, the gap filled with an invalid kind and
    symbol: the presorted, wide and small plans give the oracle's result of the log."""
    soa, ref = _case(base, name)
    dc = DeviceCompose(soa, b_gap=b_gap)
    dc.run()
    plan = dc.last_plan()
    _eq_soa(dc.results(), ref, f"{base}/{name} b_gap={b_gap} (plan {plan})")
    if name == "odd_sizes":
        assert plan == PLAN[base]


@pytest.mark.parametrize("base,words", [("shuf", "not timestamp-ordered"), ("seg", "timestamp groups too long")])
def test_b_gap_needs_presorted_plan(base, words):
    """include/smx.h: the sorting plans need b_gap = 0.  A gapped log that is not
    timestamp-ordered, or whose timestamp groups no presorted window holds (the segmented
    plan's logs), is refused with SMX_E_ARG."""
    soa, _ = _case(base, "odd_sizes")
    dc = DeviceCompose(soa, b_gap=1 if base == "shuf" else 255)
    with pytest.raises(SmxError) as e:
        dc.run()
    assert e.value.code == -1, str(e.value)  # SMX_E_ARG
    assert words in str(e.value) and "needs b_gap = 0" in str(e.value)


def _adv_small():
    """The first 1000 ops of each branch of `adv`: many conflicts on the small plan."""
    key = ("adv", "cut2000")
    if key not in _cache:
        adv = _base("adv")
        soa = pick(adv, np.arange(adv.n_a) < 1000, np.arange(adv.n_b) < 1000)
        _cache[key] = (soa, oracle.compose(soa))
    return _cache[key]


@pytest.mark.parametrize("cap", ["one_short", "zero"])
@pytest.mark.parametrize("plan", ["windows", "small"])
def test_conflict_cap_too_small(plan, cap):
    """include/smx.h: a conflict_cap below the number of conflicts is not an error of the
    call; counts[1] is the full number, the first conflict_cap pairs are written, nothing
    at or after conflicts[2 * conflict_cap] (64 guard words), the composed ops are whole."""
    soa, ref = _case("adv", "odd_sizes") if plan == "windows" else _adv_small()
    true = len(ref[4])
    assert true >= 2
    c = true - 1 if cap == "one_short" else 0
    dc = DeviceCompose(soa, conflict_cap=c)
    dc.counts.fill_(-7)
    dc.run()
    assert (dc.last_plan() == "small") == (plan == "small")
    assert dc.guard_intact(), "wrote past conflicts[2 * conflict_cap]"
    assert dc.counts.cpu().tolist() == [len(ref[0]), true]
    with pytest.raises(SmxError) as e:
        dc.results()
    assert e.value.code == -2
    _eq_soa(dc.results(truncated=True), ref[:4] + (ref[4][:c],), f"{plan} conflict_cap={c} of {true}")
    # the asynchronous half alone: the same
    dc = DeviceCompose(soa, conflict_cap=c)
    dc.run_async()
    dc.finish()
    assert dc.guard_intact() and dc.counts.cpu().tolist() == [len(ref[0]), true]
    _eq_soa(dc.results(truncated=True), ref[:4] + (ref[4][:c],), f"{plan} async conflict_cap={c} of {true}")


def test_conflict_cap_exact_and_negative():
    soa, ref = _case("adv", "odd_sizes")
    dc = DeviceCompose(soa, conflict_cap=len(ref[4]))
    dc.run()
    assert dc.guard_intact()
    _eq_soa(dc.results(), ref, "conflict_cap = number of conflicts")
    dc = DeviceCompose(soa, conflict_cap=-1)
    dc.counts.fill_(-7)
    with pytest.raises(SmxError) as e:
        dc.run()
    assert e.value.code == -1 and "conflict_cap" in str(e.value)
    assert dc.guard_intact() and dc.counts.cpu().tolist() == [-7, -7]


@pytest.mark.parametrize("base", ["lift", "small"])
def test_workspace_one_byte_short(base):
    soa, _ = _case(base, "odd_sizes")
    full = DeviceCompose(soa)
    assert full.ws_needed > 1
    for call in ("run", "run_async", "finish"):
        dc = DeviceCompose(soa, ws_bytes=full.ws_needed - 1)
        dc.counts.fill_(-7)
        with pytest.raises(SmxError) as e:
            getattr(dc, call)()
        assert e.value.code == -4, str(e.value)  # SMX_E_WORKSPACE
        assert str(full.ws_needed) in str(e.value), str(e.value)
        dc.torch.cuda.synchronize()
        assert dc.counts.cpu().tolist() == [-7, -7], f"{call}: counts touched"


def test_zero_ops():
    """n_a = n_b = 0: SMX_OK and counts {0, 0}, from the synchronous call and from both halves."""
    base = _base("lift")
    soa = pick(base, np.zeros(base.n_a, bool), np.zeros(base.n_b, bool))
    assert soa.n == 0
    for calls in (("run",), ("run_async", "finish")):
        dc = DeviceCompose(soa)
        dc.counts.fill_(-7)
        for call in calls:
            getattr(dc, call)()
        assert dc.counts.cpu().tolist() == [0, 0]
        assert all(len(x) == 0 for x in dc.results())
    assert all(len(x) == 0 for x in compose_soa(soa))


@pytest.mark.parametrize("sizes", [(0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("plan", ["small", "windows"])
def test_one_op(plan, sizes):
    """One op on one branch and none on the other (and one on each), on the small plan and,
    with it off, on the window plans: every kind of op in turn."""
    old = set_small_limit(2048 if plan == "small" else 0)
    try:
        base = _base("adv")
        for i in range(12):
            ka, kb = np.zeros(base.n_a, bool), np.zeros(base.n_b, bool)
            ka[i:i + sizes[0]] = True
            kb[i:i + sizes[1]] = True
            soa = pick(base, ka, kb)
            assert (soa.n_a, soa.n_b) == sizes
            ref = oracle.compose(soa)
            dc = DeviceCompose(soa)
            dc.counts.fill_(-7)
            dc.run()
            _eq_soa(dc.results(), ref, f"{plan} {sizes} op {i} (synchronous)")
            assert (dc.last_plan() == "small") == (plan == "small")
            _eq_soa(compose_soa(soa), ref, f"{plan} {sizes} op {i} (session)")
    finally:
        set_small_limit(old)
