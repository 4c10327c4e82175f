"""GPU parity for smx_rga_replay_onto (semantic_merge_amd/csrc/smx_rga.hip, smx_rga_onto.h):
many jobs, each a base's events followed by its own, over bases stored once.

Expected results: the CPU oracle (oracle/crdt_ref.c) on the batch whose list j is job j's
base events followed by its own, its src mapped back to column indices.  Every comparison is
exact array equality of (values, src, offsets), plus the tombstones in list mode.  The job
totals stand on both sides of every size at which the list kernels change path (one event per
lane up to 64, k_rga_wave up to 256, k_rga_wave2 up to 512, k_rga_big beyond), with the cut
between base and own events at each end; the coverage conditions (own moves, deletes and tied
inserts that reach base-created elements; ties at every level of the key) are asserted on the
oracle's output."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd._lib import lib, rga_replay_onto_device

import _rga_onto as onto
import _rga_shapes as shapes

pytestmark = pytest.mark.gpu

NAMES = ("values", "src", "offsets", "tombstones")
SMX_E_ARG = -1
EDGE_TOTALS = (64, 65, 256, 257, 512, 513, 1024, 1025)
SHARED_LEN, SHARED_JOBS = 200, 300
SEEDS = {"narrow": 2, "wide": 2, "one_key": 2}


def edge_shape():
    """(base lengths, jobs, the index of the base that 300 jobs share, of the one no job names)."""
    base_len, jobs = [], []

    def base(n):
        base_len.append(n)
        return len(base_len) - 1

    empty = base(0)
    jobs += [(None, 0), (empty, 0), (None, 1), (empty, 1), (base(1), 0)]  # totals 0 and 1
    for total in EDGE_TOTALS:
        jobs += [(base(total - 1), 1), (base(1), total - 1), (base(total), 0), (None, total)]
        if total == 257:
            unused = base(50)
    jobs.append((base(1500), 1500))  # one job of about 3000
    shared = base(SHARED_LEN)  # with its jobs in all three size classes
    jobs += [(shared, k) for k in range(SHARED_JOBS)] + [(shared, 320), (shared, 400)]
    order = np.random.default_rng(99).permutation(len(jobs))
    return base_len, [jobs[i] for i in order], shared, unused


@functools.lru_cache(maxsize=None)
def _edge_case(regime):
    base_len, jobs, shared, unused = edge_shape()
    batch = onto.build(base_len, jobs, SEEDS[regime], regime)
    return (batch,) + onto.expected(batch) + (shared, unused)


def _compare(got, want, label):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, f"{label} {name}: {g.shape[0]} elements, the oracle has {w.shape[0]}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            at = np.searchsorted(want[2], bad[:5], side="right") - 1 if name != "offsets" else bad[:5]
            raise AssertionError(f"{label} {name}: {bad.size} differ, first at {bad[:5].tolist()} (jobs {at.tolist()})")


def _check(batch, want, tombstones, label=""):
    _compare(rga_replay_onto_device(batch, tombstones=tombstones), want if tombstones else onto.materialized(want),
             label)


@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("regime", ["narrow", "wide", "one_key"])
def test_onto_at_every_size_and_cut(regime, tombstones):
    batch, ex, idx, state, want, shared, unused = _edge_case(regime)
    total, own = batch.job_len, np.diff(batch.own_off)
    # the shape: every total, each from 64 up at its four cuts; the classes of the shared base's jobs
    assert {0, 1, *EDGE_TOTALS} <= set(total.tolist()) and (total > 2900).any()
    for t in EDGE_TOTALS:
        cuts = {(int(o), int(b) < 0) for o, b in zip(own[total == t], batch.job_base[total == t])}
        assert {(1, False), (t - 1, False), (0, False), (t, True)} <= cuts, t
    of_shared = batch.job_base == shared
    assert of_shared.sum() == SHARED_JOBS + 2 and set(own[of_shared].tolist()) >= set(range(SHARED_JOBS))
    assert (total[of_shared] <= 256).any() and (total[of_shared] > 512).any()
    assert ((total[of_shared] > 256) & (total[of_shared] <= 512)).any()
    assert not (batch.job_base == unused).any() and np.diff(batch.base_off)[unused] > 0
    assert (np.diff(batch.job_base[batch.job_base >= 0]) < 0).any()  # the bases named in any order
    assert batch.n_out - batch.n >= SHARED_JOBS * SHARED_LEN  # the shared base is stored once
    # coverage, on the oracle's output
    assert onto.coverage(batch, want) >= SHARED_JOBS - onto.COVERED_OWN + len(EDGE_TOTALS)
    if regime == "one_key":  # one tie run per job, ordered by the creation index alone
        for c in shapes.tie_counts(ex, state[1], state[2]).values():
            assert c[:3] == [0, 0, 0] and c[3] >= 1
        for j in np.flatnonzero(total >= 63):
            s = want[1][want[2][j]:want[2][j + 1]]
            assert (np.diff(s) > 0).all(), f"job {j}: not in column order"
    else:
        shapes.assert_ties(ex, state[1], state[2])
    if regime == "wide":  # key word 0 equal to the sorting network's padding value
        assert ((batch.anchor[want[1]] == 0xFFFFFFFF) & (batch.t[want[1]] == shapes.I64_MAX)).any()
    assert state[3].any() and not state[3].all()
    _check(batch, want, tombstones, regime)


@functools.lru_cache(maxsize=None)
def _many_case():
    """More jobs than k_rga_out_fused takes (RGA_FUSED_MAX = 65536): the scan output path."""
    nj = 65_536 + 70
    j = np.arange(nj)
    base_len = [3, 0, 5, 2]
    jobs = [(None if b == 4 else int(b), int(n)) for b, n in zip((j * 7) % 5, (j * 3) % 4)]
    batch = onto.build(base_len, jobs, 21, "narrow")
    return (batch,) + onto.expected(batch)


@pytest.mark.parametrize("tombstones", [False, True])
def test_onto_more_jobs_than_the_fused_output_takes(tombstones):
    batch, ex, idx, state, want = _many_case()
    assert batch.n_jobs > 65_536 and state[3].any() and batch.job_len.max() <= 8
    _check(batch, want, tombstones, "many jobs")


@functools.lru_cache(maxsize=None)
def _small_case():
    batch = onto.build([40, 9, 300], [(0, 30), (2, 5), (None, 12), (0, 0), (2, 270)], 31, "narrow")  # (base 1: unused)
    return (batch,) + onto.expected(batch)


def _ws(*sizes):
    import torch
    return torch.empty(max(sizes), dtype=torch.uint8, device="cuda")


def test_replay_ex_is_unchanged_around_an_onto_call():
    """smx_rga_replay_ex on an unrelated batch, before and after an onto call on the same
    workspace: identical results (the oracle's), grouped and partitioned, in both modes."""
    b = shapes.tie_batch((0, 1, 64, 257, 600, 130), seed=3)
    g = shapes.grouped(b)
    batch, _, _, _, want = _small_case()
    need = C.c_size_t(0)
    assert lib().smx_rga_workspace_bytes(b.n, b.n_lists, C.byref(need)) == 0
    ws = _ws(need.value, onto.workspace_bytes(lib(), batch.n_jobs, batch.n_out))
    for tombstones in (False, True):
        before = [onto.run_replay_ex(lib(), x, tombstones, ws, flags) for x, flags in ((b, 0), (g, 1))]
        rc, got = onto.run_onto(lib(), batch, tombstones, ws)
        assert rc == 0, lib().smx_last_error()
        _compare(got, want if tombstones else onto.materialized(want), "onto")
        after = [onto.run_replay_ex(lib(), x, tombstones, ws, flags) for x, flags in ((b, 0), (g, 1))]
        for x, bef, aft in zip((b, g), before, after):
            state = oracle.rga(*shapes.args(x), tombstones=True)
            _compare(bef, state if tombstones else onto.materialized(state), "replay_ex before")
            _compare(aft, bef, "replay_ex after")


def test_two_onto_shapes_share_one_workspace():
    big, _, _, _, want_big = _edge_case("narrow")[:5]
    small, _, _, _, want_small = _small_case()
    ws = _ws(onto.workspace_bytes(lib(), big.n_jobs, big.n_out), onto.workspace_bytes(lib(), small.n_jobs, small.n_out))
    for batch, want, tombstones in ((big, want_big, True), (small, want_small, False), (small, want_small, True),
                                    (big, want_big, False), (small, want_small, True)):
        rc, got = onto.run_onto(lib(), batch, tombstones, ws)
        assert rc == 0, lib().smx_last_error()
        _compare(got, want if tombstones else onto.materialized(want), f"{batch.n_jobs} jobs")


def test_invalid_input_is_an_argument_error():
    """Found on the device, before a list kernel reads a column: SMX_E_ARG, and the next call on
    the same workspace is served."""
    good, _, _, _, want = _small_case()
    ws = _ws(onto.workspace_bytes(lib(), good.n_jobs, good.n_out))

    def variant(change):
        v = copy.deepcopy(good)
        change(v)
        return v

    def op3(v, base):
        v.op[v.base_off[base] + 3] = 3

    def decreasing(v):
        v.own_off[2] = v.own_off[1] - 1

    def base_past_own(v):
        v.base_off[-1] = v.own_off[0] + 1

    bad = {
        "op = 3 in a base that a job uses": variant(lambda v: op3(v, 0)),
        "op = 3 in an own stream": variant(lambda v: v.op.__setitem__(int(v.own_off[2]), 3)),
        "op = 255 in a long job's base": variant(lambda v: v.op.__setitem__(int(v.base_off[2]) + 299, 255)),
        "job_base = n_bases": variant(lambda v: v.job_base.__setitem__(1, v.n_bases)),
        "job_base = -2": variant(lambda v: v.job_base.__setitem__(2, -2)),
        "own_off decreasing": variant(decreasing),
        "own_off past n_total": variant(lambda v: v.own_off.__setitem__(-1, v.n + 1)),
        "base_off negative": variant(lambda v: v.base_off.__setitem__(0, -1)),
        "bases not before the own events": variant(base_past_own),
    }
    n_out = good.n_out
    for tombstones in (False, True):
        for label, v in bad.items():
            rc, _ = onto.run_onto(lib(), v, tombstones, ws, n_out=n_out)
            assert rc == SMX_E_ARG, label
            assert b"invalid input" in lib().smx_last_error(), label
        rc, _ = onto.run_onto(lib(), good, tombstones, ws, n_out=n_out - 1)
        assert rc == SMX_E_ARG, "n_out one short"
        # a base named by no job is never read: an op = 3 there is not this call's input
        rc, got = onto.run_onto(lib(), variant(lambda v: op3(v, 1)), tombstones, ws)
        assert rc == 0, lib().smx_last_error()
        _compare(got, want if tombstones else onto.materialized(want), "after the errors")


@pytest.mark.parametrize("tombstones", [False, True])
def test_no_jobs_and_empty_jobs_through_the_abi(tombstones):
    """n_jobs = 0 writes out_offsets[0] = 0 and counts[0] = 0 and needs no workspace; jobs
    that are all empty give all-zero offsets."""
    import torch
    from semantic_merge_amd import _abi
    dev = torch.device("cuda")
    offs = torch.full((1,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((1,), 99, dtype=torch.int64, device=dev)
    tomb = torch.zeros(1, dtype=torch.uint8, device=dev)
    boff = torch.zeros(1, dtype=torch.int64, device=dev)
    q = _abi.SmxRgaOnto(0, 0, 0, 0, boff.data_ptr(), boff.data_ptr(), *([None] * 8))
    out = _abi.SmxRgaOut(None, None, offs.data_ptr(), counts.data_ptr(), tomb.data_ptr() if tombstones else None)
    rc = lib().smx_rga_replay_onto(C.byref(q), C.byref(out), None, 0, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib().smx_last_error()
    torch.cuda.synchronize(dev)
    assert offs.cpu().tolist() == [0] and counts.cpu().tolist() == [0]
    batch = onto.build([0, 0], [(0, 0), (None, 0), (1, 0)], 1, "narrow")
    got = rga_replay_onto_device(batch, tombstones=tombstones)
    assert all(g.size == 0 for g in got[:2] + got[3:]) and got[2].tolist() == [0, 0, 0, 0]
