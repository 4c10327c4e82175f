"""GPU parity for smx_rga_replay_chain (semantic_merge_amd/csrc/smx_rga.hip, smx_rga_chain.h):
many jobs, each a strictly ascending run of segments, over segments stored once.

Expected results: the CPU oracle (oracle/crdt_ref.c) on the batch whose list j is job j's
segments' events one segment after another, its src mapped back to column indices.  Every
comparison is exact array equality of (values, src, offsets), plus the tombstones in list mode.
The job totals stand on both sides of every size at which the list kernels change path (one
event per lane up to 64, k_rga_wave up to 256, k_rga_wave2 up to 512, k_rga_big beyond), each
cut into segments five ways; the coverage conditions (a tied insert two segments after the
element it ties with, a delete and a move of the last segment that reach what the first created,
a survivor of the first segment; ties at every level of the key) are asserted on the oracle's
output."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd._lib import lib, rga_replay_chain_device
from semantic_merge_amd.crdt import RgaChainBatch

import _rga_chain as chain
import _rga_onto as onto
import _rga_shapes as shapes

pytestmark = pytest.mark.gpu

NAMES = ("values", "src", "offsets", "tombstones")
SMX_E_ARG = -1
EDGE_TOTALS = (64, 65, 256, 257, 512, 513, 1024, 1025, 3001)
CUTS = 5                       # ways each total is cut
SHARED_LEN, SHARED_JOBS = 200, 300
STACK, STACK_LEN = 12, 40
GRID, GRID_LEN = (3, 4, 5), (60, 30, 30)  # bases x targets x pull requests; their lengths
SEEDS = {"narrow": 4, "wide": 4, "one_key": 4}


def edge_shape():
    """(segment lengths, families, jobs, marks): marks name the jobs and segments the test
    asserts on.  Segments are made in the order the jobs name them, so every job ascends."""
    seg_len, family, jobs, marks = [], [], [], {}
    fam = iter(range(1 << 20))
    rng = np.random.default_rng(5)

    def segs(lengths, f=None):
        f = next(fam) if f is None else f
        first = len(seg_len)
        seg_len.extend(int(x) for x in lengths)
        family.extend([f] * len(lengths))
        return list(range(first, first + len(lengths)))

    e, one = segs([0, 1])
    jobs += [[], [e], [one], [e, one]]  # totals 0 and 1
    marks["empty_middle"] = []
    for total in EDGE_TOTALS:
        jobs.append(segs([total]))
        jobs.append(segs([total - 1, 1]))
        jobs.append(segs([1, total - 1]))
        marks["empty_middle"].append(len(jobs))
        jobs.append(segs([total // 2, 0, total - total // 2]))
        cut = np.sort(rng.integers(0, total + 1, size=39))  # about 40 segments of uneven length
        jobs.append(segs(np.diff(np.concatenate([[0], cut, [total]]))))
        if total == 257:
            marks["unused"] = segs([50])[0]
    # one segment under 300 jobs, in all three size classes
    f = next(fam)
    shared = segs([SHARED_LEN], f)[0]
    marks["shared"] = shared
    jobs += [[shared, s] for s in segs(list(range(SHARED_JOBS)) + [320, 400], f)]
    # a stack of commits with its prefixes, and jobs that skip segments of it
    stack = segs([STACK_LEN] * STACK)
    marks["prefix"] = list(range(len(jobs), len(jobs) + STACK))
    jobs += [stack[:k + 1] for k in range(STACK)]
    marks["skip"] = list(range(len(jobs), len(jobs) + 4))
    jobs += [[stack[0], stack[2], stack[5], stack[11]], [stack[1], stack[3]], [stack[0], stack[11]],
             [stack[0], stack[4], stack[5], stack[6], stack[9]]]
    # the three-way grid: base ++ target ++ pull request
    f = next(fam)
    bases, targets, prs = (segs([n] * k, f) for k, n in zip(GRID, GRID_LEN))
    marks["grid"] = list(range(len(jobs), len(jobs) + len(bases) * len(targets) * len(prs)))
    jobs += [[b, t, p] for b in bases for t in targets for p in prs]
    order = np.random.default_rng(99).permutation(len(jobs))  # the jobs in any order
    where = np.argsort(order)
    marks = {k: (where[v].tolist() if k in ("empty_middle", "prefix", "skip", "grid") else v) for k, v in marks.items()}
    return seg_len, family, [jobs[i] for i in order], marks


@functools.lru_cache(maxsize=None)
def _edge_case(regime):
    seg_len, family, jobs, marks = edge_shape()
    batch = chain.build(seg_len, jobs, SEEDS[regime], regime, family)
    return (batch,) + chain.expected(batch) + (chain.covered(seg_len, family, jobs), marks)


def _compare(got, want, label):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, f"{label} {name}: {g.shape[0]} elements, the oracle has {w.shape[0]}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            at = np.searchsorted(want[2], bad[:5], side="right") - 1 if name != "offsets" else bad[:5]
            raise AssertionError(f"{label} {name}: {bad.size} differ, first at {bad[:5].tolist()} (jobs {at.tolist()})")


def _check(batch, want, tombstones, label=""):
    _compare(rga_replay_chain_device(batch, tombstones=tombstones), want if tombstones else onto.materialized(want),
             label)


@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("regime", ["narrow", "wide", "one_key"])
def test_chain_at_every_size_and_cut(regime, tombstones):
    batch, ex, idx, state, want, covered, marks = _edge_case(regime)
    total, nseg = batch.job_len, np.diff(batch.job_off)
    seg_len = np.diff(batch.seg_off)
    segs = [chain.job_segments(batch, j) for j in range(batch.n_jobs)]
    # the shape: every total, each from 64 up at its five cuts
    assert {0, 1, *EDGE_TOTALS} <= set(total.tolist())
    for t in EDGE_TOTALS:
        cuts = {tuple(seg_len[s].tolist()) if len(s) <= 3 else len(s) for s, tt in zip(segs, total) if tt == t}
        assert {(t,), (t - 1, 1), (1, t - 1), (t // 2, 0, t - t // 2), 40} <= cuts, t
    uneven = [seg_len[s] for s in segs if len(s) == 40]
    assert len(uneven) == len(EDGE_TOTALS) and all(len(set(u.tolist())) >= 3 for u in uneven)
    # the shared segment's jobs in the three size classes; the prefixes; the grid; skips; shuffled; unused
    of_shared = np.asarray([marks["shared"] in s for s in segs])
    assert of_shared.sum() == SHARED_JOBS + 2
    assert (total[of_shared] <= 256).any() and (total[of_shared] > 512).any()
    assert ((total[of_shared] > 256) & (total[of_shared] <= 512)).any()
    first = segs[marks["prefix"][0]][0]
    assert [segs[j] for j in marks["prefix"]] == [list(range(first, first + k + 1)) for k in range(STACK)]
    assert len(marks["grid"]) == 60 and len({tuple(segs[j]) for j in marks["grid"]}) == 60
    assert all(len(segs[j]) == 3 for j in marks["grid"])
    assert all((np.diff(segs[j]) > 1).any() for j in marks["skip"])
    assert all((np.diff(s) > 0).all() for s in segs) and (np.diff([s[0] for s in segs if s]) < 0).any()
    assert not (batch.job_seg == marks["unused"]).any() and seg_len[marks["unused"]] > 0
    assert batch.n_out - batch.n >= SHARED_JOBS * SHARED_LEN  # the shared segment is stored once
    # coverage, on the oracle's output: strictly the jobs the shape promises
    promised = marks["empty_middle"] + marks["prefix"][2:] + marks["grid"] + [marks["skip"][0], marks["skip"][3]]
    assert set(promised) <= set(covered) and len(promised) == len(EDGE_TOTALS) + (STACK - 2) + 60 + 2
    assert chain.coverage(batch, want, covered) == len(covered)
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
    seg_len = [3, 0, 5, 2, 1, 4]
    jobs = [[s for s in range(6) if ((j * 7) % 64) >> s & 1] for j in range(nj)]
    batch = chain.build(seg_len, jobs, 21, "narrow")
    return (batch,) + chain.expected(batch)


@pytest.mark.parametrize("tombstones", [False, True])
def test_chain_more_jobs_than_the_fused_output_takes(tombstones):
    batch, ex, idx, state, want = _many_case()
    assert batch.n_jobs > 65_536 and state[3].any() and batch.job_len.max() == 15 and batch.job_len.min() == 0
    _check(batch, want, tombstones, "many jobs")


SMALL_LEN = [40, 9, 300, 30, 5, 270, 12]  # (segment 1: in no job)
SMALL_JOBS = [[0, 3], [2, 4], [6], [], [0, 2, 5]]


@functools.lru_cache(maxsize=None)
def _small_case():
    batch = chain.build(SMALL_LEN, SMALL_JOBS, 31, "narrow")
    return (batch,) + chain.expected(batch)


def _ws(*sizes):
    import torch
    return torch.empty(max(sizes), dtype=torch.uint8, device="cuda")


def _chain_ws_bytes(b):
    return chain.workspace_bytes(lib(), b.n_jobs, b.n_links, b.n_out)


def _as_chain(b):
    """An onto batch as a chain batch over the same columns: the bases, then the own streams."""
    assert b.base_off[-1] == b.own_off[0]
    nb = b.n_bases
    jobs = [([int(b.job_base[j])] if b.job_base[j] >= 0 else []) + [nb + j] for j in range(b.n_jobs)]
    job_off = np.concatenate([[0], np.cumsum([len(j) for j in jobs])]).astype(np.int64)
    job_seg = np.asarray([s for j in jobs for s in j], np.int32)
    return RgaChainBatch(nb + b.n_jobs, b.n_jobs, np.concatenate([b.base_off, b.own_off[1:]]), job_off, job_seg,
                         b.op, b.value, b.anchor, b.t, b.author, b.opid_hi, b.opid_lo, [])


@pytest.mark.parametrize("tombstones", [False, True])
def test_chain_of_base_and_own_is_onto_bit_for_bit(tombstones):
    base_len = [40, 9, 300, 0, 256, 700]
    jobs = [(0, 30), (2, 5), (None, 12), (0, 0), (2, 270), (4, 1), (4, 0), (None, 257), (3, 64), (5, 90), (None, 0),
            (5, 0), (0, 216), (0, 217), (2, 212), (2, 213)]
    b = onto.build(base_len, jobs, 33, "narrow")
    c = _as_chain(b)
    assert c.n_out == b.n_out and np.array_equal(c.job_len, b.job_len)
    ws = _ws(onto.workspace_bytes(lib(), b.n_jobs, b.n_out), _chain_ws_bytes(c))
    rc, want = onto.run_onto(lib(), b, tombstones, ws)
    assert rc == 0, lib().smx_last_error()
    rc, got = chain.run_chain(lib(), c, tombstones, ws)
    assert rc == 0, lib().smx_last_error()
    assert want[0].size > 1000
    _compare(got, want, "chain against onto")


def test_replay_ex_and_onto_are_unchanged_around_a_chain_call():
    """smx_rga_replay_ex (partitioned and grouped) on an unrelated batch and smx_rga_replay_onto,
    before and after a chain call on the same workspace: identical results (the oracle's), in
    both modes."""
    b = shapes.tie_batch((0, 1, 64, 257, 600, 130), seed=3)
    g = shapes.grouped(b)
    ob = onto.build([40, 9, 300], [(0, 30), (2, 5), (None, 12), (0, 0), (2, 270)], 31, "narrow")
    owant = onto.expected(ob)[3]
    batch, _, _, _, want = _small_case()
    need = C.c_size_t(0)
    assert lib().smx_rga_workspace_bytes(b.n, b.n_lists, C.byref(need)) == 0
    ws = _ws(need.value, onto.workspace_bytes(lib(), ob.n_jobs, ob.n_out), _chain_ws_bytes(batch))

    def others(tombstones):
        res = [onto.run_replay_ex(lib(), x, tombstones, ws, flags) for x, flags in ((b, 0), (g, 1))]
        rc, r = onto.run_onto(lib(), ob, tombstones, ws)
        assert rc == 0, lib().smx_last_error()
        return res + [r]

    for tombstones in (False, True):
        before = others(tombstones)
        rc, got = chain.run_chain(lib(), batch, tombstones, ws)
        assert rc == 0, lib().smx_last_error()
        _compare(got, want if tombstones else onto.materialized(want), "chain")
        after = others(tombstones)
        states = [oracle.rga(*shapes.args(x), tombstones=True) for x in (b, g)] + [owant]
        for state, bef, aft in zip(states, before, after):
            _compare(bef, state if tombstones else onto.materialized(state), "before")
            _compare(aft, bef, "after")


def test_two_chain_shapes_share_one_workspace():
    big, _, _, _, want_big = _edge_case("narrow")[:5]
    small, _, _, _, want_small = _small_case()
    ws = _ws(_chain_ws_bytes(big), _chain_ws_bytes(small))
    for batch, want, tombstones in ((big, want_big, True), (small, want_small, False), (small, want_small, True),
                                    (big, want_big, False), (small, want_small, True)):
        rc, got = chain.run_chain(lib(), batch, tombstones, ws)
        assert rc == 0, lib().smx_last_error()
        _compare(got, want if tombstones else onto.materialized(want), f"{batch.n_jobs} jobs")


def test_invalid_input_is_an_argument_error():
    """Found on the device, before a kernel reads a column through an unchecked offset:
    SMX_E_ARG, and the next call on the same workspace is served."""
    good, _, _, _, want = _small_case()
    ws = _ws(_chain_ws_bytes(good))
    assert good.job_len.tolist() == [70, 305, 12, 0, 610]

    def variant(change):
        v = copy.deepcopy(good)
        change(v)
        return v

    def put(name, i, x):
        return variant(lambda v: getattr(v, name).__setitem__(i, x))

    def swap(v, a, b):
        v.job_seg[a], v.job_seg[b] = v.job_seg[b], v.job_seg[a]

    long_links = int(good.job_off[4])  # job 4 = segments 0, 2, 5
    bad = {
        "seg_off negative": put("seg_off", 0, -1),
        "seg_off decreasing": put("seg_off", 2, int(good.seg_off[1]) - 1),
        "seg_off past n_total": put("seg_off", -1, good.n + 1),
        "job_off negative": put("job_off", 0, -1),
        "job_off decreasing": put("job_off", 2, int(good.job_off[1]) - 1),
        "job_off past n_links": put("job_off", -1, good.n_links + 1),
        "job_seg = n_segs": put("job_seg", 1, good.n_segs),
        "job_seg = -1": put("job_seg", 2, -1),
        "job_seg far outside": put("job_seg", long_links + 2, 1 << 30),
        "a segment twice in a job": put("job_seg", 1, 0),
        "segments descending in a short job": variant(lambda v: swap(v, 0, 1)),
        "segments descending at the end of a long job": variant(lambda v: swap(v, long_links + 1, long_links + 2)),
        "op = 3 in a short job's segment": put("op", int(good.seg_off[6]) + 3, 3),
        "op = 3 at the last event of a long job's middle segment": put("op", int(good.seg_off[3]) - 1, 3),
        "op = 255 in a segment two jobs name": put("op", int(good.seg_off[0]), 255),
    }
    n_out = good.n_out
    for tombstones in (False, True):
        for label, v in bad.items():
            rc, _ = chain.run_chain(lib(), v, tombstones, ws, n_out=n_out)
            assert rc == SMX_E_ARG, label
            assert b"invalid input" in lib().smx_last_error(), label
        rc, _ = chain.run_chain(lib(), good, tombstones, ws, n_out=n_out - 1)
        assert rc == SMX_E_ARG, "n_out one short"
        assert b"invalid input" in lib().smx_last_error()
        # a segment named by no job is never read: an op = 3 there is not this call's input
        rc, got = chain.run_chain(lib(), put("op", int(good.seg_off[1]) + 3, 3), tombstones, ws)
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
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    q = _abi.SmxRgaChain(0, 0, 0, 0, 0, zero.data_ptr(), zero.data_ptr(), *([None] * 8))
    out = _abi.SmxRgaOut(None, None, offs.data_ptr(), counts.data_ptr(), tomb.data_ptr() if tombstones else None)
    rc = lib().smx_rga_replay_chain(C.byref(q), C.byref(out), None, 0, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib().smx_last_error()
    torch.cuda.synchronize(dev)
    assert offs.cpu().tolist() == [0] and counts.cpu().tolist() == [0]
    batch = chain.build([0, 0], [[0], [], [0, 1]], 1, "narrow")
    got = rga_replay_chain_device(batch, tombstones=tombstones)
    assert all(g.size == 0 for g in got[:2] + got[3:]) and got[2].tolist() == [0, 0, 0, 0]
