"""GPU parity for the RGA replay (semantic_merge_amd/csrc/smx_rga.hip) where its kernels
branch: list sizes on both sides of every kernel and lane boundary, keys tied at every
level of (anchor, t, author, opid_hi, opid_lo, creation index), list mode
(smx_rga_out.out_tomb), every depth of the partition by list id, and tiny calls.

Every comparison is exact array equality against the CPU oracle (oracle/crdt_ref.c):
(values, src, offsets) of materialize(), (values, src, offsets, tombstones) of the list
state.  The oracle is run once per batch in list mode; materialize() is that state
without its tombstoned elements (tests/test_rga_oracle.py checks both against the
reference's own outputs)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import _abi, synth
from semantic_merge_amd._lib import lib, rga_replay_device

import _rga_shapes as shapes

pytestmark = pytest.mark.gpu

NAMES = ("values", "src", "offsets", "tombstones")


def _state(b):
    """The oracle's list state of b: (values, src, offsets, tombstones)."""
    return oracle.rga(*shapes.args(b), tombstones=True)


def _materialized(state):
    vals, src, offs, tomb = state
    live = np.concatenate([[0], np.cumsum(~tomb)])
    return vals[~tomb], src[~tomb], live[offs]


def _check(b, state, tombstones, grouped=False, label=""):
    want = state if tombstones else _materialized(state)
    got = rga_replay_device(b, tombstones=tombstones, grouped=grouped)
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, f"{label} {name}: {g.shape[0]} elements, the oracle has {w.shape[0]}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            lists = np.searchsorted(want[2], bad[:5], side="right") - 1 if name != "offsets" else bad[:5]
            raise AssertionError(f"{label} {name}: {bad.size} differ, first at {bad[:5].tolist()} "
                                 f"(lists {lists.tolist()})")


@functools.lru_cache(maxsize=None)
def _tie_case(regime, grouped):
    b = shapes.tie_batch(regime=regime)
    if grouped:
        b = shapes.grouped(b)
    state = _state(b)
    return b, state


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("regime", ["narrow", "wide"])
def test_rga_ties_at_every_size(regime, tombstones, grouped):
    """Lists of 0 to 5000 events (every kernel, every K, every boundary) whose keys tie at
    every level: rga_key_lt's tail, rw_order's tie runs, rec_lt in rga_big_list -- from the
    partitioned records (RecSrc) and, grouped, from the input columns (ColSrc)."""
    b, state = _tie_case(regime, grouped)
    shapes.assert_ties(b, state[1], state[2])
    if regime == "wide":  # key word 0 equal to the sorting network's padding value
        assert ((b.anchor[state[1]] == 0xFFFFFFFF) & (b.t[state[1]] == shapes.I64_MAX)).any()
    _check(b, state, tombstones, grouped, f"{regime}")


FULL = (64, 256, 257, 512, 513)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("tombstones", [False, True])
@pytest.mark.parametrize("regime", ["narrow", "one_key"])
def test_rga_full_networks(regime, tombstones, grouped):
    """Insert-only lists of exactly 64, 256 and 512 events fill their sorting network (no
    padding entries), 257 and 513 are the first sizes of the next kernel: every event
    survives, so a tie run ends at the network's last slot; with one key for all events
    the whole network is one run ordered by creation index."""
    b = shapes.tie_batch(FULL, seed=11, regime=regime, ops=(1, 0, 0))
    if grouped:
        b = shapes.grouped(b)
    state = _state(b)
    assert np.array_equal(np.diff(state[2]), FULL) and not state[3].any()  # every event survives
    counts = shapes.tie_counts(b, state[1], state[2])
    for l, size in enumerate(FULL):
        if regime == "one_key":
            assert counts[l] == [0, 0, 0, size - 1]
            assert np.array_equal(state[1][state[2][l]:state[2][l + 1]], np.flatnonzero(b.list_id == l))
        else:
            assert min(counts[l]) >= 1, f"list {l}: adjacent ties by level {counts[l]}"
            last = state[1][state[2][l + 1] - 2:state[2][l + 1]]  # the last slot is inside a tie run
            assert b.anchor[last[0]] == b.anchor[last[1]] and b.t[last[0]] >> 32 == b.t[last[1]] >> 32
    _check(b, state, tombstones, grouped, regime)


CHAIN = (256, 512, 513, 2049)


@pytest.mark.parametrize("tombstones", [True, False])
@pytest.mark.parametrize("ops", [(0.3, 0.4, 0.3), (0, 0, 1), (0, 1, 0)], ids=["mixed", "all_delete", "all_move"])
def test_rga_move_delete_chains_list_mode(ops, tombstones):
    """Two values per list: long per-value chains in which moves meet only tombstoned
    elements (the reference pops the first LIVE one, crdt.py:33-37, so nothing is popped)
    and deletes hit elements already tombstoned; lists of deletes alone and of moves
    alone.  In list mode the tombstoned elements, their places and their flags are
    compared too."""
    b = shapes.tie_batch(CHAIN, seed=18, regime="narrow", ops=ops, values_per_list=2)
    vals, src, offs, tomb = state = _state(b)
    sizes = np.diff(offs)
    if ops == (0, 0, 1):
        assert not sizes.any()
    elif ops == (0, 1, 0):
        assert np.array_equal(sizes, [2] * len(CHAIN)) and not tomb.any()  # one live element per value
    else:
        shapes.assert_ties(b, src, offs)
        for l in range(len(CHAIN)):  # live and tombstoned elements of one value
            v, tb = vals[offs[l]:offs[l + 1]], tomb[offs[l]:offs[l + 1]]
            assert np.intersect1d(v[tb], v[~tb]).size > 0, f"list {l}"
    _check(b, state, tombstones, False, "chains")
    g = shapes.grouped(b)
    _check(g, _state(g), tombstones, True, "chains grouped")


def _spread(n_ops, n_lists, seed):
    """synth.rga_batch with list 0 and the last list surely used."""
    b = synth.rga_batch(n_ops, n_lists, seed)
    b.list_id[0] = 0
    b.list_id[-1] = n_lists - 1
    return b


@pytest.mark.parametrize("n_lists,seed", [(1, 31), (256, 32), (257, 33), (65_536, 34), (65_537, 35)])
def test_rga_partition_depth(n_lists, seed):
    """The partition by list id on both sides of its switches: one pass up to 256 lists,
    the high-byte pass and per-bucket low-byte pass up to 65536, three LSD passes beyond
    (65537 is also the first n_lists past k_rga_out_fused)."""
    b = _spread(20_000, n_lists, seed)
    state = _state(b)
    assert state[3].any()
    _check(b, state, False, label=f"{n_lists} lists")
    _check(b, state, True, label=f"{n_lists} lists")


@pytest.mark.timeout(120)
def test_rga_partition_four_passes():
    """More than 2^24 lists: four LSD passes, the records ping-ponged twice.  The 20 000
    events' list ids cover the whole range (the top byte varies), list 0 and the last
    list included."""
    n_lists = (1 << 24) + 5
    b = _spread(20_000, n_lists, 36)
    assert len(np.unique(b.list_id >> 24)) == 2 and len(np.unique((b.list_id >> 16) & 255)) == 256
    state = _state(b)
    _check(b, state, True, label="2^24 + 5 lists")


@functools.lru_cache(maxsize=None)
def _tiny_case(n_ops, n_lists, ops=shapes.OPS):
    rng = np.random.default_rng(n_ops * 100_003 + n_lists)
    b = shapes.events(rng.integers(0, n_lists, size=n_ops), n_lists, 40 + n_ops + n_lists, "narrow", ops)
    return b, _state(b)


@pytest.mark.parametrize("n_lists", [1, 3, 300, 70_000])
@pytest.mark.parametrize("n_ops", [1, 2, 5, 64, 65, 1000])
def test_rga_tiny_ungrouped_calls(n_ops, n_lists):
    """Calls of a few events through the partition (one tile, mostly empty digit runs) at
    each of its depths, in both output modes."""
    b, state = _tiny_case(n_ops, n_lists)
    for l, c in shapes.tie_counts(b, state[1], state[2]).items():  # (lists of 63 events or more)
        assert min(c) >= 1, f"list {l}: adjacent ties by level {c}"
    _check(b, state, False, label="tiny")
    _check(b, state, True, label="tiny")


@pytest.mark.parametrize("n_lists", [1, 3, 300, 70_000])
def test_rga_only_deletes(n_lists):
    """A batch of deletes alone: no elements, every offset zero, in both modes."""
    b, state = _tiny_case(1000, n_lists, (0, 0, 1))
    assert state[0].size == 0 and not state[2].any()
    for tombstones in (False, True):
        got = rga_replay_device(b, tombstones=tombstones)
        assert all(g.size == 0 for g in got[:2] + got[3:])
        assert got[2].shape == (n_lists + 1,) and not got[2].any()
        _check(b, state, tombstones, label="deletes")


@pytest.mark.parametrize("tombstones", [False, True])
def test_rga_zero_events_through_the_abi(tombstones):
    """n_ops = 0 straight through the C ABI (the Python wrapper returns before the call):
    SMX_OK, offsets of all n_lists + 1 entries and counts zeroed, nothing else needed."""
    import torch
    dev = torch.device("cuda")
    n_lists = 7
    offs = torch.full((n_lists + 1,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((1,), 99, dtype=torch.int64, device=dev)
    tomb = torch.zeros(1, dtype=torch.uint8, device=dev)
    ops = _abi.SmxRgaOps(0, n_lists, *([None] * 8))
    out = _abi.SmxRgaOut(None, None, offs.data_ptr(), counts.data_ptr(), tomb.data_ptr() if tombstones else None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for call in ("smx_rga_replay", "smx_rga_replay_ex"):
        offs.fill_(-1)
        counts.fill_(99)
        torch.cuda.synchronize(dev)
        if call == "smx_rga_replay":
            rc = lib().smx_rga_replay(C.byref(ops), C.byref(out), None, 0, stream)
        else:
            rc = lib().smx_rga_replay_ex(C.byref(ops), C.byref(out), None, 0, 0, stream)
        assert rc == 0, lib().smx_last_error()
        torch.cuda.synchronize(dev)
        assert offs.cpu().tolist() == [0] * (n_lists + 1)
        assert counts.cpu().tolist() == [0]


@pytest.mark.parametrize("regime", ["narrow", "wide"])
def test_rga_grouped_claim_false_list_mode(regime):
    """SMX_RGA_GROUPED on interleaved events in list mode: the call redoes itself through
    the partition and still returns the whole list state."""
    b, state = _tie_case(regime, False)
    assert (np.diff(b.list_id.astype(np.int64)) < 0).any()
    shapes.assert_ties(b, state[1], state[2])
    _check(b, state, True, True, "claimed grouped")
