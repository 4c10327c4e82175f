"""Loader for libsmx.so (the HIP library), the table of the op columns and the small direct
calls.  The product's path through the library is _session.py; the resident-buffer rigs of
tests, tools and bench.py are _rigs.py.  PyTorch-ROCm only owns device memory and names the
current HIP stream; every computation happens in libsmx's kernels through the C ABI of
include/smx.h.  There is no CPU fallback: without the library or a GPU these functions raise."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMX_LIB", os.path.join(HERE, "libsmx.so"))
_lib: Optional[C.CDLL] = None

# The seven columns of an op log (include/smx.h smx_ops): name, dtype (its itemsize is the
# column's width in bytes) and the signed dtype torch views it as.
OP_COLS = tuple((name, np.dtype(dt), np.dtype(view)) for name, dt, view in (
    ("kind", np.uint8, np.uint8), ("ts", np.uint64, np.int64), ("oid_hi", np.uint64, np.int64),
    ("oid_lo", np.uint64, np.int64), ("sym", np.uint32, np.int32), ("v0", np.int32, np.int32),
    ("v1", np.int32, np.int32)))
SCREEN_COLS = tuple(c for c in OP_COLS if c[0] != "v1")                # smx_screen reads no v1
CAND_COLS = tuple(c for c in OP_COLS if c[0] in ("kind", "sym", "v0"))  # smx_screen_candidates


class SmxError(RuntimeError):
    def __init__(self, code: int, msg: str) -> None:
        super().__init__(f"smx error {code}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libsmx.so not built at {LIB_PATH}; run __graft_entry__.build()")
        _lib = _abi.declare(C.CDLL(LIB_PATH))
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise SmxError(rc, lib().smx_last_error().decode(errors="replace"))


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("semantic_merge_amd needs a ROCm GPU (torch.cuda.is_available() is False)")
    return torch


def _ptr(t) -> int:
    return t.data_ptr() if t is not None and t.numel() > 0 else 0


_hip: Optional[C.CDLL] = None


def _hiprt() -> C.CDLL:
    """The HIP runtime the process already runs (torch's, which libsmx shares: the same
    soname), for the session's two copies and its one stream sync -- a ctypes call each,
    against ~10 us of torch dispatch per copy_ / stream context on a 1k-op merge."""
    global _hip
    if _hip is None:
        _torch()
        lib()
        # the copy this process already mapped (torch's; libsmx resolved to it), by its
        # path: dlopen returns that same copy, never a second runtime
        path = None
        with open("/proc/self/maps") as fh:
            for line in fh:
                f = line.split()[-1] if line.strip() else ""
                if os.path.basename(f).startswith("libamdhip64.so"):
                    path = f
                    break
        if path is None:
            raise RuntimeError("the HIP runtime (libamdhip64) is not loaded in this process")
        h = C.CDLL(path)
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        h.hipMemcpyAsync.restype = C.c_int
        h.hipStreamSynchronize.argtypes = [C.c_void_p]
        h.hipStreamSynchronize.restype = C.c_int
        _hip = h
    return _hip


def _hip_check(rc: int, what: str) -> None:
    if rc != 0:
        raise SmxError(rc, f"{what} failed (hipError_t {rc})")


def _rename_counts(kind, log_off) -> np.ndarray:
    """Renames per log (i64 [n_logs]) of a LogsSoA's kind column."""
    csum = np.concatenate([[0], np.cumsum(np.asarray(kind) == 1, dtype=np.int64)])  # SMX_KIND_RENAME
    off = np.clip(np.asarray(log_off, np.int64), 0, len(csum) - 1)
    return np.maximum(csum[off[1:]] - csum[off[:-1]], 0)


def set_small_limit(n: int) -> int:
    """Merges of at most n ops (0..2048) take the one-workgroup plan; returns the old limit."""
    return int(lib().smx_set_small_limit(int(n)))


def stage_times():
    """{stage: (total_ms, calls)} accumulated while smx_set_profiling(1)."""
    L = lib()
    ms = (C.c_double * 16)()
    calls = (C.c_int64 * 16)()
    n = L.smx_stage_times(ms, calls, 16)
    return {L.smx_stage_name(i).decode(): (ms[i], calls[i]) for i in range(n)}


def rga_replay_device(batch, device: str = "cuda", tombstones: bool = False, grouped: bool = False):
    """(values, src, offsets) of a batched RGA replay computed on the GPU; with
    tombstones=True the whole list state (live and tombstoned elements, crdt.py RGA.list)
    and a fourth array, the tombstone flags.  grouped=True: the batch's events come list
    by list (non-decreasing list ids, as crdt.marshal_streams builds them): the library
    skips its partition by list (it checks the claim and partitions when it is false)."""
    torch = _torch()
    dev = torch.device(device)
    n = batch.n
    if n == 0:
        e = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(batch.n_lists + 1, np.int64))
        return e + (np.zeros(0, np.bool_),) if tombstones else e

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    ins = [up(batch.list_id, np.int32), up(batch.op, np.uint8), up(batch.value, np.int32),
           up(batch.anchor, np.int32), up(batch.t, np.int64), up(batch.author, np.int32),
           up(batch.opid_hi, np.int64), up(batch.opid_lo, np.int64)]
    vals, src = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    offs = torch.empty(batch.n_lists + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    tomb = torch.empty(n, dtype=torch.uint8, device=dev) if tombstones else None
    ws = C.c_size_t(0)
    check(lib().smx_rga_workspace_bytes(n, batch.n_lists, C.byref(ws)))
    wst = torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)
    ops = _abi.SmxRgaOps(n, batch.n_lists, *[_ptr(t) for t in ins])
    out = _abi.SmxRgaOut(_ptr(vals), _ptr(src), _ptr(offs), _ptr(counts), _ptr(tomb))
    check(lib().smx_rga_replay_ex(C.byref(ops), C.byref(out), _ptr(wst), ws.value,
                                  _abi.RGA_GROUPED if grouped else 0,
                                  torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    k = int(counts.item())
    res = (vals[:k].cpu().numpy().view(np.uint32), src[:k].cpu().numpy(), offs.cpu().numpy())
    return res + (tomb[:k].cpu().numpy().astype(np.bool_),) if tombstones else res


def rga_replay_onto_device(batch, device: str = "cuda", tombstones: bool = False):
    """(values, src, offsets) of smx_rga_replay_onto for a crdt.RgaOntoBatch, one list per
    job; src holds column indices of the batch.  With tombstones=True the whole list states
    and a fourth array, the tombstone flags.  Buffers and stream as rga_replay_device."""
    torch = _torch()
    dev = torch.device(device)
    n, nj, n_out = batch.n, batch.n_jobs, batch.n_out
    if nj == 0:
        e = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(1, np.int64))
        return e + (np.zeros(0, np.bool_),) if tombstones else e

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    ins = [up(batch.base_off, np.int64), up(batch.own_off, np.int64), up(batch.job_base, np.int32),
           up(batch.op, np.uint8), up(batch.value, np.int32), up(batch.anchor, np.int32), up(batch.t, np.int64),
           up(batch.author, np.int32), up(batch.opid_hi, np.int64), up(batch.opid_lo, np.int64)]
    vals, src = (torch.empty(max(n_out, 1), dtype=torch.int32, device=dev) for _ in range(2))
    offs = torch.empty(nj + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    tomb = torch.empty(max(n_out, 1), dtype=torch.uint8, device=dev) if tombstones else None
    ws = C.c_size_t(0)
    check(lib().smx_rga_replay_onto_workspace_bytes(nj, n_out, C.byref(ws)))
    wst = torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)
    onto = _abi.SmxRgaOnto(n, batch.n_bases, nj, n_out, *[_ptr(t) for t in ins])
    out = _abi.SmxRgaOut(_ptr(vals), _ptr(src), _ptr(offs), _ptr(counts), _ptr(tomb))
    check(lib().smx_rga_replay_onto(C.byref(onto), C.byref(out), _ptr(wst), ws.value,
                                    torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    k = int(counts.item())
    res = (vals[:k].cpu().numpy().view(np.uint32), src[:k].cpu().numpy(), offs.cpu().numpy())
    return res + (tomb[:k].cpu().numpy().astype(np.bool_),) if tombstones else res


def rga_replay_chain_device(batch, device: str = "cuda", tombstones: bool = False):
    """(values, src, offsets) of smx_rga_replay_chain for a crdt.RgaChainBatch, one list per
    job; src holds column indices of the batch.  With tombstones=True the whole list states
    and a fourth array, the tombstone flags.  Buffers and stream as rga_replay_device."""
    torch = _torch()
    dev = torch.device(device)
    n, nj, nk, n_out = batch.n, batch.n_jobs, batch.n_links, batch.n_out
    if nj == 0:
        e = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(1, np.int64))
        return e + (np.zeros(0, np.bool_),) if tombstones else e

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)

    ins = [up(batch.seg_off, np.int64), up(batch.job_off, np.int64), up(batch.job_seg, np.int32),
           up(batch.op, np.uint8), up(batch.value, np.int32), up(batch.anchor, np.int32), up(batch.t, np.int64),
           up(batch.author, np.int32), up(batch.opid_hi, np.int64), up(batch.opid_lo, np.int64)]
    vals, src = (torch.empty(max(n_out, 1), dtype=torch.int32, device=dev) for _ in range(2))
    offs = torch.empty(nj + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    tomb = torch.empty(max(n_out, 1), dtype=torch.uint8, device=dev) if tombstones else None
    ws = C.c_size_t(0)
    check(lib().smx_rga_replay_chain_workspace_bytes(nj, nk, n_out, C.byref(ws)))
    wst = torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)
    chain = _abi.SmxRgaChain(n, batch.n_segs, nj, nk, n_out, *[_ptr(t) for t in ins])
    out = _abi.SmxRgaOut(_ptr(vals), _ptr(src), _ptr(offs), _ptr(counts), _ptr(tomb))
    check(lib().smx_rga_replay_chain(C.byref(chain), C.byref(out), _ptr(wst), ws.value,
                                     torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    k = int(counts.item())
    res = (vals[:k].cpu().numpy().view(np.uint32), src[:k].cpu().numpy(), offs.cpu().numpy())
    return res + (tomb[:k].cpu().numpy().astype(np.bool_),) if tombstones else res


# These moved to _session.py and _rigs.py and stay importable from here under their old names
# (bench.py, the tests and the tools import them from _lib); resolved on first use, because
# both modules import this one.
_MOVED = {**dict.fromkeys(("ComposeSession", "session", "dropin_session", "compose_soa", "compose_soa_many",
                          "compose_soa_shared", "compose_pairs_soa", "compose_trains_soa", "compose_tree_soa", "tree_levels", "screen_soa", "screen_all_soa",
                          "screen_trains_soa", "screen_tree_soa"),
                          "_session"),
          **dict.fromkeys(("DeviceCompose", "DeviceBatch", "DeviceBatchShared", "DevicePairs", "DeviceTrains", "DeviceTree", "DeviceScreen",
                           "DeviceScreenTrains", "DeviceScreenTree", "DeviceCandidates"), "_rigs")}


def __getattr__(name: str):
    if name not in _MOVED:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    import importlib
    return getattr(importlib.import_module("." + _MOVED[name], __package__), name)
