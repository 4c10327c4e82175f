"""Loader for libsmx.so (the HIP library) and device-buffer plumbing.

PyTorch-ROCm is used only to own device memory and to name the current HIP
stream; every computation happens in libsmx's kernels through the C ABI of
include/smx.h.  There is no CPU fallback: without the library or a GPU these
functions raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

from . import _abi
from .marshal import SoA

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMX_LIB", os.path.join(HERE, "libsmx.so"))
_lib: Optional[C.CDLL] = None


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


class DeviceCompose:
    """Device-resident inputs, outputs and workspace for repeated smx_compose calls.

    The optional arguments reach the corners of the C ABI (include/smx.h):
    b_gap        branch B's columns start b_gap entries after branch A's (smx_ops.b_gap);
                 the gap holds an invalid kind (0xFF) and symbol (0xFFFFFFFF), so a kernel
                 that read it would report invalid input;
    conflict_cap the capacity passed for the conflict pairs (default min(n_a, n_b), which
                 always suffices); CONF_GUARD guard words follow the 2 * conflict_cap
                 words (guard_intact());
    ws_bytes     the workspace size passed (default: what smx_compose_workspace_bytes
                 asks for; the buffer itself always has that size)."""

    CONF_GUARD = 64
    _GUARD_WORD = 0x5A5A5A5A

    def __init__(self, soa: SoA, device: str = "cuda", b_gap: int = 0, conflict_cap: Optional[int] = None,
                 ws_bytes: Optional[int] = None) -> None:
        torch = _torch()
        self.torch = torch
        self.soa = soa
        self.n = soa.n
        dev = torch.device(device)
        self.device = dev
        na = soa.n_a
        if b_gap < 0:
            raise ValueError("b_gap must be >= 0")

        def up(a, dt, fill=0):
            a = np.ascontiguousarray(a)
            if b_gap:
                a = np.concatenate([a[:na], np.full(b_gap, fill, a.dtype), a[na:]])
            return torch.from_numpy(a.view(dt)).to(dev, non_blocking=False)

        self.kind = up(soa.kind, np.uint8, 0xFF)
        self.ts = up(soa.ts, np.int64)      # bit-identical u64 payload
        self.hi = up(soa.oid_hi, np.int64)
        self.lo = up(soa.oid_lo, np.int64)
        self.sym = up(soa.sym, np.int32, 0xFFFFFFFF)
        self.v0 = up(soa.v0, np.int32, -1)
        self.v1 = up(soa.v1, np.int32, -1)
        n = max(self.n, 1)
        self.order = torch.empty(n, dtype=torch.int32, device=dev)
        self.addr = torch.empty(n, dtype=torch.int32, device=dev)
        self.file = torch.empty(n, dtype=torch.int32, device=dev)
        self.ctx = torch.empty(n, dtype=torch.int32, device=dev)
        if conflict_cap is None:
            self.cap = max(min(soa.n_a, soa.n_b), 1)
            self.conf = torch.empty(2 * self.cap, dtype=torch.int32, device=dev)
        else:
            self.cap = conflict_cap
            self.conf = torch.full((2 * max(self.cap, 0) + self.CONF_GUARD,), self._GUARD_WORD,
                                   dtype=torch.int32, device=dev)
        self._guarded = conflict_cap is not None
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        ws = C.c_size_t(0)
        check(lib().smx_compose_workspace_bytes(soa.n_a, soa.n_b, soa.n_sym, C.byref(ws)))
        self.ws_needed = ws.value
        self.ws_bytes = ws.value if ws_bytes is None else ws_bytes
        self.ws = torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)
        self._ops = _abi.SmxOps(soa.n_a, soa.n_b, soa.n_sym, _ptr(self.kind), _ptr(self.ts),
                                _ptr(self.hi), _ptr(self.lo), _ptr(self.sym), _ptr(self.v0),
                                _ptr(self.v1), b_gap)
        self._out = _abi.SmxComposeOut(_ptr(self.order), _ptr(self.addr), _ptr(self.file),
                                       _ptr(self.ctx), _ptr(self.conf), self.cap,
                                       _ptr(self.counts))

    def _args(self, stream):
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        return (C.byref(self._ops), C.byref(self._out), _ptr(self.ws), self.ws_bytes, s.cuda_stream)

    def run(self, stream=None) -> None:
        """One composition on `stream` (default: torch's current stream)."""
        check(lib().smx_compose(*self._args(stream)))

    def run_async(self, stream=None) -> None:
        """Enqueue the host-sync-free part (smx_compose_async; capturable in a graph)."""
        check(lib().smx_compose_async(*self._args(stream)))

    def finish(self, stream=None) -> None:
        """Complete what run_async left (smx_compose_finish: one stream sync)."""
        check(lib().smx_compose_finish(*self._args(stream)))

    @staticmethod
    def last_plan() -> str:
        return _abi.PLAN_NAMES[lib().smx_last_plan()]

    def guard_intact(self) -> bool:
        """The CONF_GUARD words after the conflict pairs' capacity are as they were set
        (a DeviceCompose built with conflict_cap)."""
        if not self._guarded:
            raise ValueError("no guard words: built without conflict_cap")
        self.torch.cuda.synchronize(self.device)
        return bool((self.conf[2 * max(self.cap, 0):] == self._GUARD_WORD).all().item())

    def results(self, truncated: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The composed arrays and the conflict pairs.  More conflicts than conflict_cap
        (include/smx.h: counts[1] > conflict_cap, only the first conflict_cap pairs
        written) raise SmxError -2, or with truncated=True give those first pairs."""
        self.torch.cuda.synchronize(self.device)
        k, nc = (int(x) for x in self.counts.cpu().tolist())
        if k < 0:
            raise SmxError(-1, "invalid input: sym >= n_sym or kind >= 18")
        if nc > self.cap:
            if not truncated:
                raise SmxError(-2, f"{nc} conflicts exceed capacity {self.cap}")
            nc = self.cap
        return (self.order[:k].cpu().numpy(), self.addr[:k].cpu().numpy(),
                self.file[:k].cpu().numpy(), self.ctx[:k].cpu().numpy(),
                self.conf[: 2 * nc].cpu().numpy().reshape(nc, 2))


_COLS = (("kind", np.uint8, None), ("ts", np.uint64, np.int64), ("oid_hi", np.uint64, np.int64),
         ("oid_lo", np.uint64, np.int64), ("sym", np.uint32, np.int32), ("v0", np.int32, None), ("v1", np.int32, None))


class _DeviceMany:
    """What DeviceBatch, DeviceBatchShared and DeviceScreen share: the uploads, the outputs
    filled with one value and followed by CONF_GUARD such words, the workspace, and run /
    raw / results.  A subclass builds its struct (_arg) for its entry point (_call), names
    its output arrays (_OUT) and says where item m's results start (_start)."""

    CONF_GUARD = 64
    _OUT = ("order", "addr", "file", "ctx", "conf", "counts")
    _PER = 2  # counts words per item: (composed ops, conflicts), or the conflicts alone

    def _open(self, device: str) -> None:
        self.torch = _torch()
        self.device = self.torch.device(device)

    def _up(self, a, dt=None):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(dt) if dt is not None else a).to(self.device)

    def _upload_cols(self, sources, n_cols: int = 7) -> None:
        """_in: the first n_cols columns of the sources, one after another, on the device."""
        self._in = [self._up(np.concatenate([np.ascontiguousarray(getattr(s, name)).astype(dt, copy=False)
                                             for s in sources]) if sources else np.zeros(0, dt), view)
                    for name, dt, view in _COLS[:n_cols]]

    def _alloc(self, n: int, caps, n_out: int, fill: Optional[int], query, *sizes) -> None:
        """conf_off from the n items' capacities; every output array of _OUT filled (the
        results n_out entries long); the workspace that `query(*sizes)` asks for."""
        torch, dev = self.torch, self.device
        self.conf_off = np.zeros(n + 1, np.int64)
        np.cumsum(caps, out=self.conf_off[1:])
        f = 0 if fill is None else fill
        for name in self._OUT[:-2]:
            setattr(self, name, torch.full((max(n_out, 1),), f, dtype=torch.int32, device=dev))
        self.conf = torch.full((2 * int(self.conf_off[-1]) + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.counts = torch.full((self._PER * max(n, 1),), f, dtype=torch.int64, device=dev)
        ws = C.c_size_t(0)
        check(query(*sizes, C.byref(ws)))
        self.ws_bytes = ws.value
        self.ws = torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)

    def run(self, stream=None) -> None:
        """Enqueue one call of the entry point on `stream` (default: torch's current stream)."""
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        check(self._call(C.byref(self._arg), self.ws.data_ptr(), self.ws_bytes, s.cuda_stream))

    def raw(self) -> dict:
        """Every output array as the device holds it (after a device sync), on the host."""
        self.torch.cuda.synchronize(self.device)
        return {k: getattr(self, k).cpu().numpy() for k in self._OUT}

    def results(self, raw: Optional[dict] = None):
        """Per item its result arrays (if it has any) and conflict pairs, trimmed to its counts
        and its conflict capacity, or its negative count for an item that failed."""
        r = self.raw() if raw is None else raw
        out = []
        for m in range(len(self.conf_off) - 1):
            k, nc = int(r["counts"][self._PER * m]), int(r["counts"][self._PER * (m + 1) - 1])
            if k < 0:
                out.append(k)
                continue
            c = int(self.conf_off[m])
            nc = min(nc, int(self.conf_off[m + 1]) - c)
            pairs = r["conf"][2 * c: 2 * (c + nc)].reshape(nc, 2)
            if self._PER == 1:
                out.append(pairs)
            else:
                o = self._start(m)
                out.append(tuple(r[x][o: o + k] for x in self._OUT[:-2]) + (pairs,))
        return out


class DeviceBatch(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_compose_batch calls
    on a list of merges (tests, tools/batch_probe.py).  The optional arguments reach the
    corners of the C ABI (include/smx.h smx_batch):
    conflict_caps per-merge capacities of the conflict pairs (default min(n_a, n_b));
    grid_cap      smx_batch.grid_cap;
    n_a           per-merge n_a passed instead of the SoAs' own;
    n_sym         the batch's symbol bound (default: the largest of the merges');
    n_total       smx_batch.n_total passed instead of the columns' real length;
    fill          every output word (results, conflict pairs, counts) starts as this value,
                  and CONF_GUARD such words follow the last merge's conflict region."""

    def __init__(self, soas, device: str = "cuda", conflict_caps=None, grid_cap: int = 0, n_a=None,
                 n_sym: Optional[int] = None, fill: Optional[int] = None, n_total: Optional[int] = None) -> None:
        self._open(device)
        soas = self.soas = list(soas)
        M = self.n_merges = len(soas)
        self.off = np.zeros(M + 1, np.int64)
        np.cumsum([s.n for s in soas], out=self.off[1:])
        tot = self.n_total = int(self.off[-1])
        self.n_a = np.asarray([s.n_a for s in soas] if n_a is None else n_a, np.int64).reshape(M)
        self.n_sym = max([int(s.n_sym) for s in soas] + [1]) if n_sym is None else n_sym
        self._upload_cols(soas)
        self._alloc(M, [min(s.n_a, s.n_b) for s in soas] if conflict_caps is None else conflict_caps, tot, fill,
                    lib().smx_compose_batch_workspace_bytes, M)
        self._idx = [self._up(self.off), self._up(self.n_a), self._up(self.conf_off)]
        self._call = lib().smx_compose_batch
        self._arg = _abi.SmxBatch(M, tot if n_total is None else n_total, self.n_sym, self._idx[0].data_ptr(),
                                  self._idx[1].data_ptr(), *[t.data_ptr() for t in self._in], self.order.data_ptr(),
                                  self.addr.data_ptr(), self.file.data_ptr(), self.ctx.data_ptr(), self.conf.data_ptr(),
                                  self._idx[2].data_ptr(), self.counts.data_ptr(), grid_cap)

    def _start(self, m: int) -> int:
        return int(self.off[m])


class DeviceBatchShared(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_compose_batch_shared
    calls on a SharedSoA (tests, tools/shared_probe.py).  The optional arguments reach the
    corners of the C ABI (include/smx.h smx_batch_shared):
    shared_is_b   smx_batch_shared.shared_is_b;
    conflict_caps per-merge capacities of the conflict pairs (default min(n_shared, len_m));
    grid_cap      smx_batch_shared.grid_cap;
    off           the offsets passed instead of the SharedSoA's own;
    n_sym         the symbol bound passed instead of the SharedSoA's;
    n_total       smx_batch_shared.n_total passed instead of the columns' real length;
    fill          every output word (results, conflict pairs, counts) starts as this value,
                  and CONF_GUARD such words follow the last merge's conflict region."""

    def __init__(self, ssoa, device: str = "cuda", shared_is_b: bool = False, conflict_caps=None, grid_cap: int = 0,
                 off=None, n_sym: Optional[int] = None, fill: Optional[int] = None,
                 n_total: Optional[int] = None) -> None:
        self._open(device)
        self.ssoa = ssoa
        M = self.n_merges = ssoa.n_merges
        S = self.n_shared = int(ssoa.n_shared)
        self.off = np.asarray(ssoa.off if off is None else off, np.int64).reshape(M + 1)
        tot = self.n_total = int(ssoa.n_total)
        lens = np.diff(np.asarray(ssoa.off, np.int64))
        self.n_sym = int(ssoa.n_sym) if n_sym is None else n_sym
        self.n_out = tot - S + M * S
        self._upload_cols([ssoa])
        self._alloc(M, np.minimum(lens, S) if conflict_caps is None else conflict_caps, self.n_out, fill,
                    lib().smx_compose_batch_shared_workspace_bytes, M)
        self._idx = [self._up(self.off), self._up(self.conf_off)]
        self._call = lib().smx_compose_batch_shared
        self._arg = _abi.SmxBatchShared(M, tot if n_total is None else n_total, self.n_sym, S, self._idx[0].data_ptr(),
                                        *[t.data_ptr() for t in self._in], self.order.data_ptr(), self.addr.data_ptr(),
                                        self.file.data_ptr(), self.ctx.data_ptr(), self.conf.data_ptr(),
                                        self._idx[1].data_ptr(), self.counts.data_ptr(), grid_cap, int(shared_is_b))

    def slot(self, m: int) -> int:
        """r(m): where merge m's results start in order / addr / file / ctx."""
        return int(self.off[m]) + (m - 1) * self.n_shared

    _start = slot


def _rename_counts(kind, log_off) -> np.ndarray:
    """Renames per log (i64 [n_logs]) of a LogsSoA's kind column."""
    csum = np.concatenate([[0], np.cumsum(np.asarray(kind) == 1, dtype=np.int64)])  # SMX_KIND_RENAME
    off = np.clip(np.asarray(log_off, np.int64), 0, len(csum) - 1)
    return np.maximum(csum[off[1:]] - csum[off[:-1]], 0)


def _over_limit(ren, pairs) -> int:
    """How many of the (i, j) of `pairs` smx_screen sends back (counts -2) and SMX_SCREEN_LARGE
    streams: both logs have renames and together more than SCREEN_MAX_RENAMES."""
    ra, rb = ren[pairs[:, 0]].astype(np.int64), ren[pairs[:, 1]].astype(np.int64)
    return int(((ra > 0) & (rb > 0) & (ra + rb > _abi.SCREEN_MAX_RENAMES)).sum())


class DeviceScreen(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_screen calls on a
    LogsSoA and a list of (i, j) pairs (tests, tools/screen_probe.py).  The optional
    arguments reach the corners of the C ABI (include/smx.h smx_screen):
    conflict_caps per-pair capacities of the conflict pairs (default: min of the two logs'
                  renames, which always suffices); "null": conflicts and conf_off are NULL;
    grid_cap      smx_screen.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    n_total       smx_screen.n_total passed instead of the columns' real length;
    fill          every output word (conflict pairs, counts) starts as this value, and
                  CONF_GUARD such words follow the last pair's conflict region;
    large         smx_screen_ex with SMX_SCREEN_LARGE (no limit on renames, no counts -2) and
                  the workspace it asks for, instead of smx_screen."""

    _OUT = ("conf", "counts")
    _PER = 1

    def __init__(self, lsoa, pairs, device: str = "cuda", conflict_caps=None, grid_cap: int = 0, log_off=None,
                 n_total: Optional[int] = None, fill: Optional[int] = None, large: bool = False) -> None:
        self._open(device)
        self.lsoa = lsoa
        L = self.n_logs = lsoa.n_logs
        self.pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        P = self.n_pairs = len(self.pairs)
        self.log_off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64).reshape(L + 1)
        tot = self.n_total = int(lsoa.n_total)
        self.null_conf = isinstance(conflict_caps, str) and conflict_caps == "null"
        if conflict_caps is None:
            ren = _rename_counts(lsoa.kind, lsoa.log_off)
            ok = ((self.pairs >= 0) & (self.pairs < L)).all(axis=1)
            pa, pb = np.where(ok, self.pairs[:, 0], 0), np.where(ok, self.pairs[:, 1], 0)
            caps = np.where(ok, np.minimum(ren[pa], ren[pb]), 0) if L else np.zeros(P, np.int64)
        else:
            caps = np.zeros(P, np.int64) if self.null_conf else conflict_caps
        self._upload_cols([lsoa], 6)  # (no v1)
        if large:
            self._alloc(P, caps, 0, fill, lib().smx_screen_ex_workspace_bytes, L, tot, P, _abi.SCREEN_LARGE)
            self._call = lambda arg, ws, nbytes, st: lib().smx_screen_ex(arg, ws, nbytes, _abi.SCREEN_LARGE, st)
        else:
            self._alloc(P, caps, 0, fill, lib().smx_screen_workspace_bytes, L, tot, P)
            self._call = lib().smx_screen
        self._idx = [self._up(self.log_off), self._up(self.pairs[:, 0]), self._up(self.pairs[:, 1]),
                     self._up(self.conf_off)]
        self._arg = _abi.SmxScreen(L, tot if n_total is None else n_total, P, self._idx[0].data_ptr(),
                                   *[_ptr(t) for t in self._in], _ptr(self._idx[1]), _ptr(self._idx[2]),
                                   0 if self.null_conf else self.conf.data_ptr(),
                                   0 if self.null_conf else self._idx[3].data_ptr(), self.counts.data_ptr(), grid_cap)


class DeviceCandidates(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_screen_candidates calls
    on a LogsSoA (tests, tools/cand_probe.py).  The optional arguments reach the corners of
    the C ABI (include/smx.h smx_candidates):
    pair_cap      capacity of pair_a / pair_b (default: all n (n - 1) / 2 pairs); 0: both NULL;
    grid_cap      smx_candidates.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    n_total       smx_candidates.n_total passed instead of the columns' real length;
    fill          every output word (pairs, counts, log_info) starts as this value, and
                  CONF_GUARD such words follow pair_cap and the logs' entries;
    with_log_info False: smx_candidates.log_info is NULL."""

    _OUT = ("pair_a", "pair_b", "counts", "log_info")

    def __init__(self, lsoa, device: str = "cuda", pair_cap: Optional[int] = None, grid_cap: int = 0, log_off=None,
                 n_total: Optional[int] = None, fill: Optional[int] = None, with_log_info: bool = True) -> None:
        self._open(device)
        torch, dev = self.torch, self.device
        self.lsoa = lsoa
        L = self.n_logs = lsoa.n_logs
        self.log_off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64).reshape(L + 1)
        tot = self.n_total = int(lsoa.n_total)
        self.pair_cap = L * (L - 1) // 2 if pair_cap is None else pair_cap
        f = 0 if fill is None else fill
        self._in = [self._up(np.ascontiguousarray(getattr(lsoa, name)).astype(dt, copy=False), view)
                    for name, dt, view in (_COLS[0], _COLS[4], _COLS[5])]  # kind, sym, v0
        self.pair_a = torch.full((self.pair_cap + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.pair_b = torch.full((self.pair_cap + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.counts = torch.full((2 + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        self.log_info = torch.full((L + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        ws = C.c_size_t(0)
        check(lib().smx_screen_candidates_workspace_bytes(L, tot, C.byref(ws)))
        self.ws_bytes = ws.value
        self.ws = torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)
        self._idx = [self._up(self.log_off)]
        self._call = lib().smx_screen_candidates
        self._arg = _abi.SmxCandidates(L, tot if n_total is None else n_total, self._idx[0].data_ptr(),
                                       *[_ptr(t) for t in self._in],
                                       self.pair_a.data_ptr() if self.pair_cap else 0,
                                       self.pair_b.data_ptr() if self.pair_cap else 0, self.pair_cap,
                                       self.counts.data_ptr(), self.log_info.data_ptr() if with_log_info else 0, grid_cap)

    def results(self, raw: Optional[dict] = None):
        """(pairs, n_candidates, n_invalid, log_info): the written candidates as an (n, 2)
        array (the first pair_cap of them), the full count, the invalid logs, every log's entry."""
        r = self.raw() if raw is None else raw
        n, bad = int(r["counts"][0]), int(r["counts"][1])
        k = min(n, self.pair_cap)
        return np.stack([r["pair_a"][:k], r["pair_b"][:k]], axis=1), n, bad, r["log_info"][: self.n_logs]


def _al(x: int) -> int:
    return (x + 255) & ~255


def _pack(hin, h0: int, col, at: int, nbytes: int) -> None:
    """`col` (nbytes long) into the pinned staging area `hin` (at address h0) at byte `at`,
    unless it is that very memory: a column marshalled into staging*() is in place already."""
    if not (isinstance(col, np.ndarray) and col.ctypes.data == h0 + at and col.nbytes == nbytes):
        hin[at: at + nbytes] = np.ascontiguousarray(col).view(np.uint8).reshape(-1)


def _sliced(hout, q: int, start: int, k: int, conf_at: int, nc: int):
    """One merge's results in the output staging area `hout`: k entries from entry `start` of
    each of the four arrays (q bytes apart), and nc conflict pairs from byte conf_at."""
    a, b = 4 * start, 4 * (start + k)
    return (hout[a: b].view(np.int32), hout[q + a: q + b].view(np.int32), hout[2 * q + a: 2 * q + b].view(np.int32),
            hout[3 * q + a: 3 * q + b].view(np.int32), hout[conf_at: conf_at + 8 * nc].view(np.int32).reshape(nc, 2))


class ComposeSession:
    """Reusable buffers for a stream of merges of any size (the drop-in's path): one
    pinned host staging area and one device area, grown on demand, never shrunk.  A
    merge is one host-to-device copy of the packed SoA columns, smx_compose, and one
    device-to-host copy of the outputs and counts -- no allocation after warm-up.
    `last` holds the host / device split of the last merge in seconds."""

    _IN = (("kind", 1), ("ts", 8), ("oid_hi", 8), ("oid_lo", 8), ("sym", 4), ("v0", 4), ("v1", 4))
    ASYNC_MAX = 1 << 22  # smx_compose_async + one sync below this many ops (SMX_EARLY_MIN)

    def __init__(self, device: str = "cuda") -> None:
        self.torch = _torch()
        self.device = self.torch.device(device)
        self.cap_n = self.cap_ws = -1
        self.last = {}
        self.busy = False  # results handed out as views are being read (dropin_session)
        # its own stream: repeated merges of one size replay the library's HIP graph
        self.stream = self.torch.cuda.Stream(self.device)

    _DT = {"kind": np.uint8, "ts": np.uint64, "oid_hi": np.uint64, "oid_lo": np.uint64, "sym": np.uint32,
           "v0": np.int32, "v1": np.int32}

    def staging(self, n: int) -> dict:
        """The input columns of an n-op merge as views of the pinned staging area, laid out
        as compose() copies it: a SoA marshalled into them is not packed again."""
        self._ensure(n, 0)
        hin = self.h_in.numpy()
        cols, off = {}, 0
        for name, w in self._IN:
            cols[name] = hin[off: off + n * w].view(self._DT[name])
            off += _al(n * w)
        return cols

    def _ensure(self, n: int, ws_bytes: int) -> None:
        torch = self.torch
        grown = n > self.cap_n or ws_bytes > self.cap_ws
        if n > self.cap_n:
            cap = max(n + n // 4, 1024)
            in_b = sum(_al(cap * w) for _, w in self._IN)
            out_b = 4 * _al(cap * 4) + _al(cap * 4) + 256     # 4 outputs, conflicts (2 * cap/2), counts
            self.h_in = torch.empty(in_b, dtype=torch.uint8, pin_memory=True)
            self.d_in = torch.empty(in_b, dtype=torch.uint8, device=self.device)
            self.h_out = torch.empty(out_b, dtype=torch.uint8, pin_memory=True)
            self.d_out = torch.empty(out_b, dtype=torch.uint8, device=self.device)
            self.cap_n = cap
        if ws_bytes > self.cap_ws:
            self.ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=self.device)
            self.cap_ws = ws_bytes
        if grown:  # new buffers come from the current stream's pool: ready before the session's stream uses them
            torch.cuda.synchronize(self.device)

    def _copy_in(self, st, nbytes: int) -> None:
        _hip_check(_hiprt().hipMemcpyAsync(self.d_in.data_ptr(), self.h_in.data_ptr(), nbytes, 1, st),
                   "hipMemcpyAsync (inputs)")

    def _copy_back(self, st, nbytes: int) -> None:
        """The first nbytes of the outputs to the host, and the stream sync that ends a merge."""
        hip = _hiprt()
        _hip_check(hip.hipMemcpyAsync(self.h_out.data_ptr(), self.d_out.data_ptr(), nbytes, 2, st),
                   "hipMemcpyAsync (outputs)")
        _hip_check(hip.hipStreamSynchronize(st), "hipStreamSynchronize")

    def compose(self, soa: SoA, copy: bool = True):
        """(order, addr, file, ctx, conflict_pairs) of one merge, computed on the GPU.
        copy=False: views of the session's pinned staging area, valid until its next merge
        (the drop-in materialises them at once)."""
        import time
        t0 = time.perf_counter()
        n = soa.n
        if n == 0:
            e = np.zeros(0, np.int32)
            return e, e, e, e, np.zeros((0, 2), np.int32)
        ws = C.c_size_t(0)
        check(lib().smx_compose_workspace_bytes(soa.n_a, soa.n_b, soa.n_sym, C.byref(ws)))
        self._ensure(n, ws.value)
        hin = self.h_in.numpy()
        off, ptrs = 0, {}
        d0 = self.d_in.data_ptr()
        h0 = hin.ctypes.data
        for name, w in self._IN:   # pack the columns into the pinned staging area (laid out for n)
            _pack(hin, h0, getattr(soa, name), off, n * w)
            ptrs[name] = d0 + off
            off += _al(n * w)
        t1 = time.perf_counter()
        st = self.stream.cuda_stream
        self._copy_in(st, off)
        ccap = max(min(soa.n_a, soa.n_b), 1)
        o0 = self.d_out.data_ptr()
        q = _al(n * 4)             # outputs laid out for n: one contiguous copy back
        ops = _abi.SmxOps(soa.n_a, soa.n_b, soa.n_sym, ptrs["kind"], ptrs["ts"], ptrs["oid_hi"],
                          ptrs["oid_lo"], ptrs["sym"], ptrs["v0"], ptrs["v1"])
        cnt_off = 4 * q + _al(8 * ccap)
        out = _abi.SmxComposeOut(o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + 4 * q, ccap, o0 + cnt_off)
        args = (C.byref(ops), C.byref(out), self.ws.data_ptr(), ws.value, st)
        hout = self.h_out.numpy()

        def copy_back():
            self._copy_back(st, cnt_off + 16)
            return (int(x) for x in hout[cnt_off: cnt_off + 16].view(np.int64))
        if n < self.ASYNC_MAX:
            # merges below the early-verdict size: the asynchronous part, the copy back and
            # ONE stream sync; smx_compose_finish only when the counts ask for it (a plan
            # that failed, None-valued moves: counts[0] < -1)
            check(lib().smx_compose_async(*args))
            k, nc = copy_back()
            if k < -1:
                check(lib().smx_compose_finish(*args))
                k, nc = copy_back()
        else:  # (larger: the synchronous call, which waits for the plan's early verdict)
            check(lib().smx_compose(*args))
            k, nc = copy_back()
        t2 = time.perf_counter()
        if k < 0:
            raise SmxError(-1, "invalid input: sym >= n_sym or kind >= 18")
        if nc > ccap:
            raise SmxError(-2, f"{nc} conflicts exceed capacity {ccap}")
        res = _sliced(hout, q, 0, k, 4 * q, nc)
        if copy:
            res = tuple(x.copy() for x in res)
        self.last = {"pack_s": t1 - t0, "device_s": t2 - t1, "unpack_s": time.perf_counter() - t2}
        return res

    # -- the batched calls: one layout, one staged call, one unpack, one fallback ------------

    @staticmethod
    def _layout(n_total: int, segments, q: int, conf_bytes: int, counts_bytes: int) -> dict:
        """Byte offsets in the staging areas.  In: the (name, nbytes) segments one after
        another, each 256-byte aligned.  Out: four result arrays of q bytes each (0: none),
        the conflict pairs (conf_bytes, and 8 more so that the region is never empty) and
        the counts."""
        lay, o = {"n_total": n_total}, 0
        for name, nbytes in segments:
            lay[name] = o
            o += _al(nbytes)
        lay["in_bytes"] = o
        lay["conf"], lay["counts"] = 4 * q, 4 * q + _al(conf_bytes + 8)
        lay["out_bytes"] = lay["counts"] + counts_bytes
        return lay

    def _ensure_batch(self, lay, ws_bytes: int) -> None:
        # (_ensure sizes the areas per op: 37 input bytes and 20 output bytes each at least)
        self._ensure(max(-(-lay["in_bytes"] // 37), -(-lay["out_bytes"] // 20)), ws_bytes)

    def _staged_call(self, query, sizes, lay, cols, index, make_arg, fn):
        """One batched call through the staging areas: the workspace `query(*sizes)` asks
        for, the columns `cols` ((name, column, byte offset, nbytes)) and the index arrays
        `index` ((name, array)) packed at their places in `lay`, one host-to-device copy,
        fn(make_arg(d_in address, d_out address)), one copy back, one stream sync.  Returns
        the times after the pack and after the sync."""
        import time
        ws = C.c_size_t(0)
        check(query(*sizes, C.byref(ws)))
        self._ensure_batch(lay, ws.value)
        hin = self.h_in.numpy()
        h0 = hin.ctypes.data
        for col, at, nbytes in cols:
            _pack(hin, h0, col, at, nbytes)
        for name, arr in index:
            _pack(hin, h0, arr, lay[name], arr.nbytes)
        t1 = time.perf_counter()
        st = self.stream.cuda_stream
        self._copy_in(st, lay["in_bytes"])
        arg = make_arg(self.d_in.data_ptr(), self.d_out.data_ptr())
        check(fn(C.byref(arg), self.ws.data_ptr(), ws.value, st))
        self._copy_back(st, lay["out_bytes"])
        return t1, time.perf_counter()

    def _batch_results(self, lay, conf_off, starts, labels):
        """Per merge of a batch that ran: its results (views of the output staging area,
        from entry starts[m] of the four arrays), or None for a merge the library sent back
        (counts -2).  labels[m] names merge m in an error."""
        hout = self.h_out.numpy()
        counts = hout[lay["counts"]: lay["counts"] + 16 * len(labels)].view(np.int64).tolist()
        q, conf, co, starts = lay["q"], lay["conf"], conf_off.tolist(), starts.tolist()
        res = []
        for m, i in enumerate(labels):
            k, nc = counts[2 * m], counts[2 * m + 1]
            if k == -2:
                res.append(None)
                continue
            if k < 0:
                raise SmxError(-1, f"merge {i}: invalid input: sym >= n_sym or kind >= 18")
            if nc > co[m + 1] - co[m]:
                raise SmxError(-2, f"merge {i}: {nc} conflicts exceed capacity {co[m + 1] - co[m]}")
            res.append(_sliced(hout, q, starts[m], k, conf + 8 * co[m], nc))
        return res

    def _compose_routed(self, res, routed, soas, what: str, keep_last: bool = True) -> None:
        """res[i] = compose(soa) for the items the batched call did not take; an error names
        the item (`what` i).  keep_last: `last` stays the batched call's (the routed items'
        legs are compose()'s own)."""
        last = self.last
        for i, soa in zip(routed, soas):
            try:
                res[i] = self.compose(soa)
            except SmxError as e:
                raise SmxError(e.code, f"{what} {i}: {e}") from None
        if keep_last:
            self.last = last

    # -- batched compose (smx_compose_batch): many small merges, one launch sequence --------

    @staticmethod
    def _batch_layout(ns):
        """Byte offsets of a batch of merges of ns ops in the staging areas: the input
        columns for sum(ns) ops, then off / n_a / conf_off; the four outputs, the conflict
        pairs (at most sum(ns) / 2) and the counts."""
        m, tot = len(ns), int(sum(ns))
        q = _al(tot * 4)
        lay = ComposeSession._layout(tot, [(name, tot * w) for name, w in ComposeSession._IN]
                                     + [("off", (m + 1) * 8), ("n_a", m * 8), ("conf_off", (m + 1) * 8)],
                                     q, 4 * tot, 16 * m)
        lay["q"] = q
        return lay

    def staging_many(self, ns):
        """The input columns of a batch of merges of ns ops (each at most BATCH_MAX_OPS) as
        views of the pinned staging area, one dict per merge, laid out as compose_many()
        copies them: SoAs marshalled into them are not packed again."""
        lay = self._batch_layout(ns)
        self._ensure_batch(lay, 0)
        hin = self.h_in.numpy()
        offs = np.concatenate([[0], np.cumsum(ns, dtype=np.int64)]) if len(ns) else np.zeros(1, np.int64)
        return [{name: hin[lay[name] + int(offs[m]) * w: lay[name] + int(offs[m + 1]) * w].view(self._DT[name])
                 for name, w in self._IN} for m in range(len(ns))]

    def compose_many(self, soas, copy: bool = True):
        """[(order, addr, file, ctx, conflict_pairs)] of independent merges, in input order.
        The merges of at most BATCH_MAX_OPS ops are packed at consecutive offsets of the
        staging area and run as one batch: one host-to-device copy, one smx_compose_batch,
        one copy back, one stream sync.  Larger merges (and any the library sends back,
        counts -2) go through compose() afterwards.  An invalid merge raises SmxError naming
        its index.  copy=False: views of the staging area, valid until the session's next
        merge (taken only when no merge is routed through compose())."""
        soas = list(soas)
        small = [i for i, s in enumerate(soas) if s.n <= _abi.BATCH_MAX_OPS]
        routed = [i for i, s in enumerate(soas) if s.n > _abi.BATCH_MAX_OPS]
        res = [None] * len(soas)
        if small:
            M = len(small)
            ns = [soas[i].n for i in small]
            lay = self._batch_layout(ns)
            off = np.zeros(M + 1, np.int64)
            np.cumsum(ns, out=off[1:])
            n_a = np.fromiter((soas[i].n_a for i in small), np.int64, M)
            conf_off = np.zeros(M + 1, np.int64)
            np.cumsum(np.minimum(n_a, off[1:] - off[:-1] - n_a), out=conf_off[1:])  # min(n_a, n_b): never truncates
            n_sym, cols = 1, []
            for m, i in enumerate(small):
                soa, n = soas[i], ns[m]
                n_sym = max(n_sym, int(soa.n_sym))
                if n and int(np.max(soa.sym)) >= soa.n_sym:  # (the batch has one bound for all its merges)
                    raise SmxError(-1, f"merge {i}: invalid input: sym >= n_sym")
                cols += [(getattr(soa, name), lay[name] + int(off[m]) * w, n * w) for name, w in self._IN]
            q = lay["q"]
            self._staged_call(
                lib().smx_compose_batch_workspace_bytes, (M,), lay, cols,
                (("off", off), ("n_a", n_a), ("conf_off", conf_off)),
                lambda d0, o0: _abi.SmxBatch(M, lay["n_total"], n_sym, d0 + lay["off"], d0 + lay["n_a"],
                                             *[d0 + lay[name] for name, _ in self._IN],
                                             o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + lay["conf"],
                                             d0 + lay["conf_off"], o0 + lay["counts"], 0),
                lib().smx_compose_batch)
            for i, r in zip(small, self._batch_results(lay, conf_off, off[:-1], small)):
                res[i] = r
                if r is None:
                    routed.append(i)
            if copy or routed:  # (compose() below reuses the staging area)
                res = [r if r is None else tuple(x.copy() for x in r) for r in res]
        routed.sort()
        self._compose_routed(res, routed, [soas[i] for i in routed], "merge", keep_last=False)
        return res

    # -- batched compose against one shared log (smx_compose_batch_shared) -------------------

    @staticmethod
    def _shared_layout(n_total: int, n_shared: int, m: int):
        """Byte offsets of a shared-log batch in the staging areas: the input columns for
        n_total ops (the shared log once), then off / conf_off; the four outputs of
        n_total - n_shared + m * n_shared entries, the conflict pairs (at most
        n_total - n_shared) and the counts."""
        q = _al((n_total - n_shared + m * n_shared) * 4)
        lay = ComposeSession._layout(n_total, [(name, n_total * w) for name, w in ComposeSession._IN]
                                     + [("off", (m + 1) * 8), ("conf_off", (m + 1) * 8)],
                                     q, 8 * (n_total - n_shared), 16 * m)
        lay["q"] = q
        return lay

    def staging_shared(self, n_total: int, n_shared: int, n_merges: int) -> dict:
        """The input columns of a shared-log batch of n_total ops as views of the pinned
        staging area, laid out as compose_shared() copies them: a SharedSoA marshalled into
        them is not packed again."""
        lay = self._shared_layout(n_total, n_shared, n_merges)
        self._ensure_batch(lay, 0)
        hin = self.h_in.numpy()
        return {name: hin[lay[name]: lay[name] + n_total * w].view(self._DT[name]) for name, w in self._IN}

    def compose_shared(self, ssoa, shared_is_b: bool = False, copy: bool = True):
        """[(order, addr, file, ctx, conflict_pairs)] of the merges (shared, branch m) -- or
        (branch m, shared) with shared_is_b -- of a SharedSoA, in branch order.  The columns,
        the shared log once, are staged as they are: one host-to-device copy, one
        smx_compose_batch_shared, one copy back, one stream sync.  Merges over BATCH_MAX_OPS
        ops (the library sends them back, counts -2) go through compose(ssoa.merge(m))
        afterwards.  Invalid input raises SmxError naming the merge.  copy=False: views of
        the staging area, valid until the session's next merge (taken only when no merge is
        routed through compose())."""
        import time
        t0 = time.perf_counter()
        M, S, tot = ssoa.n_merges, int(ssoa.n_shared), int(ssoa.n_total)
        off = np.ascontiguousarray(ssoa.off, dtype=np.int64)
        lens = off[1:] - off[:-1]
        if M and (int(off[0]) < S or (lens < 0).any() or int(off[-1]) > tot):
            raise SmxError(-1, "invalid input: the branch offsets leave the columns or decrease")
        if M:  # (the batch has one bound for all its symbols; entries before off[0] are no merge's)
            sym = np.asarray(ssoa.sym)
            if S and int(np.max(sym[:S])) >= ssoa.n_sym:
                raise SmxError(-1, "the shared log: invalid input: sym >= n_sym")
            o0, o1 = int(off[0]), int(off[-1])
            if o1 > o0 and int(np.max(sym[o0:o1])) >= ssoa.n_sym:
                at = o0 + int(np.argmax(sym[o0:o1] >= ssoa.n_sym))
                raise SmxError(-1, f"merge {int(np.searchsorted(off, at, 'right')) - 1}: invalid input: sym >= n_sym")
        res = [None] * M
        self.last = {"pack_s": 0.0, "device_s": 0.0, "unpack_s": 0.0, "in_bytes": 0}
        if M and (S + lens <= _abi.BATCH_MAX_OPS).any():
            lay = self._shared_layout(tot, S, M)
            conf_off = np.zeros(M + 1, np.int64)
            np.cumsum(np.minimum(lens, S), out=conf_off[1:])  # min(n_a, n_b): never truncates
            q = lay["q"]
            t1, t2 = self._staged_call(
                lib().smx_compose_batch_shared_workspace_bytes, (M,), lay,
                [(getattr(ssoa, name), lay[name], tot * w) for name, w in self._IN],
                (("off", off), ("conf_off", conf_off)),
                lambda d0, o0: _abi.SmxBatchShared(M, tot, int(ssoa.n_sym), S, d0 + lay["off"],
                                                   *[d0 + lay[name] for name, _ in self._IN],
                                                   o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + lay["conf"],
                                                   d0 + lay["conf_off"], o0 + lay["counts"], 0, int(bool(shared_is_b))),
                lib().smx_compose_batch_shared)
            res = self._batch_results(lay, conf_off, off[:-1] + (np.arange(M) - 1) * S, range(M))
            routed = [m for m in range(M) if res[m] is None]
            if copy or routed:  # (compose() below reuses the staging area)
                res = [r if r is None else tuple(x.copy() for x in r) for r in res]
            self.last = {"pack_s": t1 - t0, "device_s": t2 - t1, "unpack_s": time.perf_counter() - t2,
                         "in_bytes": lay["in_bytes"]}
        else:
            routed = list(range(M))
        if routed:
            # (copies: the columns may be views of the staging area that compose() packs into)
            self._compose_routed(res, routed, [ssoa.merge(m, shared_is_b) for m in routed], "merge")
        return res

    # -- conflict screen (smx_screen): many pairs of logs stored once, conflicts only ---------

    _SCREEN_IN = _IN[:6]  # (no v1)

    @staticmethod
    def _screen_layout(n_total: int, n_logs: int, n_pairs: int, n_conf: int = 0):
        """Byte offsets of a screen in the staging areas: the six input columns for n_total
        ops, then log_off / pair_a / pair_b / conf_off; the conflict pairs and the counts."""
        lay = ComposeSession._layout(n_total, [(name, n_total * w) for name, w in ComposeSession._SCREEN_IN]
                                     + [("log_off", (n_logs + 1) * 8), ("pair_a", n_pairs * 4),
                                        ("pair_b", n_pairs * 4), ("conf_off", (n_pairs + 1) * 8)],
                                     0, 8 * n_conf, 8 * n_pairs)
        lay["col_bytes"] = lay["log_off"]
        return lay

    def staging_logs(self, n_total: int, n_logs: int, n_pairs: int) -> dict:
        """The input columns of a screen of n_total ops as views of the pinned staging area,
        laid out as screen() copies them (plus a v1 column of its own, which the marshaller
        fills and the screen does not read): a LogsSoA marshalled into them is not packed
        again."""
        lay = self._screen_layout(n_total, n_logs, n_pairs)
        self._ensure_batch(lay, 0)
        hin = self.h_in.numpy()
        cols = {name: hin[lay[name]: lay[name] + n_total * w].view(self._DT[name]) for name, w in self._SCREEN_IN}
        cols["v1"] = np.empty(n_total, np.int32)
        return cols

    def screen(self, lsoa, pairs, large: bool = False):
        """The conflict pairs (an (n, 2) int32 array of (A index, B index) into
        log i || log j, as compose()'s fifth result) of every (i, j) of `pairs` over a
        LogsSoA: one host-to-device copy of the six columns (33 bytes per op, each log once),
        one smx_screen, one copy back of the counts and the conflict pairs, one stream sync.
        Pairs whose renames exceed SCREEN_MAX_RENAMES (the library sends them back, counts -2)
        go through compose(lsoa.pair(i, j)) afterwards, keeping only the conflicts.  Invalid
        input raises SmxError naming the pair.  large=True: smx_screen_ex with SMX_SCREEN_LARGE
        screens those pairs too, in the same call -- nothing goes through compose()
        (`last["routed"]` is 0, `last["large"]` the number of pairs over the limit)."""
        import time
        t0 = time.perf_counter()
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        P, L, tot = len(pairs), lsoa.n_logs, int(lsoa.n_total)
        self.last = {"pack_s": 0.0, "device_s": 0.0, "unpack_s": 0.0, "in_bytes": 0, "out_bytes": 0, "routed": 0}
        if large:
            self.last["large"] = 0
        flags = _abi.SCREEN_LARGE if large else 0
        if P == 0:
            return []
        bad = np.flatnonzero(((pairs < 0) | (pairs >= L)).any(axis=1))
        if len(bad):
            raise SmxError(-1, f"pair {int(bad[0])}: a log index outside [0, {L})")
        log_off = np.ascontiguousarray(lsoa.log_off, dtype=np.int64)
        ren = _rename_counts(lsoa.kind, log_off)
        conf_off = np.zeros(P + 1, np.int64)
        np.cumsum(np.minimum(ren[pairs[:, 0]], ren[pairs[:, 1]]), out=conf_off[1:])  # never truncates
        lay = self._screen_layout(tot, L, P, int(conf_off[-1]))
        t1, t2 = self._staged_call(
            lib().smx_screen_ex_workspace_bytes, (L, tot, P, flags), lay,
            [(getattr(lsoa, name), lay[name], tot * w) for name, w in self._SCREEN_IN],
            (("log_off", log_off), ("pair_a", pairs[:, 0]), ("pair_b", pairs[:, 1]), ("conf_off", conf_off)),
            lambda d0, o0: _abi.SmxScreen(L, tot, P, d0 + lay["log_off"],
                                          *[d0 + lay[name] for name, _ in self._SCREEN_IN],
                                          d0 + lay["pair_a"], d0 + lay["pair_b"], o0 + lay["conf"],
                                          d0 + lay["conf_off"], o0 + lay["counts"], 0),
            lambda arg, ws, nbytes, st: lib().smx_screen_ex(arg, ws, nbytes, flags, st))
        hout = self.h_out.numpy()
        counts = hout[lay["counts"]: lay["counts"] + 8 * P].view(np.int64)
        bad = np.flatnonzero((counts < 0) & (counts != -2))
        if len(bad):
            p = int(bad[0])
            raise SmxError(-1, f"pair {p} (logs {int(pairs[p, 0])}, {int(pairs[p, 1])}): invalid input: "
                               "log offsets that decrease or leave the columns, or kind >= 18")
        over = np.flatnonzero(counts > conf_off[1:] - conf_off[:-1])
        if len(over):
            raise SmxError(-2, f"pair {int(over[0])}: {int(counts[over[0]])} conflicts exceed its capacity")
        conf = hout[lay["conf"]: lay["conf"] + 8 * int(conf_off[-1])].view(np.int32).reshape(-1, 2)
        res = [None if counts[p] < 0 else conf[int(conf_off[p]): int(conf_off[p]) + int(counts[p])].copy()
               for p in range(P)]
        routed = [p for p in range(P) if res[p] is None]
        self.last = {"pack_s": t1 - t0, "device_s": t2 - t1, "unpack_s": time.perf_counter() - t2,
                     "in_bytes": lay["in_bytes"], "out_bytes": lay["out_bytes"], "routed": len(routed)}
        if large:
            self.last["large"] = _over_limit(ren, pairs)
        if routed:
            # (copies: the columns may be views of the staging area that compose() packs into)
            self._compose_routed(res, routed, [lsoa.pair(int(pairs[p, 0]), int(pairs[p, 1])) for p in routed], "pair")
            for p in routed:
                res[p] = res[p][4]
        return res

    # -- candidate pairs (smx_screen_candidates) and the screen of all of them ----------------

    _CAND_IN = (_IN[0], _IN[4], _IN[5])  # kind, sym, v0

    @staticmethod
    def _cand_layout(n_total: int, n_logs: int, cap: int, cols):
        """Byte offsets of a candidates call in the staging areas.  In: the columns `cols`
        for n_total ops, then log_off (the six columns lie as _screen_layout has them).  Out:
        the two counts, log_info, then pair_a and pair_b of `cap` entries."""
        lay = ComposeSession._layout(n_total, [(name, n_total * w) for name, w in cols]
                                     + [("log_off", (n_logs + 1) * 8)], 0, 0, 0)
        lay["counts"] = 0
        lay["log_info"] = 256
        lay["pair_a"] = 256 + _al(4 * n_logs)
        lay["pair_b"] = lay["pair_a"] + _al(4 * cap)
        lay["out_bytes"] = lay["pair_b"] + _al(4 * cap)
        return lay

    def _ensure_aux(self, in_bytes: int, out_bytes: int) -> None:
        """A second, small pair of staging areas (screen_all's second call), so that the
        first call's columns and pairs stay where they are on the device."""
        torch = self.torch
        if in_bytes > getattr(self, "cap_aux_in", -1) or out_bytes > getattr(self, "cap_aux_out", -1):
            self.cap_aux_in = max(in_bytes + in_bytes // 4, 4096)
            self.cap_aux_out = max(out_bytes + out_bytes // 4, 4096)
            self.h_aux_in = torch.empty(self.cap_aux_in, dtype=torch.uint8, pin_memory=True)
            self.d_aux_in = torch.empty(self.cap_aux_in, dtype=torch.uint8, device=self.device)
            self.h_aux_out = torch.empty(self.cap_aux_out, dtype=torch.uint8, pin_memory=True)
            self.d_aux_out = torch.empty(self.cap_aux_out, dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)  # (as _ensure: ready before the session's stream uses them)

    def _candidates(self, lsoa, cols, start_cap: Optional[int]):
        """smx_screen_candidates on the columns `cols` of a LogsSoA, staged once: one copy in,
        one call, one copy back, one sync; once more with the exact count when the
        candidates exceed the starting capacity (the columns are copied again only if the
        staging areas had to grow for it).  Returns the (n, 2) pairs (a view of the output
        staging area), every log's rename count and the layout; `last` is set."""
        import time
        t0 = time.perf_counter()
        L, tot = lsoa.n_logs, int(lsoa.n_total)
        if L > _abi.CAND_MAX_LOGS:
            raise SmxError(-1, f"{L} logs exceed the {_abi.CAND_MAX_LOGS} of one candidates call")
        log_off = np.ascontiguousarray(lsoa.log_off, dtype=np.int64)
        full = L * (L - 1) // 2
        cap = max(min(full, max(8 * L, 1024) if start_cap is None else start_cap), 1)
        ws = C.c_size_t(0)
        check(lib().smx_screen_candidates_workspace_bytes(L, tot, C.byref(ws)))
        st = self.stream.cuda_stream
        retries, in_bytes, out_bytes, staged = 0, 0, 0, None
        t1 = t0
        while True:
            lay = self._cand_layout(tot, L, cap, cols)
            self._ensure_batch(lay, ws.value)
            if staged != self.d_in.data_ptr():  # (not yet, or the areas grew)
                hin = self.h_in.numpy()
                h0 = hin.ctypes.data
                for name, w in cols:
                    _pack(hin, h0, getattr(lsoa, name), lay[name], tot * w)
                _pack(hin, h0, log_off, lay["log_off"], log_off.nbytes)
                t1 = time.perf_counter()
                self._copy_in(st, lay["in_bytes"])
                staged = self.d_in.data_ptr()
                in_bytes += lay["in_bytes"]
            d0, o0 = self.d_in.data_ptr(), self.d_out.data_ptr()
            arg = _abi.SmxCandidates(L, tot, d0 + lay["log_off"], d0 + lay["kind"], d0 + lay["sym"], d0 + lay["v0"],
                                     o0 + lay["pair_a"], o0 + lay["pair_b"], cap, o0 + lay["counts"],
                                     o0 + lay["log_info"], 0)
            check(lib().smx_screen_candidates(C.byref(arg), self.ws.data_ptr(), ws.value, st))
            self._copy_back(st, lay["out_bytes"])
            out_bytes += lay["out_bytes"]
            hout = self.h_out.numpy()
            n_cand, n_bad = (int(x) for x in hout[:16].view(np.int64))
            info = hout[lay["log_info"]: lay["log_info"] + 4 * L].view(np.int32)
            if n_bad:
                raise SmxError(-1, f"log {int(np.flatnonzero(info < 0)[0])}: invalid input: log offsets that "
                                   "decrease or leave the columns, or kind >= 18")
            if n_cand <= cap:
                break
            cap, retries = n_cand, retries + 1
        pairs = np.stack([hout[lay["pair_a"]: lay["pair_a"] + 4 * n_cand].view(np.int32),
                          hout[lay["pair_b"]: lay["pair_b"] + 4 * n_cand].view(np.int32)], axis=1)
        t2 = time.perf_counter()
        self.last = {"pack_s": t1 - t0, "device_s": t2 - t1, "unpack_s": 0.0, "in_bytes": in_bytes,
                     "out_bytes": out_bytes, "n_candidates": n_cand, "retries": retries, "routed": 0}
        return pairs, info.copy(), lay

    def candidates(self, lsoa, start_cap: Optional[int] = None) -> np.ndarray:
        """The pairs (i, j), i < j, of a LogsSoA's logs that share a symbol both rename to
        different names, as an (n, 2) int32 array in ascending order -- every other pair has
        no conflicts in either orientation (include/smx.h smx_screen_candidates).  One copy in
        (kind, sym, v0, log_off), one call, one copy back, one sync; the call starts with a
        capacity of 8 pairs per log (start_cap: another one) and runs once more with the
        exact count when there are more: `last["retries"]`.  An invalid log raises SmxError
        naming the first one."""
        if lsoa.n_logs == 0:
            self.last = {"pack_s": 0.0, "device_s": 0.0, "unpack_s": 0.0, "in_bytes": 0, "out_bytes": 0,
                         "n_candidates": 0, "retries": 0, "routed": 0}
            return np.zeros((0, 2), np.int32)
        return self._candidates(lsoa, self._CAND_IN, start_cap)[0]

    def screen_all(self, lsoa, start_cap: Optional[int] = None, large: bool = False):
        """(pairs, [conflict_pairs]): the candidate pairs of a LogsSoA (candidates()) and, for
        each, its conflict pairs as screen() gives them; every pair i < j that is not listed
        has none.  The six screen columns go to the device once: smx_screen_candidates runs
        on them, counts and pairs come back with one sync, the host sizes conf_off from the
        logs' rename counts, and smx_screen runs on the same device columns with its pair
        lists pointing at the candidates' device output -- only conf_off is copied in for it.
        Pairs over SCREEN_MAX_RENAMES renames go through compose() as in screen(); with
        large=True the second call is smx_screen_ex with SMX_SCREEN_LARGE and screens them too
        (`last["routed"]` is 0, `last["large"]` their number)."""
        import time
        flags = _abi.SCREEN_LARGE if large else 0
        if lsoa.n_logs == 0:
            self.candidates(lsoa)
            if large:
                self.last["large"] = 0
            return np.zeros((0, 2), np.int32), []
        pairs, ren, lay = self._candidates(lsoa, self._SCREEN_IN, start_cap)
        pairs = pairs.copy()
        last = self.last
        if large:
            last["large"] = _over_limit(ren, pairs)
        t0 = time.perf_counter()
        P, L, tot = len(pairs), lsoa.n_logs, int(lsoa.n_total)
        if P == 0:
            return pairs, []
        conf_off = np.zeros(P + 1, np.int64)
        np.cumsum(np.minimum(ren[pairs[:, 0]], ren[pairs[:, 1]]), out=conf_off[1:])  # never truncates
        n_conf = int(conf_off[-1])
        ws = C.c_size_t(0)
        check(lib().smx_screen_ex_workspace_bytes(L, tot, P, flags, C.byref(ws)))
        self._ensure(0, ws.value)  # (the workspace alone: the columns and the pairs stay on the device)
        a_counts = _al(8 * n_conf + 8)
        self._ensure_aux(conf_off.nbytes, a_counts + 8 * P)
        self.h_aux_in.numpy()[: conf_off.nbytes] = conf_off.view(np.uint8)
        t1 = time.perf_counter()
        st = self.stream.cuda_stream
        hip = _hiprt()
        _hip_check(hip.hipMemcpyAsync(self.d_aux_in.data_ptr(), self.h_aux_in.data_ptr(), conf_off.nbytes, 1, st),
                   "hipMemcpyAsync (conf_off)")
        d0, o0, x0 = self.d_in.data_ptr(), self.d_out.data_ptr(), self.d_aux_out.data_ptr()
        arg = _abi.SmxScreen(L, tot, P, d0 + lay["log_off"], *[d0 + lay[name] for name, _ in self._SCREEN_IN],
                             o0 + lay["pair_a"], o0 + lay["pair_b"], x0, self.d_aux_in.data_ptr(), x0 + a_counts, 0)
        check(lib().smx_screen_ex(C.byref(arg), self.ws.data_ptr(), ws.value, flags, st))
        _hip_check(hip.hipMemcpyAsync(self.h_aux_out.data_ptr(), x0, a_counts + 8 * P, 2, st),
                   "hipMemcpyAsync (conflicts)")
        _hip_check(hip.hipStreamSynchronize(st), "hipStreamSynchronize")
        t2 = time.perf_counter()
        hout = self.h_aux_out.numpy()
        counts = hout[a_counts: a_counts + 8 * P].view(np.int64)
        bad = np.flatnonzero((counts < 0) & (counts != -2))
        if len(bad):
            p = int(bad[0])
            raise SmxError(-1, f"pair {p} (logs {int(pairs[p, 0])}, {int(pairs[p, 1])}): invalid input")
        over = np.flatnonzero(counts > conf_off[1:] - conf_off[:-1])
        if len(over):
            raise SmxError(-2, f"pair {int(over[0])}: {int(counts[over[0]])} conflicts exceed its capacity")
        conf = hout[: 8 * n_conf].view(np.int32).reshape(-1, 2)
        res = [None if counts[p] < 0 else conf[int(conf_off[p]): int(conf_off[p]) + int(counts[p])].copy()
               for p in range(P)]
        routed = [p for p in range(P) if res[p] is None]
        self.last = {"pack_s": last["pack_s"] + t1 - t0, "device_s": last["device_s"] + t2 - t1,
                     "unpack_s": time.perf_counter() - t2, "in_bytes": last["in_bytes"] + conf_off.nbytes,
                     "out_bytes": last["out_bytes"] + a_counts + 8 * P, "n_candidates": P,
                     "retries": last["retries"], "routed": len(routed)}
        if large:
            self.last["large"] = last["large"]
        if routed:
            # (copies: the columns may be views of the staging area that compose() packs into)
            self._compose_routed(res, routed, [lsoa.pair(int(pairs[p, 0]), int(pairs[p, 1])) for p in routed], "pair")
            for p in routed:
                res[p] = res[p][4]
        return pairs, res


_sessions = {}


def session(device: str = "cuda") -> ComposeSession:
    """The calling thread's ComposeSession on `device`."""
    import threading
    key = (threading.get_ident(), str(device))
    s = _sessions.get(key)
    if s is None:
        s = _sessions[key] = ComposeSession(device)
    return s


class dropin_session:
    """The thread's session for one drop-in merge whose results are read as views of its
    staging area (marshal into it, compose, materialise): marked busy meanwhile, so that a
    merge started from inside that materialise -- a caller's Op class or deepcopy hook
    composing again -- gets buffers of its own instead of overwriting the views."""

    def __init__(self, device: str = "cuda") -> None:
        self.device = device

    def __enter__(self) -> ComposeSession:
        s = session(self.device)
        self.s = s if not s.busy else ComposeSession(self.device)
        self.s.busy = True
        return self.s

    def __exit__(self, *exc) -> None:
        self.s.busy = False


def compose_soa(soa: SoA, device: str = "cuda"):
    """(order, addr, file, ctx, conflict_pairs) of one merge, computed on the GPU
    (through the thread's reusable ComposeSession, or buffers of its own while a drop-in
    merge of this thread holds that session)."""
    s = session(device)
    return (s if not s.busy else ComposeSession(device)).compose(soa)


def compose_soa_many(soas, device: str = "cuda"):
    """[(order, addr, file, ctx, conflict_pairs)] of independent merges in one batch
    (ComposeSession.compose_many on the thread's session, or on buffers of its own while a
    drop-in merge of this thread holds that session)."""
    s = session(device)
    return (s if not s.busy else ComposeSession(device)).compose_many(soas)


def compose_soa_shared(ssoa, shared_is_b: bool = False, device: str = "cuda"):
    """[(order, addr, file, ctx, conflict_pairs)] of a SharedSoA's merges in one batch
    (ComposeSession.compose_shared on the thread's session, or on buffers of its own while a
    drop-in merge of this thread holds that session)."""
    s = session(device)
    return (s if not s.busy else ComposeSession(device)).compose_shared(ssoa, shared_is_b)


def screen_soa(lsoa, pairs, device: str = "cuda", large: bool = False):
    """[conflict_pairs] of the (i, j) of `pairs` over a LogsSoA (ComposeSession.screen on the
    thread's session, or on buffers of its own while a drop-in merge of this thread holds
    that session)."""
    s = session(device)
    return (s if not s.busy else ComposeSession(device)).screen(lsoa, pairs, large=large)


def screen_all_soa(lsoa, device: str = "cuda", large: bool = False):
    """(pairs, [conflict_pairs]) of the candidate pairs i < j of a LogsSoA
    (ComposeSession.screen_all on the thread's session, or on buffers of its own while a
    drop-in merge of this thread holds that session)."""
    s = session(device)
    return (s if not s.busy else ComposeSession(device)).screen_all(lsoa, large=large)


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
    vals = torch.empty(n, dtype=torch.int32, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
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
