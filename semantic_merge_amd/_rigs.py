"""Resident-buffer rigs over libsmx's entry points, for tests, tools and bench.py (no product
path): inputs uploaded once, outputs and workspace allocated once, the call repeated.  The
optional arguments reach the corners of the C ABI that the product's path never passes."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _abi
from ._lib import CAND_COLS, OP_COLS, SCREEN_COLS, SmxError, _ptr, _rename_counts, _torch, check, lib
from .marshal import SoA


def _workspace(torch, dev, query, *sizes):
    """(bytes, buffer): the workspace that `query(*sizes)` asks for, allocated on `dev`."""
    ws = C.c_size_t(0)
    check(query(*sizes, C.byref(ws)))
    return ws.value, torch.empty(max(ws.value, 1), dtype=torch.uint8, device=dev)


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
        torch = self.torch = _torch()
        dev = self.device = torch.device(device)
        self.soa, self.n, na = soa, soa.n, soa.n_a
        if b_gap < 0:
            raise ValueError("b_gap must be >= 0")

        def up(a, dt, fill=0):
            a = np.ascontiguousarray(a)
            if b_gap:
                a = np.concatenate([a[:na], np.full(b_gap, fill, a.dtype), a[na:]])
            return torch.from_numpy(a.view(dt)).to(dev, non_blocking=False)

        gap = {"kind": 0xFF, "sym": 0xFFFFFFFF, "v0": -1, "v1": -1}  # (u64 columns: bit-identical payload)
        cols = [up(getattr(soa, name), view, gap.get(name, 0)) for name, _, view in OP_COLS]
        self.kind, self.ts, self.hi, self.lo, self.sym, self.v0, self.v1 = cols
        outs = [torch.empty(max(self.n, 1), dtype=torch.int32, device=dev) for _ in range(4)]
        self.order, self.addr, self.file, self.ctx = outs
        if conflict_cap is None:
            self.cap = max(min(soa.n_a, soa.n_b), 1)
            self.conf = torch.empty(2 * self.cap, dtype=torch.int32, device=dev)
        else:
            self.cap = conflict_cap
            self.conf = torch.full((2 * max(self.cap, 0) + self.CONF_GUARD,), self._GUARD_WORD,
                                   dtype=torch.int32, device=dev)
        self._guarded = conflict_cap is not None
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.ws_needed, self.ws = _workspace(torch, dev, lib().smx_compose_workspace_bytes,
                                             soa.n_a, soa.n_b, soa.n_sym)
        self.ws_bytes = self.ws_needed if ws_bytes is None else ws_bytes
        self._ops = _abi.SmxOps(soa.n_a, soa.n_b, soa.n_sym, *[_ptr(t) for t in cols], b_gap)
        self._out = _abi.SmxComposeOut(*[_ptr(t) for t in outs], _ptr(self.conf), self.cap, _ptr(self.counts))

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
        return tuple(t[:k].cpu().numpy() for t in (self.order, self.addr, self.file, self.ctx)) \
            + (self.conf[: 2 * nc].cpu().numpy().reshape(nc, 2),)


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

    def _train_index(self, lsoa, trains, log_off, train_off, per_log):
        """What DeviceTrains and DeviceScreenTrains keep of their trains alike: lsoa, n_logs, trains,
        n_trains, train_log, n_steps, train_off, log_off, n_total.  Returns (per step per_log's
        entry of its log, 0 for a log index outside the logs; the default region offsets: those
        summed per train, one train after another)."""
        self.lsoa = lsoa
        L = self.n_logs = lsoa.n_logs
        self.trains = [[int(l) for l in tr] for tr in trains]
        R = self.n_trains = len(self.trains)
        self.train_log = np.asarray([l for tr in self.trains for l in tr], np.int32)
        S = self.n_steps = len(self.train_log)
        own_off = np.concatenate([[0], np.cumsum([len(tr) for tr in self.trains], dtype=np.int64)]).astype(np.int64)
        self.train_off = np.asarray(own_off if train_off is None else train_off, np.int64).reshape(R + 1)
        self.log_off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64).reshape(L + 1)
        self.n_total = int(lsoa.n_total)
        ok = (self.train_log >= 0) & (self.train_log < L)
        per_step = np.where(ok, per_log[np.where(ok, self.train_log, 0)], 0).astype(np.int64) if L \
            else np.zeros(S, np.int64)
        csum = np.concatenate([[0], np.cumsum(per_step, dtype=np.int64)])
        return per_step, np.concatenate([[0], np.cumsum(csum[own_off[1:]] - csum[own_off[:-1]], dtype=np.int64)])

    def _tree_index(self, lsoa, parents, node_log, level_off, log_off, per_log):
        """What DeviceTree and DeviceScreenTree keep of their tree alike: lsoa, n_logs, parents,
        n_nodes, node_log, level_off, n_levels, log_off, n_total.  Returns per node per_log's
        entry of its log, 0 for a log index outside the logs."""
        self.lsoa = lsoa
        L = self.n_logs = lsoa.n_logs
        self.parents = np.asarray(parents, np.int32).reshape(-1)
        N = self.n_nodes = len(self.parents)
        self.node_log = np.asarray(node_log, np.int32).reshape(N)
        self.level_off = np.asarray(level_off, np.int64).reshape(-1)
        self.n_levels = len(self.level_off) - 1
        self.log_off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64).reshape(L + 1)
        self.n_total = int(lsoa.n_total)
        ok = (self.node_log >= 0) & (self.node_log < L)
        return np.where(ok, per_log[np.where(ok, self.node_log, 0)], 0).astype(np.int64) if L else np.zeros(N, np.int64)

    def _upload_cols(self, sources, cols=OP_COLS) -> None:
        """_in: the columns `cols` (rows of OP_COLS) of the sources, one after another, uploaded."""
        self._in = [self._up(np.concatenate([np.ascontiguousarray(getattr(s, name)).astype(dt, copy=False)
                                             for s in sources]) if sources else np.zeros(0, dt), view)
                    for name, dt, view in cols]

    def _workspace(self, query, *sizes) -> None:
        """ws, ws_bytes: the workspace that `query(*sizes)` asks for."""
        self.ws_bytes, self.ws = _workspace(self.torch, self.device, query, *sizes)

    def _alloc(self, n: int, caps, n_out: int, fill: Optional[int]) -> None:
        """conf_off from the n items' capacities; every output array of _OUT filled (the
        results n_out entries long)."""
        torch, dev = self.torch, self.device
        self.conf_off = np.zeros(n + 1, np.int64)
        np.cumsum(caps, out=self.conf_off[1:])
        f = 0 if fill is None else fill
        for name in self._OUT[:-2]:
            setattr(self, name, torch.full((max(n_out, 1),), f, dtype=torch.int32, device=dev))
        self.conf = torch.full((2 * int(self.conf_off[-1]) + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.counts = torch.full((self._PER * max(n, 1),), f, dtype=torch.int64, device=dev)

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
                  and CONF_GUARD such words follow the last merge's conflict region;
    flags         smx_compose_batch_ex's flags (_abi.BATCH_LARGE: no limit on a merge's ops, no
                  counts -2) and the workspace it asks for with them."""

    def __init__(self, soas, device: str = "cuda", conflict_caps=None, grid_cap: int = 0, n_a=None,
                 n_sym: Optional[int] = None, fill: Optional[int] = None, n_total: Optional[int] = None,
                 flags: int = 0) -> None:
        self._open(device)
        soas = self.soas = list(soas)
        M = self.n_merges = len(soas)
        self.off = np.zeros(M + 1, np.int64)
        np.cumsum([s.n for s in soas], out=self.off[1:])
        tot = self.n_total = int(self.off[-1])
        self.n_a = np.asarray([s.n_a for s in soas] if n_a is None else n_a, np.int64).reshape(M)
        self.n_sym = max([int(s.n_sym) for s in soas] + [1]) if n_sym is None else n_sym
        self._upload_cols(soas)
        self._alloc(M, [min(s.n_a, s.n_b) for s in soas] if conflict_caps is None else conflict_caps, tot, fill)
        self.flags = flags
        self._workspace(lib().smx_compose_batch_ex_workspace_bytes, M, tot, flags)
        self._idx = [self._up(self.off), self._up(self.n_a), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_compose_batch_ex(arg, ws, nbytes, self.flags, st)
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
                  and CONF_GUARD such words follow the last merge's conflict region;
    flags         smx_compose_batch_shared_ex's flags (_abi.BATCH_LARGE) and the workspace it
                  asks for with them."""

    def __init__(self, ssoa, device: str = "cuda", shared_is_b: bool = False, conflict_caps=None, grid_cap: int = 0,
                 off=None, n_sym: Optional[int] = None, fill: Optional[int] = None,
                 n_total: Optional[int] = None, flags: int = 0) -> None:
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
        self._alloc(M, np.minimum(lens, S) if conflict_caps is None else conflict_caps, self.n_out, fill)
        self.flags = flags
        self._workspace(lib().smx_compose_batch_shared_ex_workspace_bytes, M, tot, S, flags)
        self._idx = [self._up(self.off), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_compose_batch_shared_ex(arg, ws, nbytes, self.flags, st)
        self._arg = _abi.SmxBatchShared(M, tot if n_total is None else n_total, self.n_sym, S, self._idx[0].data_ptr(),
                                        *[t.data_ptr() for t in self._in], self.order.data_ptr(), self.addr.data_ptr(),
                                        self.file.data_ptr(), self.ctx.data_ptr(), self.conf.data_ptr(),
                                        self._idx[1].data_ptr(), self.counts.data_ptr(), grid_cap, int(shared_is_b))

    def slot(self, m: int) -> int:
        """r(m): where merge m's results start in order / addr / file / ctx."""
        return int(self.off[m]) + (m - 1) * self.n_shared

    _start = slot


class DevicePairs(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_compose_pairs calls on a
    LogsSoA and a list of (i, j) pairs (tests, tools/pairs_probe.py).  The optional arguments
    reach the corners of the C ABI (include/smx.h smx_pairs):
    conflict_caps per-pair capacities of the conflict pairs (default min(len_a, len_b));
    grid_cap      smx_pairs.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    res_off       the result offsets passed (default: len_a + len_b entries per pair, one after
                  another; a pair with an index outside the logs gets none);
    n_sym         the symbol bound passed instead of the LogsSoA's;
    n_total       smx_pairs.n_total passed instead of the columns' real length;
    n_out         smx_pairs.n_out passed instead of the result arrays' real length, res_off[-1];
    fill          every output word (results, conflict pairs, counts) starts as this value,
                  and CONF_GUARD such words follow the last pair's regions;
    flags         smx_compose_pairs' flags (_abi.BATCH_LARGE: no limit on a pair's ops, no
                  counts -2) and the workspace it asks for with them."""

    def __init__(self, lsoa, pairs, device: str = "cuda", conflict_caps=None, grid_cap: int = 0, log_off=None,
                 res_off=None, n_sym: Optional[int] = None, n_total: Optional[int] = None,
                 n_out: Optional[int] = None, fill: Optional[int] = None, flags: int = 0) -> None:
        self._open(device)
        self.lsoa = lsoa
        L = self.n_logs = lsoa.n_logs
        self.pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        P = self.n_pairs = len(self.pairs)
        self.log_off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64).reshape(L + 1)
        tot = self.n_total = int(lsoa.n_total)
        lens = np.diff(np.asarray(lsoa.log_off, np.int64))
        ok = ((self.pairs >= 0) & (self.pairs < L)).all(axis=1)
        pa, pb = np.where(ok, self.pairs[:, 0], 0), np.where(ok, self.pairs[:, 1], 0)
        self.len_a = np.where(ok, lens[pa], 0) if L else np.zeros(P, np.int64)
        self.len_b = np.where(ok, lens[pb], 0) if L else np.zeros(P, np.int64)
        if res_off is None:
            res_off = np.concatenate([[0], np.cumsum(self.len_a + self.len_b, dtype=np.int64)])
        self.res_off = np.asarray(res_off, np.int64).reshape(P + 1)
        self.n_out = max(int(self.res_off.max()), 0) if P else 0
        self.n_sym = int(lsoa.n_sym) if n_sym is None else n_sym
        self._upload_cols([lsoa])
        self._alloc(P, np.minimum(self.len_a, self.len_b) if conflict_caps is None else conflict_caps,
                    self.n_out + self.CONF_GUARD, fill)
        self.flags = flags
        self._workspace(lib().smx_compose_pairs_workspace_bytes, L, P, self.n_out, flags)
        self._idx = [self._up(self.log_off), self._up(self.pairs[:, 0]), self._up(self.pairs[:, 1]),
                     self._up(self.res_off), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_compose_pairs(arg, ws, nbytes, self.flags, st)
        self._arg = _abi.SmxPairs(L, tot if n_total is None else n_total, P, self.n_sym,
                                  self.n_out if n_out is None else n_out, self._idx[0].data_ptr(),
                                  *[t.data_ptr() for t in self._in], self._idx[1].data_ptr(), self._idx[2].data_ptr(),
                                  self._idx[3].data_ptr(), self.order.data_ptr(), self.addr.data_ptr(),
                                  self.file.data_ptr(), self.ctx.data_ptr(), self.conf.data_ptr(),
                                  self._idx[4].data_ptr(), self.counts.data_ptr(), grid_cap)

    def _start(self, m: int) -> int:
        return int(self.res_off[m])


class DeviceTrains(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_compose_train calls on a
    LogsSoA and a list of trains, each a list of log indices (tests, tools/train_probe.py).  The
    optional arguments reach the corners of the C ABI (include/smx.h smx_train):
    conflict_caps per-step capacities in conflict records (default: the step's log's length,
                  which always suffices);
    grid_cap      smx_train.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    train_off     the offsets into the steps passed instead of the trains' own;
    res_off       the result offsets passed (default: the sum of its logs' lengths per train, one
                  after another; a log index outside the logs counts as empty);
    n_sym, n_total, n_steps, n_out  passed instead of the real ones;
    v1_alt, empty_str  smx_train's two (default: none, SMX_NONE);
    fill          every output word (results, conflict records, counts, step counts) starts as
                  this value, and CONF_GUARD such words follow the last regions."""

    _OUT = ("src", "addr", "file", "ctx", "conf", "counts", "step_counts")

    def __init__(self, lsoa, trains, device: str = "cuda", conflict_caps=None, grid_cap: int = 0, log_off=None,
                 train_off=None, res_off=None, n_sym: Optional[int] = None, n_total: Optional[int] = None,
                 n_steps: Optional[int] = None, n_out: Optional[int] = None, fill: Optional[int] = None,
                 v1_alt=None, empty_str: int = -1) -> None:
        self._open(device)
        torch, dev = self.torch, self.device
        self._alt = None if v1_alt is None else self._up(np.asarray(v1_alt, np.int32))
        self.step_len, own_res = self._train_index(lsoa, trains, log_off, train_off,
                                                   np.diff(np.asarray(lsoa.log_off, np.int64)))
        L, R, S, tot = self.n_logs, self.n_trains, self.n_steps, self.n_total
        self.res_off = np.asarray(own_res if res_off is None else res_off, np.int64).reshape(R + 1)
        self.n_out = max(int(self.res_off.max()), 0) if R else 0
        self.n_sym = int(lsoa.n_sym) if n_sym is None else n_sym
        self._upload_cols([lsoa])
        self.conf_off = np.zeros(S + 1, np.int64)
        np.cumsum(self.step_len if conflict_caps is None else conflict_caps, out=self.conf_off[1:])
        f = 0 if fill is None else fill
        for name in self._OUT[:4]:
            setattr(self, name, torch.full((self.n_out + self.CONF_GUARD,), f, dtype=torch.int32, device=dev))
        self.conf = torch.full((4 * int(self.conf_off[-1]) + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.counts = torch.full((2 * R + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        self.step_counts = torch.full((2 * S + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        self._workspace(lib().smx_compose_train_workspace_bytes, L, R, S, self.n_out, 0)
        self._idx = [self._up(self.log_off), self._up(self.train_off), self._up(self.train_log),
                     self._up(self.res_off), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_compose_train(arg, ws, nbytes, 0, st)
        self._arg = _abi.SmxTrain(L, tot if n_total is None else n_total, R, S if n_steps is None else n_steps,
                                  self.n_sym, self.n_out if n_out is None else n_out, self._idx[0].data_ptr(),
                                  *[t.data_ptr() for t in self._in], _ptr(self._alt), self._idx[1].data_ptr(),
                                  self._idx[2].data_ptr(), self._idx[3].data_ptr(), self.src.data_ptr(),
                                  self.addr.data_ptr(), self.file.data_ptr(), self.ctx.data_ptr(),
                                  self.conf.data_ptr(), self._idx[4].data_ptr(), self.counts.data_ptr(),
                                  self.step_counts.data_ptr(), grid_cap, empty_str)

    def results(self, raw: Optional[dict] = None):
        """Per train -1 for one that failed, else (src, addr, file, ctx, landed, steps): the final
        accumulator trimmed to its count, the steps that landed, and per step (accumulator length
        after it, outcome, its conflict records as an (n, 4) array trimmed to its capacity)."""
        r = self.raw() if raw is None else raw
        out = []
        for t, tr in enumerate(self.trains):
            k, landed = int(r["counts"][2 * t]), int(r["counts"][2 * t + 1])
            if k < 0:
                out.append(k)
                continue
            steps = []
            for g in range(int(self.train_off[t]), int(self.train_off[t + 1])):
                acc, oc = int(r["step_counts"][2 * g]), int(r["step_counts"][2 * g + 1])
                c = int(self.conf_off[g])
                nc = min(max(oc, 0), int(self.conf_off[g + 1]) - c)
                steps.append((acc, oc, r["conf"][4 * c: 4 * (c + nc)].reshape(nc, 4)))
            o = int(self.res_off[t])
            out.append(tuple(r[x][o: o + k] for x in self._OUT[:4]) + (landed, steps))
        return out


class DeviceTree(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_compose_tree calls on a
    LogsSoA and a tree in level order (tests, tools/tree_probe.py): `parents` and `node_log` per
    node, `level_off` the levels' bounds (_session.tree_levels gives all three for a tree in any
    order).  The optional arguments reach the corners of the C ABI (include/smx.h smx_tree):
    conflict_caps per-node capacities in conflict records (default: the node's log's length,
                  which always suffices);
    grid_cap      smx_tree.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    res_off       the result offsets passed (default: min(2048, the sum of the logs' lengths on
                  its root path) per node, one after another; a log index outside the logs
                  counts as empty);
    n_sym, n_total, n_levels, n_out  passed instead of the real ones;
    v1_alt, empty_str  smx_tree's two (default: none, SMX_NONE);
    fill          every output word (results, conflict records, node counts, node_acc) starts as
                  this value, and CONF_GUARD such words follow the last regions;
    share         another DeviceTree or DeviceTrains with a workspace at least as large: its
                  workspace is used instead of a new one."""

    _OUT = ("src", "addr", "file", "ctx", "conf", "node_counts", "node_acc")

    def __init__(self, lsoa, parents, node_log, level_off, device: str = "cuda", conflict_caps=None,
                 grid_cap: int = 0, log_off=None, res_off=None, n_sym: Optional[int] = None,
                 n_total: Optional[int] = None, n_levels: Optional[int] = None, n_out: Optional[int] = None,
                 fill: Optional[int] = None, v1_alt=None, empty_str: int = -1, share=None) -> None:
        self._open(device)
        torch, dev = self.torch, self.device
        self._alt = None if v1_alt is None else self._up(np.asarray(v1_alt, np.int32))
        self.node_len = self._tree_index(lsoa, parents, node_log, level_off, log_off,
                                         np.diff(np.asarray(lsoa.log_off, np.int64)))
        L, N, D, tot = self.n_logs, self.n_nodes, self.n_levels, self.n_total
        if res_off is None:
            psum = np.zeros(N, np.int64)
            for n in range(N):  # (level order: a parent lies before its children)
                p = int(self.parents[n])
                psum[n] = (psum[p] if 0 <= p < n else 0) + self.node_len[n]
            res_off = np.concatenate([[0], np.cumsum(np.minimum(psum, _abi.BATCH_MAX_OPS), dtype=np.int64)])
        self.res_off = np.asarray(res_off, np.int64).reshape(N + 1)
        self.n_out = max(int(self.res_off.max()), 0) if N else 0
        self.n_sym = int(lsoa.n_sym) if n_sym is None else n_sym
        self._upload_cols([lsoa])
        self.conf_off = np.zeros(N + 1, np.int64)
        np.cumsum(self.node_len if conflict_caps is None else conflict_caps, out=self.conf_off[1:])
        f = 0 if fill is None else fill
        for name in self._OUT[:4]:
            setattr(self, name, torch.full((self.n_out + self.CONF_GUARD,), f, dtype=torch.int32, device=dev))
        self.conf = torch.full((4 * max(int(self.conf_off.max()), 0) + self.CONF_GUARD,), f, dtype=torch.int32,
                               device=dev)
        self.node_counts = torch.full((2 * N + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        self.node_acc = torch.full((N + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        if share is None:
            self._workspace(lib().smx_compose_tree_workspace_bytes, L, N, D, self.n_out, 0)
        else:
            ws = C.c_size_t(0)
            check(lib().smx_compose_tree_workspace_bytes(L, N, D, self.n_out, 0, C.byref(ws)))
            if share.ws_bytes < ws.value:
                raise ValueError("share: a rig whose workspace is at least as large")
            self.ws_bytes, self.ws = share.ws_bytes, share.ws
        self._idx = [self._up(self.log_off), self._up(self.level_off), self._up(self.parents),
                     self._up(self.node_log), self._up(self.res_off), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_compose_tree(arg, ws, nbytes, 0, st)
        self._arg = _abi.SmxTree(L, tot if n_total is None else n_total, N, D if n_levels is None else n_levels,
                                 self.n_sym, self.n_out if n_out is None else n_out, self._idx[0].data_ptr(),
                                 *[t.data_ptr() for t in self._in], _ptr(self._alt), self._idx[1].data_ptr(),
                                 self._idx[2].data_ptr(), self._idx[3].data_ptr(), self._idx[4].data_ptr(),
                                 self.src.data_ptr(), self.addr.data_ptr(), self.file.data_ptr(),
                                 self.ctx.data_ptr(), self.conf.data_ptr(), self._idx[5].data_ptr(),
                                 self.node_counts.data_ptr(), self.node_acc.data_ptr(), grid_cap, empty_str)

    def results(self, raw: Optional[dict] = None):
        """Per node -1 for one that failed structurally, else (src, addr, file, ctx, acc, length,
        outcome, records): the accumulator after the node, read through node_acc (`acc`: that
        node, or -1 for an empty accumulator) and trimmed to the node's count, the node's
        outcome, and its conflict records as an (n, 4) array trimmed to its capacity."""
        r = self.raw() if raw is None else raw
        out = []
        for n in range(self.n_nodes):
            k, oc, acc = int(r["node_counts"][2 * n]), int(r["node_counts"][2 * n + 1]), int(r["node_acc"][n])
            if k < 0:
                out.append(-1)
                continue
            c = int(self.conf_off[n])
            nc = min(max(oc, 0), max(int(self.conf_off[n + 1]) - c, 0)) if c >= 0 else 0
            o = int(self.res_off[acc]) if acc >= 0 else 0
            out.append(tuple(r[x][o: o + k] for x in self._OUT[:4]) + (acc, k, oc, r["conf"][4 * c: 4 * (c + nc)].reshape(nc, 4)))
        return out


class DeviceTrainLoop(_DeviceMany):
    """One train of any size on device-resident columns, as the host loop of smx_train_stage,
    smx_compose and smx_train_land (_session.run_train_loop; tests, tools/train_loop_probe.py).
    v1_alt, empty_str  smx_train_step's two (default: none, SMX_NONE);
    record_caps   per-step capacities in conflict records (default: the step's log's length,
                  which always suffices);
    fill          every output word (the staged columns, the two state buffers, the records,
                  status) starts as this value, and CONF_GUARD such words follow every array;
    acc           a hand-made accumulator to start from: (src, addr, file, ctx) arrays;
    log_off, n_sym, n_total  passed instead of the LogsSoA's own;
    share         another DeviceTrainLoop over the same LogsSoA, at least as large: its device
                  buffers and workspace are used instead of new ones.
    run() keeps, per step that ran on the device, its status triple in `steps`."""

    _OUT = ("st_kind", "st_ts", "st_oid_hi", "st_oid_lo", "st_sym", "st_v0", "st_v1", "state0", "state1", "records",
            "status")

    def __init__(self, lsoa, train, v1_alt=None, empty_str: int = -1, record_caps=None, fill: Optional[int] = None,
                 device: str = "cuda", acc=None, log_off=None, n_sym: Optional[int] = None,
                 n_total: Optional[int] = None, share=None) -> None:
        self._open(device)
        torch, dev = self.torch, self.device
        self.lsoa = lsoa
        self.train = [int(l) for l in train]
        L, S = lsoa.n_logs, len(self.train)
        self.log_off = np.asarray(lsoa.log_off if log_off is None else log_off, np.int64).reshape(L + 1)
        tot = int(lsoa.n_total)
        self.n_total = tot if n_total is None else n_total
        self.n_sym = int(lsoa.n_sym) if n_sym is None else n_sym
        lens = np.diff(np.asarray(lsoa.log_off, np.int64))
        self.step_len = np.asarray([int(lens[l]) if 0 <= l < L else 0 for l in self.train], np.int64)
        self._acc = None if acc is None else [np.ascontiguousarray(a, dtype=np.int32) for a in acc]
        cap = self.cap = int(self.step_len.sum()) + (len(self._acc[0]) if acc is not None else 0)
        self.rec_off = np.zeros(S + 1, np.int64)
        np.cumsum(self.step_len if record_caps is None else record_caps, out=self.rec_off[1:])
        f = 0 if fill is None else fill
        G = self.CONF_GUARD

        def full(n, dt):
            return torch.full((n + G,), f & 0xFF if dt == torch.uint8 else f, dtype=dt, device=dev)

        if share is not None:
            if share.lsoa is not lsoa or cap > share.cap or self.rec_off[-1] > share.rec_off[-1]:
                raise ValueError("share: a DeviceTrainLoop over the same LogsSoA, at least as large")
            cap = self.cap = share.cap
            for name in self._OUT + ("_in", "_alt", "order", "addr", "file", "ctx", "conf", "counts", "_status_host",
                                     "_wsbox"):
                setattr(self, name, getattr(share, name))
        else:
            self._upload_cols([lsoa])
            self._alt = None if v1_alt is None else self._up(np.asarray(v1_alt, np.int32))
            for (name, _, view) in OP_COLS:
                setattr(self, "st_" + name, full(cap, getattr(torch, view.name)))
            self.state0, self.state1 = full(4 * (cap + G), torch.int32), full(4 * (cap + G), torch.int32)
            self.records = full(4 * int(self.rec_off[-1]), torch.int32)
            self.status = full(3, torch.int64)
            # (smx_compose's own outputs: it alone writes them)
            self.order, self.addr, self.file, self.ctx = (torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
                                                          for _ in range(4))
            self.conf = torch.zeros(max(cap, 2), dtype=torch.int32, device=dev)  # (2 * min(n_acc, log_n) words at most)
            self.counts = torch.zeros(2, dtype=torch.int64, device=dev)
            self._status_host = torch.zeros(3, dtype=torch.int64, pin_memory=True)
            self._wsbox = {"bytes": 0, "ws": None}  # (the workspace, grown on demand)
        self._base = _abi.SmxTrainStep(
            n_total=self.n_total, n_sym=self.n_sym, **{name: _ptr(t) for (name, _, _), t in zip(OP_COLS, self._in)},
            v1_alt=_ptr(self._alt), **{"st_" + name: getattr(self, "st_" + name).data_ptr() for name, _, _ in OP_COLS},
            order=self.order.data_ptr(), addr=self.addr.data_ptr(), file=self.file.data_ptr(), ctx=self.ctx.data_ptr(),
            conflicts=self.conf.data_ptr(), counts=self.counts.data_ptr(), records=self.records.data_ptr(),
            status=self.status.data_ptr(), empty_str=empty_str)
        self.steps, self.cur, self.n_acc, self.landed = [], 0, 0, 0

    def _state(self, i: int):
        """The four arrays of state buffer i, cap + CONF_GUARD words apart."""
        t, q = (self.state0, self.state1)[i], self.cap + self.CONF_GUARD
        return tuple(t.data_ptr() + 4 * q * f for f in range(4))

    def _ws(self, nbytes: int) -> int:
        box = self._wsbox
        if box["ws"] is None or nbytes > box["bytes"]:
            self.torch.cuda.synchronize(self.device)
            box["bytes"], box["ws"] = nbytes, self.torch.empty(max(nbytes, 1), dtype=self.torch.uint8, device=self.device)
            self.torch.cuda.synchronize(self.device)
        return box["ws"].data_ptr()

    def run(self, stream=None, hook=None) -> None:
        """The train's steps one after another on `stream` (default: torch's current stream),
        from an empty accumulator (or `acc`) in state buffer 0."""
        from ._session import run_train_loop
        s = stream if stream is not None else self.torch.cuda.current_stream(self.device)
        n0 = 0
        if self._acc is not None:
            n0, q = len(self._acc[0]), self.cap + self.CONF_GUARD
            for f, a in enumerate(self._acc):
                self.state0[f * q: f * q + n0] = self._up(a)
            self.torch.cuda.synchronize(self.device)
        self.cur, self.n_acc, self.landed, self.steps = run_train_loop(
            s.cuda_stream, self._base, (self._state(0), self._state(1)), self.log_off, self.train, self.rec_off,
            self._ws, self._status_host.numpy(), hook, n_acc=n0)

    def results(self, raw: Optional[dict] = None):
        """DeviceTrains' per-train tuple (src, addr, file, ctx, landed, steps): the final
        accumulator, the steps that landed, and per step (accumulator length after it, outcome,
        its conflict records as an (n, 4) array trimmed to its capacity)."""
        r = self.raw() if raw is None else raw
        q = self.cap + self.CONF_GUARD
        fin = r["state%d" % self.cur]
        steps = []
        for g, (acc, oc, _) in enumerate(self.steps):
            c = int(self.rec_off[g])
            nc = min(max(oc, 0), int(self.rec_off[g + 1]) - c)
            steps.append((acc, oc, r["records"][4 * c: 4 * (c + nc)].reshape(nc, 4)))
        return tuple(fin[f * q: f * q + self.n_acc] for f in range(4)) + (self.landed, steps)


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
        self._upload_cols([lsoa], SCREEN_COLS)
        self._alloc(P, caps, 0, fill)
        if large:
            self._workspace(lib().smx_screen_ex_workspace_bytes, L, tot, P, _abi.SCREEN_LARGE)
            self._call = lambda arg, ws, nbytes, st: lib().smx_screen_ex(arg, ws, nbytes, _abi.SCREEN_LARGE, st)
        else:
            self._workspace(lib().smx_screen_workspace_bytes, L, tot, P)
            self._call = lib().smx_screen
        self._idx = [self._up(self.log_off), self._up(self.pairs[:, 0]), self._up(self.pairs[:, 1]),
                     self._up(self.conf_off)]
        self._arg = _abi.SmxScreen(L, tot if n_total is None else n_total, P, self._idx[0].data_ptr(),
                                   *[_ptr(t) for t in self._in], _ptr(self._idx[1]), _ptr(self._idx[2]),
                                   0 if self.null_conf else self.conf.data_ptr(),
                                   0 if self.null_conf else self._idx[3].data_ptr(), self.counts.data_ptr(), grid_cap)


class DeviceScreenTrains(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_screen_train calls on a
    LogsSoA and a list of trains, each a list of log indices (tests, tools/screen_train_probe.py).
    The optional arguments reach the corners of the C ABI (include/smx.h smx_screen_train):
    conf_caps     per-step capacities in conflict records (default: the renames of the step's
                  log, which always suffices); "null": conflicts and conf_off are NULL;
    grid_cap      smx_screen_train.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    train_off     the offsets into the steps passed instead of the trains' own;
    acc_off       the accumulator offsets passed (default: the sum of its logs' rename counts per
                  train, one after another; a log index outside the logs counts as empty);
    n_total, n_steps, n_acc  passed instead of the real ones;
    fill          every output word (conflict records, counts, step counts) starts as this value,
                  and CONF_GUARD such words follow the last regions."""

    _OUT = ("conf", "counts", "step_counts")

    def __init__(self, lsoa, trains, device: str = "cuda", conf_caps=None, grid_cap: int = 0, log_off=None,
                 train_off=None, acc_off=None, n_total: Optional[int] = None, n_steps: Optional[int] = None,
                 n_acc: Optional[int] = None, fill: Optional[int] = None) -> None:
        self._open(device)
        torch, dev = self.torch, self.device
        self.step_ren, own_acc = self._train_index(lsoa, trains, log_off, train_off,
                                                   _rename_counts(lsoa.kind, lsoa.log_off))
        L, R, S, tot = self.n_logs, self.n_trains, self.n_steps, self.n_total
        self.acc_off = np.asarray(own_acc if acc_off is None else acc_off, np.int64).reshape(R + 1)
        self.n_acc = max(int(self.acc_off.max()), 0) if R else 0
        self.null_conf = isinstance(conf_caps, str) and conf_caps == "null"
        self._upload_cols([lsoa], SCREEN_COLS)
        self.conf_off = np.zeros(S + 1, np.int64)
        if not self.null_conf:
            np.cumsum(self.step_ren if conf_caps is None else conf_caps, out=self.conf_off[1:])
        f = 0 if fill is None else fill
        self.conf = torch.full((2 * int(self.conf_off[-1]) + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.counts = torch.full((2 * R + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        self.step_counts = torch.full((2 * S + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        n_acc = self.n_acc if n_acc is None else n_acc
        self._workspace(lib().smx_screen_train_workspace_bytes, L, tot, R, S, max(n_acc, self.n_acc, 0), 0)
        self._idx = [self._up(self.log_off), self._up(self.train_off), self._up(self.train_log),
                     self._up(self.acc_off), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_screen_train(arg, ws, nbytes, 0, st)
        self._arg = _abi.SmxScreenTrain(L, tot if n_total is None else n_total, R, S if n_steps is None else n_steps,
                                        n_acc, self._idx[0].data_ptr(), *[_ptr(t) for t in self._in],
                                        self._idx[1].data_ptr(), _ptr(self._idx[2]), self._idx[3].data_ptr(),
                                        0 if self.null_conf else self.conf.data_ptr(),
                                        0 if self.null_conf else self._idx[4].data_ptr(), self.counts.data_ptr(),
                                        self.step_counts.data_ptr(), grid_cap)

    def results(self, raw: Optional[dict] = None):
        """Per train its failing count (-1), else (n_renames, landed, steps): the renames in the
        final accumulator, the steps that landed, and per step (the accumulator's renames after
        it, outcome, its conflict records as an (n, 2) array trimmed to its capacity)."""
        r = self.raw() if raw is None else raw
        out = []
        for t in range(self.n_trains):
            k, landed = int(r["counts"][2 * t]), int(r["counts"][2 * t + 1])
            if k < 0:
                out.append(k)
                continue
            steps = []
            for g in range(int(self.train_off[t]), int(self.train_off[t + 1])):
                acc, oc = int(r["step_counts"][2 * g]), int(r["step_counts"][2 * g + 1])
                c = int(self.conf_off[g])
                nc = min(max(oc, 0), int(self.conf_off[g + 1]) - c)
                steps.append((acc, oc, r["conf"][2 * c: 2 * (c + nc)].reshape(nc, 2)))
            out.append((k, landed, steps))
        return out


class DeviceScreenTree(_DeviceMany):
    """Device-resident inputs, outputs and workspace for repeated smx_screen_tree calls on a
    LogsSoA and a tree in level order (tests, tools/screen_tree_probe.py): `parents` and `node_log`
    per node, `level_off` the levels' bounds (_session.tree_levels gives all three for a tree in
    any order).  The optional arguments reach the corners of the C ABI (include/smx.h
    smx_screen_tree):
    conf_caps     per-node capacities in conflict records (default: the renames of the node's
                  log, which always suffices); "null": conflicts and conf_off are NULL;
    conf_off      the record offsets passed instead of the capacities' running sum;
    grid_cap      smx_screen_tree.grid_cap;
    log_off       the offsets passed instead of the LogsSoA's own;
    acc_off       the accumulator offsets passed (default: the room rule, _session.tree_room, one
                  region after another; a log index outside the logs counts as empty);
    n_total, n_levels, n_acc  passed instead of the real ones;
    fill          every output word (conflict records, node counts) starts as this value, and
                  CONF_GUARD such words follow the last regions;
    share         another screen rig with a workspace at least as large: its workspace is used
                  instead of a new one."""

    _OUT = ("conf", "node_counts")

    def __init__(self, lsoa, parents, node_log, level_off, device: str = "cuda", conf_caps=None, grid_cap: int = 0,
                 log_off=None, acc_off=None, conf_off=None, n_total: Optional[int] = None,
                 n_levels: Optional[int] = None, n_acc: Optional[int] = None, fill: Optional[int] = None,
                 share=None) -> None:
        from ._session import tree_room
        self._open(device)
        torch, dev = self.torch, self.device
        self.node_ren = self._tree_index(lsoa, parents, node_log, level_off, log_off,
                                         _rename_counts(lsoa.kind, lsoa.log_off))
        L, N, D, tot = self.n_logs, self.n_nodes, self.n_levels, self.n_total
        if acc_off is None:
            acc_off = np.concatenate([[0], np.cumsum(tree_room(self.parents, self.node_ren), dtype=np.int64)])
        self.acc_off = np.asarray(acc_off, np.int64).reshape(N + 1)
        self.n_acc = max(int(self.acc_off.max()), 0) if N else 0
        self.null_conf = isinstance(conf_caps, str) and conf_caps == "null"
        self._upload_cols([lsoa], SCREEN_COLS)
        self.conf_off = np.zeros(N + 1, np.int64)
        if conf_off is not None:
            self.conf_off = np.asarray(conf_off, np.int64).reshape(N + 1)
        elif not self.null_conf:
            np.cumsum(self.node_ren if conf_caps is None else conf_caps, out=self.conf_off[1:])
        f = 0 if fill is None else fill
        self.conf = torch.full((2 * max(int(self.conf_off.max()), 0) + self.CONF_GUARD,), f, dtype=torch.int32,
                               device=dev)
        self.node_counts = torch.full((2 * N + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        n_acc = self.n_acc if n_acc is None else n_acc
        sizes = (L, tot, N, D, max(n_acc, self.n_acc, 0), 0)
        if share is None:
            self._workspace(lib().smx_screen_tree_workspace_bytes, *sizes)
        else:
            ws = C.c_size_t(0)
            check(lib().smx_screen_tree_workspace_bytes(*sizes, C.byref(ws)))
            if share.ws_bytes < ws.value:
                raise ValueError("share: a rig whose workspace is at least as large")
            self.ws_bytes, self.ws = share.ws_bytes, share.ws
        self._idx = [self._up(self.log_off), self._up(self.level_off), self._up(self.parents),
                     self._up(self.node_log), self._up(self.acc_off), self._up(self.conf_off)]
        self._call = lambda arg, ws, nbytes, st: lib().smx_screen_tree(arg, ws, nbytes, 0, st)
        self._arg = _abi.SmxScreenTree(L, tot if n_total is None else n_total, N, D if n_levels is None else n_levels,
                                       n_acc, self._idx[0].data_ptr(), *[_ptr(t) for t in self._in],
                                       self._idx[1].data_ptr(), _ptr(self._idx[2]), _ptr(self._idx[3]),
                                       self._idx[4].data_ptr(), 0 if self.null_conf else self.conf.data_ptr(),
                                       0 if self.null_conf else self._idx[5].data_ptr(),
                                       self.node_counts.data_ptr(), grid_cap)

    def results(self, raw: Optional[dict] = None):
        """Per node -1 for one that failed structurally, else (renames, outcome, records): the
        renames in the accumulator after the node, its outcome, and its conflict records as an
        (n, 2) array trimmed to its capacity."""
        r = self.raw() if raw is None else raw
        out = []
        for n in range(self.n_nodes):
            k, oc = int(r["node_counts"][2 * n]), int(r["node_counts"][2 * n + 1])
            if k < 0:
                out.append(-1)
                continue
            c = int(self.conf_off[n])
            nc = min(max(oc, 0), max(int(self.conf_off[n + 1]) - c, 0)) if c >= 0 else 0
            out.append((k, oc, r["conf"][2 * c: 2 * (c + nc)].reshape(nc, 2)))
        return out


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
        self._upload_cols([lsoa], CAND_COLS)
        self.pair_a = torch.full((self.pair_cap + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.pair_b = torch.full((self.pair_cap + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self.counts = torch.full((2 + self.CONF_GUARD,), f, dtype=torch.int64, device=dev)
        self.log_info = torch.full((L + self.CONF_GUARD,), f, dtype=torch.int32, device=dev)
        self._workspace(lib().smx_screen_candidates_workspace_bytes, L, tot)
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
