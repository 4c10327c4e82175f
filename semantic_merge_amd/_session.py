"""The product's path through libsmx: ComposeSession, the thread's reusable staging areas
that every drop-in call of compose.py goes through, and the *_soa* wrappers over it.  A call
packs its inputs into a pinned host area, copies them in, calls the library on the session's
stream, copies the results back and syncs once (torch only owns memory and stream: _lib.py)."""
from __future__ import annotations

import ctypes as C
import threading
import time
from typing import Optional

import numpy as np

from . import _abi
from ._lib import (CAND_COLS, OP_COLS, SCREEN_COLS, SmxError, _hip_check, _hiprt, _rename_counts, _torch, check,
                   lib)
from .marshal import SoA

_OP_BYTES = sum(dt.itemsize for _, dt, _ in OP_COLS)  # input bytes per op, all seven columns


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


def _merge_bytes(n: int):
    """(input, output) bytes that hold one merge of n ops as staging() and compose() lay it out."""
    return n * _OP_BYTES + 256 * len(OP_COLS), 5 * _al(4 * n) + 256


_SCREEN_KEYS = ("in_bytes", "out_bytes", "routed")
_CAND_KEYS = _SCREEN_KEYS + ("n_candidates", "retries")


def _last(counters=(), **measured) -> dict:
    """A `last` dict: the three legs in seconds and the counters named, zero unless measured."""
    return {"pack_s": 0.0, "device_s": 0.0, "unpack_s": 0.0, **dict.fromkeys(counters, 0), **measured}


def _over_limit(ren, pairs) -> int:
    """How many of the (i, j) of `pairs` smx_screen sends back (counts -2) and SMX_SCREEN_LARGE
    streams: both logs have renames and together more than SCREEN_MAX_RENAMES."""
    ra, rb = ren[pairs[:, 0]].astype(np.int64), ren[pairs[:, 1]].astype(np.int64)
    return int(((ra > 0) & (rb > 0) & (ra + rb > _abi.SCREEN_MAX_RENAMES)).sum())


def _conf_off(ren, pairs) -> np.ndarray:
    """Where each pair's conflicts start (i64 [n_pairs + 1]): min(renames of log i, of log j) each."""
    return np.concatenate([[0], np.cumsum(np.minimum(ren[pairs[:, 0]], ren[pairs[:, 1]]), dtype=np.int64)])


def screen_results(hout, conf_at: int, counts_at: int, conf_off, pairs) -> list:
    """Per pair of a screen that ran, from the output staging bytes `hout` (the conflict pairs
    from byte conf_at, pair p's from entry conf_off[p]; the i64 counts from byte counts_at):
    its conflict pairs as an (n, 2) int32 copy, or None for a pair the library sent back (counts
    -2).  Another negative count, or one over the pair's capacity, raises SmxError naming it."""
    P = len(pairs)
    counts = hout[counts_at: counts_at + 8 * P].view(np.int64)
    bad = np.flatnonzero((counts < 0) & (counts != -2))
    if len(bad):
        p = int(bad[0])
        raise SmxError(-1, f"pair {p} (logs {int(pairs[p, 0])}, {int(pairs[p, 1])}): invalid input: "
                           "log offsets that decrease or leave the columns, or kind >= 18")
    over = np.flatnonzero(counts > conf_off[1:] - conf_off[:-1])
    if len(over):
        raise SmxError(-2, f"pair {int(over[0])}: {int(counts[over[0]])} conflicts exceed its capacity")
    conf = hout[conf_at: conf_at + 8 * int(conf_off[-1])].view(np.int32).reshape(-1, 2)
    return [None if counts[p] < 0 else conf[int(conf_off[p]): int(conf_off[p]) + int(counts[p])].copy()
            for p in range(P)]


def tree_levels(parents):
    """A tree given as per-node parents in the caller's order (None or -1: a root; a parent
    precedes its children) in the level order smx_compose_tree takes: (order, level_off, back).
    order[i] is the caller's index of the node stored at i -- level by level, nodes of a level
    in the caller's order --, level_off the levels' bounds (int64 [n_levels + 1]) and back its
    inverse: back[order[i]] = i.  A parent at or after its child raises ValueError, an index
    outside the nodes IndexError."""
    par = [-1 if p is None else int(p) for p in parents]
    n = len(par)
    depth = np.zeros(n, np.int64)
    for i, p in enumerate(par):
        if p < -1 or p >= n:
            raise IndexError(f"node {i}: parent {p} outside the {n} nodes")
        if p >= i:
            raise ValueError(f"node {i}: parent {p} does not precede it")
        depth[i] = depth[p] + 1 if p >= 0 else 0
    order = np.argsort(depth, kind="stable").astype(np.int64)
    level_off = np.concatenate([[0], np.cumsum(np.bincount(depth, minlength=0), dtype=np.int64)]).astype(np.int64)
    back = np.empty(n, np.int64)
    back[order] = np.arange(n, dtype=np.int64)
    return order, level_off, back


def tree_room(parents, ren) -> np.ndarray:
    """smx_screen_tree's room rule for a tree in level order (a parent lies before its children;
    any other parent counts as none): per node, with ren[n] the renames of its log, P(n) -- the
    sum of ren over its root path -- if ren[n] > 0, else 0 (int64 [n_nodes])."""
    par, ren = np.asarray(parents, np.int64).tolist(), np.asarray(ren, np.int64).tolist()
    psum = [0] * len(par)
    for n, p in enumerate(par):
        psum[n] = (psum[p] if 0 <= p < n else 0) + ren[n]
    return np.asarray([s if r > 0 else 0 for s, r in zip(psum, ren)], np.int64)


def checked_log_off(lsoa) -> np.ndarray:
    """A LogsSoA's log offsets as contiguous int64, checked: they start at or after 0, do not
    decrease and end inside the columns; else SmxError."""
    log_off = np.ascontiguousarray(lsoa.log_off, dtype=np.int64)
    if int(log_off[0]) < 0 or (log_off[1:] < log_off[:-1]).any() or int(log_off[-1]) > int(lsoa.n_total):
        raise SmxError(-1, "invalid input: the log offsets leave the columns or decrease")
    return log_off


def train_index(lsoa, trains):
    """What compose_trains and screen_trains build of `trains` (lists of log indices over a
    LogsSoA) alike: (train_log, train_off, log_off) -- the trains flattened (int32), their bounds
    in that (int64 [n_trains + 1]) and the checked log offsets.  A log index outside the logs
    raises SmxError naming the train."""
    trains = [np.asarray(tr, np.int32).reshape(-1) for tr in trains]
    L = lsoa.n_logs
    for r, tr in enumerate(trains):
        if len(tr) and (int(tr.min()) < 0 or int(tr.max()) >= L):
            raise SmxError(-1, f"train {r}: a log index outside [0, {L})")
    train_log = np.ascontiguousarray(np.concatenate(trains)) if trains else np.zeros(0, np.int32)
    train_off = np.concatenate([[0], np.cumsum([len(tr) for tr in trains], dtype=np.int64)]).astype(np.int64)
    return train_log, train_off, checked_log_off(lsoa)


def tree_index(lsoa, parents, node_log, order, level_off, back):
    """What compose_tree and screen_tree build of a tree in tree_levels' order alike:
    (lv_par, lv_log, log_off) -- per stored node its parent's place (int32, -1: a root) and its
    log (int32), and the checked log offsets.  More levels than SMX_TREE_MAX_LEVELS or a log
    index outside the logs raises SmxError."""
    N, D, L = len(order), len(level_off) - 1, lsoa.n_logs
    if D > _abi.TREE_MAX_LEVELS:
        raise SmxError(-1, f"a tree of {D} levels: over SMX_TREE_MAX_LEVELS ({_abi.TREE_MAX_LEVELS})")
    logs = np.asarray(node_log, np.int32).reshape(N)
    if int(logs.min()) < 0 or int(logs.max()) >= L:
        raise SmxError(-1, f"node {int(np.flatnonzero((logs < 0) | (logs >= L))[0])}: a log index outside [0, {L})")
    log_off = checked_log_off(lsoa)
    par = np.asarray([-1 if p is None else int(p) for p in parents], np.int64)
    # (level order: the stored parent is the caller's parent's place)
    lv_par = np.where(par[order] >= 0, back[np.maximum(par[order], 0)], -1).astype(np.int32)
    return lv_par, np.ascontiguousarray(logs[order]), log_off


def run_train_loop(st: int, base, state, log_off, train, rec_off, ws, status_host, hook=None, n_acc: int = 0):
    """One train of any size as a host loop over device-resident columns (include/smx.h
    smx_train_step): per step smx_train_stage, smx_compose on the staged columns with
    conflict_cap = max(min(n_acc, log_n), 1), smx_train_land, then the 24 bytes of `status`
    read back on stream `st` -- the step's only read-back -- and the two state buffers flipped
    when the step landed.

    base        an _abi.SmxTrainStep with the log store, the staged columns, the compose result
                (conflicts with room for the largest step's pairs), status and empty_str set;
                its records field is the start of all the steps' records
    state       two 4-tuples of device addresses (src, addr, file, ctx); the train starts with
                the accumulator in state[0], n_acc entries long (0: empty)
    log_off     the logs' offsets (host); a log index outside them, or offsets that decrease
                or leave the columns, give the step -1 on the host, as smx_compose_train does
    rec_off     per step where its records start, in records, n_steps + 1 entries
    ws          ws(nbytes) -> device address of a workspace of at least nbytes
    status_host int64[3] in pinned host memory
    hook        hook(step index, status triple) after each step that ran on the device

    Returns (cur, n_acc, landed, steps): the state buffer that holds the accumulator, its
    length, the steps that landed, and per step (length after it, outcome, status triple or
    None for a step decided on the host)."""
    L = lib()
    off = np.asarray(log_off, np.int64)
    n_total, n_logs = int(base.n_total), len(off) - 1
    before = np.maximum.accumulate(np.concatenate([[0], off[:-1]]))[:-1] if n_logs > 0 else np.zeros(0, np.int64)
    ok = (off[:-1] >= before) & (off[1:] >= off[:-1]) & (off[1:] <= n_total)
    records, h_status = int(base.records or 0), status_host.ctypes.data
    ops = _abi.SmxOps(0, 0, int(base.n_sym), base.st_kind, base.st_ts, base.st_oid_hi, base.st_oid_lo, base.st_sym,
                      base.st_v0, base.st_v1, 0)
    out = _abi.SmxComposeOut(base.order, base.addr, base.file, base.ctx, base.conflicts, 0, base.counts)
    need = C.c_size_t(0)
    cur, landed, steps = 0, 0, []
    for g, l in enumerate(train):
        if not (0 <= l < n_logs) or not ok[l]:
            steps.append((n_acc, -1, None))
            continue
        lo, nb = int(off[l]), int(off[l + 1] - off[l])
        if n_acc + nb == 0:  # (nothing to launch: empty against empty lands)
            landed += 1
            steps.append((0, 0, None))
            continue
        base.n_acc, base.log_lo, base.log_n = n_acc, lo, nb
        base.acc_src, base.acc_addr, base.acc_file, base.acc_ctx = state[cur]
        base.out_src, base.out_addr, base.out_file, base.out_ctx = state[cur ^ 1]
        base.conflict_cap = out.conflict_cap = max(min(n_acc, nb), 1)
        base.records = records + 16 * int(rec_off[g])
        base.record_cap = int(rec_off[g + 1] - rec_off[g])
        ops.n_a, ops.n_b = n_acc, nb
        check(L.smx_train_stage(C.byref(base), st))
        check(L.smx_compose_workspace_bytes(n_acc, nb, ops.n_sym, C.byref(need)))
        rc = L.smx_compose(C.byref(ops), C.byref(out), ws(need.value), need.value, st)
        err = L.smx_last_error().decode(errors="replace") if rc else ""
        check(L.smx_train_land(C.byref(base), st))
        _Staging._copy(h_status, int(base.status), 24, 2, st, "hipMemcpyAsync (status)")
        _hip_check(_hiprt().hipStreamSynchronize(st), "hipStreamSynchronize")
        s = tuple(int(x) for x in status_host)
        if rc and s[0] == 0:  # (a step that stage found invalid is refused by smx_compose too: that is its -1)
            raise SmxError(rc, f"step {g}: {err}")
        if s[1] == 0:
            cur ^= 1
            n_acc = s[2]
            landed += 1
        steps.append((n_acc, s[1], s))
        if hook is not None:
            hook(g, s)
    base.records = records
    return cur, n_acc, landed, steps


class _Staging:
    """One pair of pinned-host and device buffers for a call's input (h_in, d_in) and one for
    its output (h_out, d_out), sized in bytes; hin / hout are the host buffers as numpy bytes.
    Each pair grows alone, to a quarter over the need (at least its floor), and never shrinks."""

    def __init__(self, torch, device, floor_in: int, floor_out: int) -> None:
        self.torch, self.device, self.floor_in, self.floor_out = torch, device, floor_in, floor_out
        self.cap_in = self.cap_out = -1

    def _pair(self, need: int, floor: int):
        cap = max(need + need // 4, floor)
        h = self.torch.empty(cap, dtype=self.torch.uint8, pin_memory=True)
        return cap, h, self.torch.empty(cap, dtype=self.torch.uint8, device=self.device), h.numpy()

    def ensure(self, in_bytes: int, out_bytes: int) -> bool:
        """Room for in_bytes of input and out_bytes of output.  True: a pair was replaced (its
        contents are gone, and the device must sync before another stream uses it)."""
        grow_in, grow_out = in_bytes > self.cap_in, out_bytes > self.cap_out
        if grow_in:
            self.cap_in, self.h_in, self.d_in, self.hin = self._pair(in_bytes, self.floor_in)
        if grow_out:
            self.cap_out, self.h_out, self.d_out, self.hout = self._pair(out_bytes, self.floor_out)
        return grow_in or grow_out

    @staticmethod
    def _copy(dst: int, src: int, nbytes: int, kind: int, st, what: str) -> None:
        _hip_check(_hiprt().hipMemcpyAsync(dst, src, nbytes, kind, st), what)

    def copy_in(self, st, nbytes: int) -> None:
        """The first nbytes of the input, host to device, on stream `st`."""
        self._copy(self.d_in.data_ptr(), self.h_in.data_ptr(), nbytes, 1, st, "hipMemcpyAsync (inputs)")

    def copy_back(self, st, nbytes: int, sync: bool = True) -> None:
        """The first nbytes of the output, device to host, and the stream sync that ends a call."""
        self._copy(self.h_out.data_ptr(), self.d_out.data_ptr(), nbytes, 2, st, "hipMemcpyAsync (outputs)")
        if sync:
            _hip_check(_hiprt().hipStreamSynchronize(st), "hipStreamSynchronize")


class ComposeSession:
    """Reusable buffers for a stream of merges of any size (the drop-in's path): the main
    staging areas (pinned host and device, input and output, each grown alone on demand and
    never shrunk), small auxiliary ones and the workspace.  A merge is one host-to-device
    copy of the packed SoA columns, smx_compose, and one device-to-host copy of the outputs
    and counts -- no allocation after warm-up.  `last` holds the host / device split of the
    last merge in seconds."""

    ASYNC_MAX = 1 << 22  # smx_compose_async + one sync below this many ops (SMX_EARLY_MIN)
    # large=True: merges of up to this many ops join the batch (SMX_BATCH_LARGE: one workgroup
    # each); longer ones belong on the whole chip and go through compose().  Measured (DESIGN.md
    # §16, profiles/batch_large/): the largest probed size at which a batch of 16 merges still
    # beats the loop of smx_compose calls -- 1.9x at 16,000 ops, 0.4x at 64,000.
    LARGE_MAX = 16000

    def __init__(self, device: str = "cuda") -> None:
        self.torch = _torch()
        self.device = self.torch.device(device)
        self.main = _Staging(self.torch, self.device, 1024 * _OP_BYTES, 1024 * 20 + 256)  # (1024 ops at least)
        # (small ones for screen_all's second call: the first call's columns and pairs stay on the device)
        self.aux = _Staging(self.torch, self.device, 4096, 4096)
        self.cap_ws = -1
        self.last = {}
        self.busy = False  # results handed out as views are being read (dropin_session)
        # its own stream: repeated merges of one size replay the library's HIP graph
        self.stream = self.torch.cuda.Stream(self.device)

    def _ensure(self, area: _Staging, in_bytes: int, out_bytes: int, ws_bytes: int) -> None:
        grown = area.ensure(in_bytes, out_bytes)
        if ws_bytes > self.cap_ws:
            self.ws = self.torch.empty(max(ws_bytes, 1), dtype=self.torch.uint8, device=self.device)
            self.cap_ws = ws_bytes
            grown = True
        if grown:  # new buffers come from the current stream's pool: ready before the session's stream uses them
            self.torch.cuda.synchronize(self.device)

    def staging(self, n: int) -> dict:
        """The input columns of an n-op merge as views of the pinned staging area, laid out
        as compose() copies it: a SoA marshalled into them is not packed again."""
        self._ensure(self.main, *_merge_bytes(n), 0)
        hin, cols, off = self.main.hin, {}, 0
        for name, dt, _ in OP_COLS:
            cols[name] = hin[off: off + n * dt.itemsize].view(dt)
            off += _al(n * dt.itemsize)
        return cols

    def compose(self, soa: SoA, copy: bool = True):
        """(order, addr, file, ctx, conflict_pairs) of one merge, computed on the GPU.
        copy=False: views of the session's pinned staging area, valid until its next merge
        (the drop-in materialises them at once)."""
        t0 = time.perf_counter()
        n = soa.n
        if n == 0:
            e = np.zeros(0, np.int32)
            return e, e, e, e, np.zeros((0, 2), np.int32)
        ws = C.c_size_t(0)
        check(lib().smx_compose_workspace_bytes(soa.n_a, soa.n_b, soa.n_sym, C.byref(ws)))
        m = self.main
        self._ensure(m, *_merge_bytes(n), ws.value)
        hin, h0, d0 = m.hin, m.hin.ctypes.data, m.d_in.data_ptr()
        off, ptrs = 0, {}
        for name, dt, _ in OP_COLS:   # pack the columns into the pinned staging area (laid out for n)
            w = dt.itemsize
            _pack(hin, h0, getattr(soa, name), off, n * w)
            ptrs[name] = d0 + off
            off += _al(n * w)
        t1 = time.perf_counter()
        st = self.stream.cuda_stream
        m.copy_in(st, off)
        ccap = max(min(soa.n_a, soa.n_b), 1)
        o0 = m.d_out.data_ptr()
        q = _al(n * 4)             # outputs laid out for n: one contiguous copy back
        ops = _abi.SmxOps(soa.n_a, soa.n_b, soa.n_sym, ptrs["kind"], ptrs["ts"], ptrs["oid_hi"],
                          ptrs["oid_lo"], ptrs["sym"], ptrs["v0"], ptrs["v1"])
        cnt_off = 4 * q + _al(8 * ccap)
        out = _abi.SmxComposeOut(o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + 4 * q, ccap, o0 + cnt_off)
        args = (C.byref(ops), C.byref(out), self.ws.data_ptr(), ws.value, st)
        hout = m.hout

        def copy_back():
            m.copy_back(st, cnt_off + 16)
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

    def _staged_call(self, area: _Staging, query, sizes, lay, cols, index, make_arg, fn, staged: Optional[int] = None):
        """One call through the staging areas of `area`: the workspace `query(*sizes)` asks
        for, the columns `cols` ((column, byte offset, nbytes)) and the index arrays `index`
        ((name, array)) packed at their places in `lay`, one host-to-device copy,
        fn(make_arg(device input address, device output address)), one copy back, one stream
        sync.  `staged`: the device address these inputs were last copied to; while it is still
        the area's, they are not packed or copied again.  Returns the times after the pack
        (None: nothing was packed) and after the sync."""
        ws = C.c_size_t(0)
        check(query(*sizes, C.byref(ws)))
        self._ensure(area, lay["in_bytes"], lay["out_bytes"], ws.value)
        st, d0, t1 = self.stream.cuda_stream, area.d_in.data_ptr(), None
        if staged != d0:
            hin, h0 = area.hin, area.hin.ctypes.data
            for col, at, nbytes in cols:
                _pack(hin, h0, col, at, nbytes)
            for name, arr in index:
                _pack(hin, h0, arr, lay[name], arr.nbytes)
            t1 = time.perf_counter()
            area.copy_in(st, lay["in_bytes"])
        check(fn(C.byref(make_arg(d0, area.d_out.data_ptr())), self.ws.data_ptr(), ws.value, st))
        area.copy_back(st, lay["out_bytes"])
        return t1, time.perf_counter()

    def _batch_results(self, lay, conf_off, starts, labels, what: str = "merge"):
        """Per merge of a batch that ran: its results (views of the output staging area,
        from entry starts[m] of the four arrays), or None for a merge the library sent back
        (counts -2).  labels[m] names merge m (`what` labels[m]) in an error."""
        hout = self.main.hout
        counts = hout[lay["counts"]: lay["counts"] + 16 * len(labels)].view(np.int64).tolist()
        q, conf, co, starts = lay["q"], lay["conf"], conf_off.tolist(), starts.tolist()
        res = []
        for m, i in enumerate(labels):
            k, nc = counts[2 * m], counts[2 * m + 1]
            if k == -2:
                res.append(None)
                continue
            if k < 0:
                raise SmxError(-1, f"{what} {i}: invalid input: sym >= n_sym or kind >= 18")
            if nc > co[m + 1] - co[m]:
                raise SmxError(-2, f"{what} {i}: {nc} conflicts exceed capacity {co[m + 1] - co[m]}")
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

    # (the three batched composes share four more: the limit, the layout, the struct's end, the results' way)
    def _limit(self, large: bool, large_max: Optional[int]) -> int:
        """The most ops of a merge that runs in the batch (large_max: default LARGE_MAX, at least BATCH_MAX_OPS)."""
        if not large:
            return _abi.BATCH_MAX_OPS
        return self.LARGE_MAX if large_max is None else max(int(large_max), _abi.BATCH_MAX_OPS)

    @staticmethod
    def _compose_layout(n_total: int, index, n_out: int, conf_bytes: int, n_items: int) -> dict:
        """Byte offsets of a batched compose: the seven columns for n_total ops, then the index arrays ((name,
        nbytes)); the four outputs of n_out entries (q bytes each), the conflict pairs, n_items pairs of counts."""
        q = _al(n_out * 4)
        return {"q": q, **ComposeSession._layout(
            n_total, [(name, n_total * dt.itemsize) for name, dt, _ in OP_COLS] + index, q, conf_bytes, 16 * n_items)}

    def _columns(self, lay, n_total: int, cols=OP_COLS) -> dict:
        """The columns `cols` of n_total ops as views of the pinned staging area, at their places in `lay`."""
        self._ensure(self.main, lay["in_bytes"], lay["out_bytes"], 0)
        hin = self.main.hin
        return {name: hin[lay[name]: lay[name] + n_total * dt.itemsize].view(dt) for name, dt, _ in cols}

    @staticmethod
    def _out_fields(lay, d0: int, o0: int):
        """The struct fields behind every form's inputs: the four results, conflicts, conf_off and counts."""
        q = lay["q"]
        return o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + lay["conf"], d0 + lay["conf_off"], o0 + lay["counts"]

    @staticmethod
    def _take(res, routed, labels, results, copy: bool) -> None:
        """results[m] into res[labels[m]], the items sent back (None) onto `routed`; copies unless
        copy is False and nothing is routed (compose() of a routed item reuses the staging area)."""
        for i, r in zip(labels, results):
            res[i] = r
            if r is None:
                routed.append(i)
        if copy or routed:
            res[:] = [r if r is None else tuple(x.copy() for x in r) for r in res]

    # -- batched compose (smx_compose_batch): many small merges, one launch sequence --------

    @staticmethod
    def _batch_layout(ns):
        """Byte offsets of a batch of merges of ns ops in the staging areas: the input
        columns for sum(ns) ops, then off / n_a / conf_off; the four outputs, the conflict
        pairs (at most sum(ns) / 2) and the counts."""
        m, tot = len(ns), int(sum(ns))
        return ComposeSession._compose_layout(tot, [("off", (m + 1) * 8), ("n_a", m * 8), ("conf_off", (m + 1) * 8)],
                                              tot, 4 * tot, m)

    def staging_many(self, ns):
        """The input columns of a batch of merges of ns ops (each at most BATCH_MAX_OPS, or with
        compose_many(large=True) of any size) as views of the pinned staging area, one dict per
        merge, laid out as compose_many() copies them: SoAs marshalled into them are not packed
        again."""
        lay = self._batch_layout(ns)
        self._ensure(self.main, lay["in_bytes"], lay["out_bytes"], 0)
        hin = self.main.hin
        offs = np.concatenate([[0], np.cumsum(ns, dtype=np.int64)]) if len(ns) else np.zeros(1, np.int64)
        return [{name: hin[lay[name] + int(offs[m]) * dt.itemsize: lay[name] + int(offs[m + 1]) * dt.itemsize].view(dt)
                 for name, dt, _ in OP_COLS} for m in range(len(ns))]

    def compose_many(self, soas, copy: bool = True, large: bool = False, large_max: Optional[int] = None):
        """[(order, addr, file, ctx, conflict_pairs)] of independent merges, in input order.
        The merges of at most BATCH_MAX_OPS ops are packed at consecutive offsets of the
        staging area and run as one batch: one host-to-device copy, one smx_compose_batch,
        one copy back, one stream sync.  Larger merges (and any the library sends back,
        counts -2) go through compose() afterwards.  An invalid merge raises SmxError naming
        its index.  copy=False: views of the staging area, valid until the session's next
        merge (taken only when no merge is routed through compose()).  large=True: merges of up
        to large_max ops (default LARGE_MAX, measured: DESIGN.md §16) join the batch too (smx_compose_batch_ex
        with SMX_BATCH_LARGE), and only longer ones go through compose(); `last` then holds the
        call's legs, "large" (merges over BATCH_MAX_OPS ops that ran in the batch) and "routed"."""
        t0 = time.perf_counter()
        soas = list(soas)
        flags = _abi.BATCH_LARGE if large else 0
        limit = self._limit(large, large_max)
        small = [i for i, s in enumerate(soas) if s.n <= limit]
        routed = [i for i, s in enumerate(soas) if s.n > limit]
        res = [None] * len(soas)
        legs = _last(("large", "routed"))
        if small:
            M = len(small)
            ns = [soas[i].n for i in small]
            lay = self._batch_layout(ns)
            off = np.concatenate([[0], np.cumsum(ns, dtype=np.int64)])
            n_a = np.fromiter((soas[i].n_a for i in small), np.int64, M)
            # (conflict capacities of min(n_a, n_b): never truncate)
            conf_off = np.concatenate([[0], np.cumsum(np.minimum(n_a, off[1:] - off[:-1] - n_a), dtype=np.int64)])
            n_sym, cols = 1, []
            for m, i in enumerate(small):
                soa, n = soas[i], ns[m]
                n_sym = max(n_sym, int(soa.n_sym))
                if n and int(np.max(soa.sym)) >= soa.n_sym:  # (the batch has one bound for all its merges)
                    raise SmxError(-1, f"merge {i}: invalid input: sym >= n_sym")
                cols += [(getattr(soa, name), lay[name] + int(off[m]) * dt.itemsize, n * dt.itemsize)
                         for name, dt, _ in OP_COLS]
            t1, t2 = self._staged_call(
                self.main, lib().smx_compose_batch_ex_workspace_bytes, (M, lay["n_total"], flags), lay, cols,
                (("off", off), ("n_a", n_a), ("conf_off", conf_off)),
                lambda d0, o0: _abi.SmxBatch(M, lay["n_total"], n_sym, d0 + lay["off"], d0 + lay["n_a"],
                                             *[d0 + lay[name] for name, _, _ in OP_COLS],
                                             *self._out_fields(lay, d0, o0), 0),
                lambda arg, ws, nbytes, st: lib().smx_compose_batch_ex(arg, ws, nbytes, flags, st))
            self._take(res, routed, small, self._batch_results(lay, conf_off, off[:-1], small), copy)
            legs = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2,
                         large=sum(n > _abi.BATCH_MAX_OPS for n in ns) if large else 0)
        routed.sort()
        self._compose_routed(res, routed, [soas[i] for i in routed], "merge", keep_last=False)
        if large:
            self.last = {**legs, "routed": len(routed)}
        return res

    # -- batched compose against one shared log (smx_compose_batch_shared) -------------------

    @staticmethod
    def _shared_layout(n_total: int, n_shared: int, m: int):
        """Byte offsets of a shared-log batch in the staging areas: the input columns for
        n_total ops (the shared log once), then off / conf_off; the four outputs of
        n_total - n_shared + m * n_shared entries, the conflict pairs (at most
        n_total - n_shared) and the counts."""
        return ComposeSession._compose_layout(n_total, [("off", (m + 1) * 8), ("conf_off", (m + 1) * 8)],
                                              n_total - n_shared + m * n_shared, 8 * (n_total - n_shared), m)

    def staging_shared(self, n_total: int, n_shared: int, n_merges: int) -> dict:
        """The input columns of a shared-log batch of n_total ops (of any size) as views of the
        pinned staging area, laid out as compose_shared() copies them: a SharedSoA marshalled
        into them is not packed again."""
        return self._columns(self._shared_layout(n_total, n_shared, n_merges), n_total)

    def compose_shared(self, ssoa, shared_is_b: bool = False, copy: bool = True, large: bool = False,
                       large_max: Optional[int] = None):
        """[(order, addr, file, ctx, conflict_pairs)] of the merges (shared, branch m) -- or
        (branch m, shared) with shared_is_b -- of a SharedSoA, in branch order.  The columns,
        the shared log once, are staged as they are: one host-to-device copy, one
        smx_compose_batch_shared, one copy back, one stream sync.  Merges over BATCH_MAX_OPS
        ops (the library sends them back, counts -2) go through compose(ssoa.merge(m))
        afterwards.  Invalid input raises SmxError naming the merge.  copy=False: views of
        the staging area, valid until the session's next merge (taken only when no merge is
        routed through compose()).  large=True: merges of up to large_max ops, the shared log
        counted (default LARGE_MAX), run in the batch too (smx_compose_batch_shared_ex
        with SMX_BATCH_LARGE) and `last` gains "large" and "routed"; the call takes every merge
        of the columns or none, so a batch that holds a merge over large_max runs as large=False
        does (that merge and every other one over BATCH_MAX_OPS ops through compose())."""
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
        self.last = _last(("in_bytes",) + (("large", "routed") if large else ()))
        flags = _abi.BATCH_LARGE if large and M and bool((S + lens <= self._limit(large, large_max)).all()) else 0
        n_large = int((S + lens > _abi.BATCH_MAX_OPS).sum()) if flags else 0
        if M and (flags or (S + lens <= _abi.BATCH_MAX_OPS).any()):
            lay = self._shared_layout(tot, S, M)
            conf_off = np.concatenate([[0], np.cumsum(np.minimum(lens, S), dtype=np.int64)])  # (never truncates)
            routed = []
            t1, t2 = self._staged_call(
                self.main, lib().smx_compose_batch_shared_ex_workspace_bytes, (M, tot, S, flags), lay,
                [(getattr(ssoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in OP_COLS],
                (("off", off), ("conf_off", conf_off)),
                lambda d0, o0: _abi.SmxBatchShared(M, tot, int(ssoa.n_sym), S, d0 + lay["off"],
                                                   *[d0 + lay[name] for name, _, _ in OP_COLS],
                                                   *self._out_fields(lay, d0, o0), 0, int(bool(shared_is_b))),
                lambda arg, ws, nbytes, st: lib().smx_compose_batch_shared_ex(arg, ws, nbytes, flags, st))
            self._take(res, routed, range(M),
                       self._batch_results(lay, conf_off, off[:-1] + (np.arange(M) - 1) * S, range(M)), copy)
            self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2,
                              in_bytes=lay["in_bytes"])
        else:
            routed = list(range(M))
        if large:
            self.last.update(large=n_large, routed=len(routed))
        if routed:
            # (copies: the columns may be views of the staging area that compose() packs into)
            self._compose_routed(res, routed, [ssoa.merge(m, shared_is_b) for m in routed], "merge")
        return res

    # -- batched compose of pairs of logs stored once (smx_compose_pairs) ----------------------

    @staticmethod
    def _pairs_layout(n_total: int, n_logs: int, n_pairs: int, n_out: int = 0, n_conf: int = 0):
        """Byte offsets of a pairs batch in the staging areas: the seven input columns for
        n_total ops (every log once), then log_off / pair_a / pair_b / res_off / conf_off; the
        four outputs of n_out entries, the conflict pairs and the counts."""
        return ComposeSession._compose_layout(
            n_total, [("log_off", (n_logs + 1) * 8), ("pair_a", n_pairs * 4), ("pair_b", n_pairs * 4),
                      ("res_off", (n_pairs + 1) * 8), ("conf_off", (n_pairs + 1) * 8)], n_out, 8 * n_conf, n_pairs)

    def staging_pairs(self, n_total: int, n_logs: int, n_pairs: int) -> dict:
        """The seven input columns of a pairs batch of n_total ops as views of the pinned staging
        area, laid out as compose_pairs() copies them (the columns come first, so their places
        depend on n_total alone): a LogsSoA marshalled into them is not packed again."""
        return self._columns(self._pairs_layout(n_total, n_logs, n_pairs), n_total)

    def compose_pairs(self, lsoa, pairs, copy: bool = True, large: bool = False, large_max: Optional[int] = None):
        """[(order, addr, file, ctx, conflict_pairs)] of the merges (log i, log j) for every
        (i, j) of `pairs` over a LogsSoA, in input order, each as compose(lsoa.pair(i, j)) gives
        it.  The columns, every log once, are staged as they are: one host-to-device copy (37
        bytes per op of the logs plus the index arrays, whatever the number of pairs that hold a
        log), one smx_compose_pairs, one copy back, one stream sync.  Pairs over BATCH_MAX_OPS
        ops (and any the library sends back, counts -2) go through compose(lsoa.pair(i, j))
        afterwards.  Invalid input raises SmxError naming the pair.  copy=False: views of the
        staging area, valid until the session's next merge (taken only when no pair is routed
        through compose()).  large=True: pairs of up to large_max ops (default LARGE_MAX) run in
        the batch too (SMX_BATCH_LARGE) and only longer ones are routed.  `last` holds the
        call's legs, "in_bytes", "large" (pairs over BATCH_MAX_OPS ops that ran in the batch) and
        "routed"."""
        t0 = time.perf_counter()
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        P, L, tot = len(pairs), lsoa.n_logs, int(lsoa.n_total)
        self.last = _last(("in_bytes", "large", "routed"))
        if P == 0:
            return []
        bad = np.flatnonzero(((pairs < 0) | (pairs >= L)).any(axis=1))
        if len(bad):
            raise SmxError(-1, f"pair {int(bad[0])}: a log index outside [0, {L})")
        log_off = checked_log_off(lsoa)
        lens = log_off[1:] - log_off[:-1]
        if tot:  # (the batch has one bound for all its symbols; entries that no log covers are no pair's)
            over = np.flatnonzero(np.asarray(lsoa.sym) >= lsoa.n_sym)
            held = np.zeros(L, bool)
            held[pairs.reshape(-1)] = True
            for at in over.tolist():
                l = int(np.searchsorted(log_off, at, "right")) - 1
                if 0 <= l < L and at < log_off[l + 1] and held[l]:
                    p = int(np.flatnonzero((pairs == l).any(axis=1))[0])
                    raise SmxError(-1, f"pair {p}: invalid input: sym >= n_sym")
        la, lb = lens[pairs[:, 0]], lens[pairs[:, 1]]
        flags = _abi.BATCH_LARGE if large else 0
        limit = self._limit(large, large_max)
        inb = np.flatnonzero(la + lb <= limit)
        routed = np.flatnonzero(la + lb > limit).tolist()
        res = [None] * P
        if len(inb):
            M = len(inb)
            sub = np.ascontiguousarray(pairs[inb])
            na, nb = la[inb], lb[inb]
            res_off = np.concatenate([[0], np.cumsum(na + nb, dtype=np.int64)])
            conf_off = np.concatenate([[0], np.cumsum(np.minimum(na, nb), dtype=np.int64)])  # (never truncates)
            n_out = int(res_off[-1])
            lay = self._pairs_layout(tot, L, M, n_out, int(conf_off[-1]))
            t1, t2 = self._staged_call(
                self.main, lib().smx_compose_pairs_workspace_bytes, (L, M, n_out, flags), lay,
                [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in OP_COLS],
                (("log_off", log_off), ("pair_a", np.ascontiguousarray(sub[:, 0])),
                 ("pair_b", np.ascontiguousarray(sub[:, 1])), ("res_off", res_off), ("conf_off", conf_off)),
                lambda d0, o0: _abi.SmxPairs(L, tot, M, int(lsoa.n_sym), n_out, d0 + lay["log_off"],
                                             *[d0 + lay[name] for name, _, _ in OP_COLS],
                                             d0 + lay["pair_a"], d0 + lay["pair_b"], d0 + lay["res_off"],
                                             *self._out_fields(lay, d0, o0), 0),
                lambda arg, ws, nbytes, st: lib().smx_compose_pairs(arg, ws, nbytes, flags, st))
            self._take(res, routed, inb.tolist(),
                       self._batch_results(lay, conf_off, res_off[:-1], inb.tolist(), "pair"), copy)
            self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2,
                              in_bytes=lay["in_bytes"],
                              large=int((na + nb > _abi.BATCH_MAX_OPS).sum()) if large else 0)
        routed.sort()
        self.last["routed"] = len(routed)
        if routed:
            # (copies: the columns may be views of the staging area that compose() packs into)
            self._compose_routed(res, routed, [lsoa.pair(int(pairs[p, 0]), int(pairs[p, 1])) for p in routed], "pair")
        return res

    # -- merge trains over logs stored once (smx_compose_train) --------------------------------

    def compose_trains(self, lsoa, trains, v1_alt=None, empty_str: int = -1):
        """Per train of `trains` (lists of log indices over a LogsSoA) what smx_compose_train leaves:
        (src, addr, file, ctx, landed, steps) -- the final accumulator (column indices and the
        accumulated addr / file / ctx), the number of steps that landed, and per step
        (accumulator length after it, outcome, its conflict records as an (n, 4) array).  The
        columns, every log once, are staged as they are: one host-to-device copy, one
        smx_compose_train, one copy back, one stream sync, whatever the number of trains and
        steps.  A step of outcome -2 (accumulator plus log over BATCH_MAX_OPS ops) is reported as
        it is: the caller finishes that train elsewhere.  Invalid input raises SmxError naming the
        train.  v1_alt, empty_str: smx_train's two (marshal.move_file_alt).  The results are
        copies.  `last` holds the call's legs and "in_bytes"."""
        t0 = time.perf_counter()
        R, L, tot = len(trains), lsoa.n_logs, int(lsoa.n_total)
        self.last = _last(("in_bytes",))
        if R == 0:
            return []
        train_log, train_off, log_off = train_index(lsoa, trains)
        S = len(train_log)
        lens = log_off[1:] - log_off[:-1]
        step_len = lens[train_log] if S else np.zeros(0, np.int64)
        csum = np.concatenate([[0], np.cumsum(step_len, dtype=np.int64)])
        res_off = np.concatenate([[0], np.cumsum(csum[train_off[1:]] - csum[train_off[:-1]], dtype=np.int64)])
        conf_off = csum.astype(np.int64)  # (a step has at most as many conflicts as its log has ops)
        n_out, n_conf = int(res_off[-1]), int(conf_off[-1])
        alt = np.zeros(tot, np.int32) if v1_alt is None else np.ascontiguousarray(v1_alt, dtype=np.int32)
        lay = self._compose_layout(tot, [("v1_alt", tot * 4), ("log_off", (L + 1) * 8), ("train_off", (R + 1) * 8),
                                         ("train_log", S * 4), ("res_off", (R + 1) * 8), ("conf_off", (S + 1) * 8)],
                                   n_out, 16 * n_conf, 0)
        lay["step_counts"] = lay["counts"] + _al(16 * R)
        lay["out_bytes"] = lay["step_counts"] + 16 * S
        q = lay["q"]
        t1, t2 = self._staged_call(
            self.main, lib().smx_compose_train_workspace_bytes, (L, R, S, n_out, 0), lay,
            [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in OP_COLS],
            (("v1_alt", alt), ("log_off", log_off), ("train_off", train_off), ("train_log", train_log),
             ("res_off", res_off), ("conf_off", conf_off)),
            lambda d0, o0: _abi.SmxTrain(L, tot, R, S, int(lsoa.n_sym), n_out, d0 + lay["log_off"],
                                         *[d0 + lay[name] for name, _, _ in OP_COLS], d0 + lay["v1_alt"],
                                         d0 + lay["train_off"], d0 + lay["train_log"], d0 + lay["res_off"],
                                         o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + lay["conf"], d0 + lay["conf_off"],
                                         o0 + lay["counts"], o0 + lay["step_counts"], 0, int(empty_str)),
            lambda arg, ws, nbytes, st: lib().smx_compose_train(arg, ws, nbytes, 0, st))
        hout = self.main.hout
        counts = hout[lay["counts"]: lay["counts"] + 16 * R].view(np.int64).tolist()
        sc = hout[lay["step_counts"]: lay["step_counts"] + 16 * S].view(np.int64).tolist()
        conf = hout[lay["conf"]: lay["conf"] + 16 * n_conf].view(np.int32).reshape(-1, 4)
        res = []
        for r in range(R):
            k, landed = counts[2 * r], counts[2 * r + 1]
            if k < 0:
                raise SmxError(-1, f"train {r}: invalid input")
            steps = []
            for g in range(int(train_off[r]), int(train_off[r + 1])):
                oc, c = sc[2 * g + 1], int(conf_off[g])
                if oc == -1:
                    raise SmxError(-1, f"train {r}, step {g - int(train_off[r])}: invalid input: sym >= n_sym or kind >= 18")
                steps.append((sc[2 * g], oc, conf[c: c + max(oc, 0)].copy()))
            o = int(res_off[r])
            res.append(tuple(hout[f * q + 4 * o: f * q + 4 * (o + k)].view(np.int32).copy() for f in range(4))
                       + (landed, steps))
        self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2, in_bytes=lay["in_bytes"])
        return res

    # -- trains that share prefixes: a tree of logs, every node composed once (smx_compose_tree) --

    def compose_tree(self, lsoa, parents, node_log, v1_alt=None, empty_str: int = -1):
        """Per node of a tree over a LogsSoA what smx_compose_tree leaves, in the caller's order:
        (state, acc, length, outcome, records).  parents[n]: the node's parent (None or -1: a
        root; a parent precedes its children, tree_levels), node_log[n]: its log.  state: the
        node's own accumulator (src, addr, file, ctx) if it landed, else None; acc: the node
        whose state is this node's accumulator (itself if it landed, -1: the accumulator is
        empty), `length` entries long; outcome: its conflicts, or -2 (accumulator plus log over
        BATCH_MAX_OPS ops), reported as it is; records: its conflict records as an (n, 4) array.
        The columns, every log once, are staged as they are: one host-to-device copy, one
        smx_compose_tree, one copy back, one stream sync, whatever the tree.  Invalid input raises
        SmxError naming the node.  v1_alt, empty_str: smx_tree's two (marshal.move_file_alt).
        The results are copies.  `last` holds the call's legs and "in_bytes"."""
        t0 = time.perf_counter()
        order, level_off, back = tree_levels(parents)
        N, D, L, tot = len(order), len(level_off) - 1, lsoa.n_logs, int(lsoa.n_total)
        self.last = _last(("in_bytes",))
        if N == 0:
            return []
        lv_par, lv_log, log_off = tree_index(lsoa, parents, node_log, order, level_off, back)
        lv_len = (log_off[1:] - log_off[:-1])[lv_log]
        psum = np.zeros(N, np.int64)
        for d in range(D):  # (a level's path sums from the level before)
            a, b = int(level_off[d]), int(level_off[d + 1])
            psum[a:b] = lv_len[a:b] + (psum[lv_par[a:b]] if d else 0)
        res_off = np.concatenate([[0], np.cumsum(np.minimum(psum, _abi.BATCH_MAX_OPS), dtype=np.int64)])
        conf_off = np.concatenate([[0], np.cumsum(lv_len, dtype=np.int64)])  # (at most a conflict per op of the log)
        n_out, n_conf = int(res_off[-1]), int(conf_off[-1])
        alt = np.zeros(tot, np.int32) if v1_alt is None else np.ascontiguousarray(v1_alt, dtype=np.int32)
        lay = self._compose_layout(tot, [("v1_alt", tot * 4), ("log_off", (L + 1) * 8), ("level_off", (D + 1) * 8),
                                         ("node_parent", N * 4), ("node_log", N * 4), ("res_off", (N + 1) * 8),
                                         ("conf_off", (N + 1) * 8)], n_out, 16 * n_conf, 0)
        lay["node_acc"] = lay["counts"] + _al(16 * N)
        lay["out_bytes"] = lay["node_acc"] + 4 * N
        q = lay["q"]
        t1, t2 = self._staged_call(
            self.main, lib().smx_compose_tree_workspace_bytes, (L, N, D, n_out, 0), lay,
            [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in OP_COLS],
            (("v1_alt", alt), ("log_off", log_off), ("level_off", level_off), ("node_parent", lv_par),
             ("node_log", lv_log), ("res_off", res_off), ("conf_off", conf_off)),
            lambda d0, o0: _abi.SmxTree(L, tot, N, D, int(lsoa.n_sym), n_out, d0 + lay["log_off"],
                                        *[d0 + lay[name] for name, _, _ in OP_COLS], d0 + lay["v1_alt"],
                                        d0 + lay["level_off"], d0 + lay["node_parent"], d0 + lay["node_log"],
                                        d0 + lay["res_off"], o0, o0 + q, o0 + 2 * q, o0 + 3 * q, o0 + lay["conf"],
                                        d0 + lay["conf_off"], o0 + lay["counts"], o0 + lay["node_acc"], 0,
                                        int(empty_str)),
            lambda arg, ws, nbytes, st: lib().smx_compose_tree(arg, ws, nbytes, 0, st))
        hout = self.main.hout
        counts = hout[lay["counts"]: lay["counts"] + 16 * N].view(np.int64).tolist()
        acc = hout[lay["node_acc"]: lay["node_acc"] + 4 * N].view(np.int32).tolist()
        conf = hout[lay["conf"]: lay["conf"] + 16 * n_conf].view(np.int32).reshape(-1, 4)
        res = [None] * N
        for i in range(N):
            n, k, oc = int(order[i]), counts[2 * i], counts[2 * i + 1]
            if k < 0:
                raise SmxError(-1, f"node {n}: invalid input")
            if oc == -1:
                raise SmxError(-1, f"node {n}: invalid input: sym >= n_sym or kind >= 18")
            state = None
            if acc[i] == i:
                o = int(res_off[i])
                state = tuple(hout[f * q + 4 * o: f * q + 4 * (o + k)].view(np.int32).copy() for f in range(4))
            c = int(conf_off[i])
            res[n] = (state, int(order[acc[i]]) if acc[i] >= 0 else -1, k, oc, conf[c: c + max(oc, 0)].copy())
        self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2, in_bytes=lay["in_bytes"])
        return res

    # -- one train of any size: the host loop of smx_train_stage, smx_compose, smx_train_land ----

    def compose_train_loop(self, lsoa, train, v1_alt=None, empty_str: int = -1):
        """compose_trains' result for one train, (src, addr, file, ctx, landed, steps), with no
        limit on a step's size and so no outcome -2: the columns, every log once, are copied in
        once, and every step is smx_train_stage, smx_compose on the staged columns and
        smx_train_land on the session's stream, over buffers that stay on the device
        (run_train_loop: 24 bytes read back per step).  The final accumulator and the records are
        copied back once at the end.  A step over 2048 ops takes smx_compose's sorting plans: the
        accumulator is kind-major, not timestamp-ordered.  Invalid input raises
        SmxError naming the step.  The results are copies.  `last` holds the call's legs and
        "in_bytes"."""
        t0 = time.perf_counter()
        train = [int(l) for l in np.asarray(train, np.int64).reshape(-1)]
        L, tot, S = lsoa.n_logs, int(lsoa.n_total), len(train)
        if any(not 0 <= l < L for l in train):
            raise SmxError(-1, f"a log index outside [0, {L})")
        log_off = checked_log_off(lsoa)
        lens = log_off[1:] - log_off[:-1]
        rec_off = np.concatenate([[0], np.cumsum(lens[train] if S else [], dtype=np.int64)]).astype(np.int64)
        cap = int(rec_off[-1])  # (the accumulator holds at most every op of the train's steps)
        alt = np.zeros(tot, np.int32) if v1_alt is None else np.ascontiguousarray(v1_alt, dtype=np.int32)
        # in: the columns and v1_alt.  out: the two state buffers and the records (what is copied
        # back), then what only the device sees: the staged columns, the compose result, status
        q = _al(4 * cap)
        lay = self._layout(tot, [(name, tot * dt.itemsize) for name, dt, _ in OP_COLS] + [("v1_alt", tot * 4)], 0, 0, 0)
        o, scratch = 8 * q + _al(16 * cap), {}
        for name, nbytes in [("st_" + name, cap * dt.itemsize) for name, dt, _ in OP_COLS] + \
                            [(name, 4 * cap) for name in ("order", "addr", "file", "ctx")] + \
                            [("conflicts", 4 * cap + 8), ("counts", 16), ("status", 24)]:
            scratch[name] = o
            o += _al(nbytes)
        m = self.main
        self._ensure(m, lay["in_bytes"], o, 0)
        hin, h0, d0, o0 = m.hin, m.hin.ctypes.data, m.d_in.data_ptr(), m.d_out.data_ptr()
        for name, dt, _ in OP_COLS:
            _pack(hin, h0, getattr(lsoa, name), lay[name], tot * dt.itemsize)
        _pack(hin, h0, alt, lay["v1_alt"], alt.nbytes)
        t1 = time.perf_counter()
        st = self.stream.cuda_stream
        m.copy_in(st, lay["in_bytes"])
        if getattr(self, "_status_host", None) is None:
            self._status_host = self.torch.zeros(3, dtype=self.torch.int64, pin_memory=True)
        base = _abi.SmxTrainStep(n_total=tot, n_sym=int(lsoa.n_sym), **{name: d0 + lay[name] for name, _, _ in OP_COLS},
                                 v1_alt=d0 + lay["v1_alt"], records=o0 + 8 * q, empty_str=int(empty_str),
                                 **{name: o0 + at for name, at in scratch.items()})

        def ws(nbytes: int) -> int:
            self._ensure(m, 0, 0, nbytes)
            return self.ws.data_ptr()

        state = tuple(tuple(o0 + (4 * b + f) * q for f in range(4)) for b in range(2))
        cur, n_acc, landed, ran = run_train_loop(st, base, state, log_off, train, rec_off, ws, self._status_host.numpy())
        h_out = m.h_out.data_ptr()
        if n_acc:
            m._copy(h_out + 4 * cur * q, o0 + 4 * cur * q, 3 * q + 4 * n_acc, 2, st, "hipMemcpyAsync (accumulator)")
        if cap:
            m._copy(h_out + 8 * q, o0 + 8 * q, 16 * cap, 2, st, "hipMemcpyAsync (records)")
        _hip_check(_hiprt().hipStreamSynchronize(st), "hipStreamSynchronize")
        t2 = time.perf_counter()
        hout = m.hout
        recs = hout[8 * q: 8 * q + 16 * cap].view(np.int32).reshape(-1, 4)
        steps = []
        for g, (acc, oc, _) in enumerate(ran):
            if oc == -1:
                raise SmxError(-1, f"step {g}: invalid input: sym >= n_sym or kind >= 18")
            c = int(rec_off[g])
            steps.append((acc, oc, recs[c: c + min(max(oc, 0), int(rec_off[g + 1]) - c)].copy()))
        fin = 4 * cur * q
        res = tuple(hout[fin + f * q: fin + f * q + 4 * n_acc].view(np.int32).copy() for f in range(4)) + (landed, steps)
        self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2, in_bytes=lay["in_bytes"])
        return res

    # -- conflict screen (smx_screen): many pairs of logs stored once, conflicts only ---------

    @staticmethod
    def _screen_layout(n_total: int, n_logs: int, n_pairs: int, n_conf: int = 0):
        """Byte offsets of a screen in the staging areas: the six input columns for n_total
        ops, then log_off / pair_a / pair_b / conf_off; the conflict pairs and the counts."""
        lay = ComposeSession._layout(n_total, [(name, n_total * dt.itemsize) for name, dt, _ in SCREEN_COLS]
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
        cols = self._columns(self._screen_layout(n_total, n_logs, n_pairs), n_total, SCREEN_COLS)
        cols["v1"] = np.empty(n_total, np.int32)
        return cols

    def _route_pairs(self, res, routed, lsoa, pairs) -> None:
        """The pairs a screen sent back (counts -2) through compose(lsoa.pair(i, j)), keeping
        their conflicts alone; `last` stays the screen's."""
        if routed:
            # (copies: the columns may be views of the staging area that compose() packs into)
            self._compose_routed(res, routed, [lsoa.pair(int(pairs[p, 0]), int(pairs[p, 1])) for p in routed], "pair")
            for p in routed:
                res[p] = res[p][4]

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
        t0 = time.perf_counter()
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        P, L, tot = len(pairs), lsoa.n_logs, int(lsoa.n_total)
        self.last = _last(_SCREEN_KEYS + (("large",) if large else ()))
        flags = _abi.SCREEN_LARGE if large else 0
        if P == 0:
            return []
        bad = np.flatnonzero(((pairs < 0) | (pairs >= L)).any(axis=1))
        if len(bad):
            raise SmxError(-1, f"pair {int(bad[0])}: a log index outside [0, {L})")
        log_off = np.ascontiguousarray(lsoa.log_off, dtype=np.int64)
        ren = _rename_counts(lsoa.kind, log_off)
        conf_off = _conf_off(ren, pairs)
        lay = self._screen_layout(tot, L, P, int(conf_off[-1]))
        t1, t2 = self._staged_call(
            self.main, lib().smx_screen_ex_workspace_bytes, (L, tot, P, flags), lay,
            [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in SCREEN_COLS],
            (("log_off", log_off), ("pair_a", pairs[:, 0]), ("pair_b", pairs[:, 1]), ("conf_off", conf_off)),
            lambda d0, o0: _abi.SmxScreen(L, tot, P, d0 + lay["log_off"],
                                          *[d0 + lay[name] for name, _, _ in SCREEN_COLS],
                                          d0 + lay["pair_a"], d0 + lay["pair_b"], o0 + lay["conf"],
                                          d0 + lay["conf_off"], o0 + lay["counts"], 0),
            lambda arg, ws, nbytes, st: lib().smx_screen_ex(arg, ws, nbytes, flags, st))
        res = screen_results(self.main.hout, lay["conf"], lay["counts"], conf_off, pairs)
        routed = [p for p in range(P) if res[p] is None]
        self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2,
                          in_bytes=lay["in_bytes"], out_bytes=lay["out_bytes"], routed=len(routed))
        if large:
            self.last["large"] = _over_limit(ren, pairs)
        self._route_pairs(res, routed, lsoa, pairs)
        return res

    # -- the screen of merge trains (smx_screen_train): the steps' conflicts from renames alone --

    def screen_trains(self, lsoa, trains):
        """Per train of `trains` (lists of log indices over a LogsSoA) what smx_screen_train leaves:
        (n_renames, landed, steps) -- the renames in the final accumulator, the number of steps that
        landed, and per step (the accumulator's renames after it, outcome, its conflicts as an
        (n, 2) int32 array of (A column index, B column index)).  The outcomes and the pairs are
        smx_compose_train's for the same trains, whatever the sizes: no step is sent back.  One
        host-to-device copy of the six columns (33 bytes per op, each log once), one
        smx_screen_train, one copy back, one stream sync.  Invalid input raises SmxError naming
        the train.  The results are copies.  `last` holds the call's legs, "in_bytes" and "out_bytes"."""
        t0 = time.perf_counter()
        R, L, tot = len(trains), lsoa.n_logs, int(lsoa.n_total)
        self.last = _last(("in_bytes", "out_bytes"))
        if R == 0:
            return []
        train_log, train_off, log_off = train_index(lsoa, trains)
        S = len(train_log)
        ren = _rename_counts(lsoa.kind, log_off)
        step_ren = ren[train_log] if S else np.zeros(0, np.int64)
        conf_off = np.concatenate([[0], np.cumsum(step_ren, dtype=np.int64)])  # (at most one conflict per rename of B)
        acc_off = np.concatenate([[0], np.cumsum(conf_off[train_off[1:]] - conf_off[train_off[:-1]], dtype=np.int64)])
        n_acc, n_conf = int(acc_off[-1]), int(conf_off[-1])
        lay = self._layout(tot, [(name, tot * dt.itemsize) for name, dt, _ in SCREEN_COLS]
                           + [("log_off", (L + 1) * 8), ("train_off", (R + 1) * 8), ("train_log", S * 4),
                              ("acc_off", (R + 1) * 8), ("conf_off", (S + 1) * 8)], 0, 8 * n_conf, 16 * R)
        lay["step_counts"] = lay["counts"] + _al(16 * R)
        lay["out_bytes"] = lay["step_counts"] + 16 * S
        t1, t2 = self._staged_call(
            self.main, lib().smx_screen_train_workspace_bytes, (L, tot, R, S, n_acc, 0), lay,
            [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in SCREEN_COLS],
            (("log_off", log_off), ("train_off", train_off), ("train_log", train_log), ("acc_off", acc_off),
             ("conf_off", conf_off)),
            lambda d0, o0: _abi.SmxScreenTrain(L, tot, R, S, n_acc, d0 + lay["log_off"],
                                               *[d0 + lay[name] for name, _, _ in SCREEN_COLS],
                                               d0 + lay["train_off"], d0 + lay["train_log"], d0 + lay["acc_off"],
                                               o0 + lay["conf"], d0 + lay["conf_off"], o0 + lay["counts"],
                                               o0 + lay["step_counts"], 0),
            lambda arg, ws, nbytes, st: lib().smx_screen_train(arg, ws, nbytes, 0, st))
        hout = self.main.hout
        counts = hout[lay["counts"]: lay["counts"] + 16 * R].view(np.int64).tolist()
        sc = hout[lay["step_counts"]: lay["step_counts"] + 16 * S].view(np.int64).tolist()
        conf = hout[lay["conf"]: lay["conf"] + 8 * n_conf].view(np.int32).reshape(-1, 2)
        res = []
        for r in range(R):
            if counts[2 * r] < 0:
                raise SmxError(-1, f"train {r}: invalid input")
            steps = []
            for g in range(int(train_off[r]), int(train_off[r + 1])):
                oc, c = sc[2 * g + 1], int(conf_off[g])
                if oc < 0:
                    raise SmxError(-1, f"train {r}, step {g - int(train_off[r])}: invalid input: kind >= 18")
                steps.append((sc[2 * g], oc, conf[c: c + oc].copy()))
            res.append((counts[2 * r], counts[2 * r + 1], steps))
        self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2,
                          in_bytes=lay["in_bytes"], out_bytes=lay["out_bytes"])
        return res

    # -- the screen of trains that share prefixes (smx_screen_tree): every node screened once -----

    def screen_tree(self, lsoa, parents, node_log):
        """Per node of a tree over a LogsSoA what smx_screen_tree leaves, in the caller's order:
        (renames, outcome, pairs) -- the renames in the accumulator after the node, its conflicts
        (0: it landed) and its conflict records as an (n, 2) int32 array of (A column index, B
        column index).  parents[n]: the node's parent (None or -1: a root; a parent precedes its
        children, tree_levels), node_log[n]: its log.  Per node they are smx_screen_train's last
        step on the node's root path, whatever the sizes: no node is sent back.  One
        host-to-device copy of the six columns (33 bytes per op, each log once), one
        smx_screen_tree, one copy back, one stream sync, whatever the tree.  Invalid input raises
        SmxError naming the node.  The results are copies.  `last` holds the call's legs,
        "in_bytes" and "out_bytes"."""
        t0 = time.perf_counter()
        order, level_off, back = tree_levels(parents)
        N, D, L, tot = len(order), len(level_off) - 1, lsoa.n_logs, int(lsoa.n_total)
        self.last = _last(("in_bytes", "out_bytes"))
        if N == 0:
            return []
        lv_par, lv_log, log_off = tree_index(lsoa, parents, node_log, order, level_off, back)
        lv_ren = _rename_counts(lsoa.kind, log_off)[lv_log].astype(np.int64)
        acc_off = np.concatenate([[0], np.cumsum(tree_room(lv_par, lv_ren), dtype=np.int64)])
        conf_off = np.concatenate([[0], np.cumsum(lv_ren, dtype=np.int64)])  # (at most one conflict per rename of B)
        n_acc, n_conf = int(acc_off[-1]), int(conf_off[-1])
        if n_acc > 0x7fffffff:
            raise SmxError(-1, f"the nodes' accumulators need {n_acc} rename records: over 2^31 - 1")
        lay = self._layout(tot, [(name, tot * dt.itemsize) for name, dt, _ in SCREEN_COLS]
                           + [("log_off", (L + 1) * 8), ("level_off", (D + 1) * 8), ("node_parent", N * 4),
                              ("node_log", N * 4), ("acc_off", (N + 1) * 8), ("conf_off", (N + 1) * 8)],
                           0, 8 * n_conf, 16 * N)
        t1, t2 = self._staged_call(
            self.main, lib().smx_screen_tree_workspace_bytes, (L, tot, N, D, n_acc, 0), lay,
            [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in SCREEN_COLS],
            (("log_off", log_off), ("level_off", level_off), ("node_parent", lv_par), ("node_log", lv_log),
             ("acc_off", acc_off), ("conf_off", conf_off)),
            lambda d0, o0: _abi.SmxScreenTree(L, tot, N, D, n_acc, d0 + lay["log_off"],
                                              *[d0 + lay[name] for name, _, _ in SCREEN_COLS],
                                              d0 + lay["level_off"], d0 + lay["node_parent"], d0 + lay["node_log"],
                                              d0 + lay["acc_off"], o0 + lay["conf"], d0 + lay["conf_off"],
                                              o0 + lay["counts"], 0),
            lambda arg, ws, nbytes, st: lib().smx_screen_tree(arg, ws, nbytes, 0, st))
        hout = self.main.hout
        counts = hout[lay["counts"]: lay["counts"] + 16 * N].view(np.int64).tolist()
        conf = hout[lay["conf"]: lay["conf"] + 8 * n_conf].view(np.int32).reshape(-1, 2)
        res = [None] * N
        for i in range(N):
            n, k, oc = int(order[i]), counts[2 * i], counts[2 * i + 1]
            if k < 0:
                raise SmxError(-1, f"node {n}: invalid input")
            if oc < 0:
                raise SmxError(-1, f"node {n}: invalid input: kind >= 18")
            c = int(conf_off[i])
            res[n] = (k, oc, conf[c: c + oc].copy())
        self.last = _last(pack_s=t1 - t0, device_s=t2 - t1, unpack_s=time.perf_counter() - t2,
                          in_bytes=lay["in_bytes"], out_bytes=lay["out_bytes"])
        return res

    # -- candidate pairs (smx_screen_candidates) and the screen of all of them ----------------

    @staticmethod
    def _cand_layout(n_total: int, n_logs: int, cap: int, cols):
        """Byte offsets of a candidates call in the staging areas.  In: the columns `cols`
        (rows of OP_COLS) for n_total ops, then log_off (the six columns lie as
        _screen_layout has them).  Out: the two counts, log_info, then pair_a and pair_b of
        `cap` entries."""
        lay = ComposeSession._layout(n_total, [(name, n_total * dt.itemsize) for name, dt, _ in cols]
                                     + [("log_off", (n_logs + 1) * 8)], 0, 0, 0)
        lay["counts"], lay["log_info"], lay["pair_a"] = 0, 256, 256 + _al(4 * n_logs)
        lay["pair_b"] = lay["pair_a"] + _al(4 * cap)
        lay["out_bytes"] = lay["pair_b"] + _al(4 * cap)
        return lay

    def _candidates(self, lsoa, cols, start_cap: Optional[int]):
        """smx_screen_candidates on the columns `cols` of a LogsSoA, staged once: one copy in,
        one call, one copy back, one sync; once more with the exact count when the
        candidates exceed the starting capacity (the columns are copied again only if the
        input staging area had to be replaced for it).  Returns the (n, 2) pairs (a view of
        the output staging area), every log's rename count and the layout; `last` is set."""
        t0 = time.perf_counter()
        L, tot = lsoa.n_logs, int(lsoa.n_total)
        if L > _abi.CAND_MAX_LOGS:
            raise SmxError(-1, f"{L} logs exceed the {_abi.CAND_MAX_LOGS} of one candidates call")
        log_off = np.ascontiguousarray(lsoa.log_off, dtype=np.int64)
        full = L * (L - 1) // 2
        cap = max(min(full, max(8 * L, 1024) if start_cap is None else start_cap), 1)
        m = self.main
        retries, in_bytes, out_bytes, staged, t1 = 0, 0, 0, None, t0
        while True:
            lay = self._cand_layout(tot, L, cap, cols)
            t_packed, _ = self._staged_call(
                m, lib().smx_screen_candidates_workspace_bytes, (L, tot), lay,
                [(getattr(lsoa, name), lay[name], tot * dt.itemsize) for name, dt, _ in cols], (("log_off", log_off),),
                lambda d0, o0: _abi.SmxCandidates(L, tot, d0 + lay["log_off"], d0 + lay["kind"], d0 + lay["sym"],
                                                  d0 + lay["v0"], o0 + lay["pair_a"], o0 + lay["pair_b"], cap,
                                                  o0 + lay["counts"], o0 + lay["log_info"], 0),
                lib().smx_screen_candidates, staged=staged)
            if t_packed is not None:  # (the columns went in: for the first time, or the input area was replaced)
                staged, t1, in_bytes = m.d_in.data_ptr(), t_packed, in_bytes + lay["in_bytes"]
            out_bytes += lay["out_bytes"]
            hout = m.hout
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
        self.last = _last(_CAND_KEYS, pack_s=t1 - t0, device_s=t2 - t1, in_bytes=in_bytes, out_bytes=out_bytes,
                          n_candidates=n_cand, retries=retries)
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
            self.last = _last(_CAND_KEYS)
            return np.zeros((0, 2), np.int32)
        return self._candidates(lsoa, CAND_COLS, start_cap)[0]

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
        flags = _abi.SCREEN_LARGE if large else 0
        if lsoa.n_logs == 0:
            self.last = _last(_CAND_KEYS + (("large",) if large else ()))
            return np.zeros((0, 2), np.int32), []
        pairs, ren, lay = self._candidates(lsoa, SCREEN_COLS, start_cap)
        pairs = pairs.copy()
        last = self.last
        if large:
            last["large"] = _over_limit(ren, pairs)
        t0 = time.perf_counter()
        P, L, tot = len(pairs), lsoa.n_logs, int(lsoa.n_total)
        if P == 0:
            return pairs, []
        conf_off = _conf_off(ren, pairs)
        # the second call's own bytes go through the auxiliary areas: conf_off in, conflict pairs and counts out
        counts_at = _al(8 * int(conf_off[-1]) + 8)
        lay2 = {"conf_off": 0, "in_bytes": conf_off.nbytes, "out_bytes": counts_at + 8 * P}
        d0, o0 = self.main.d_in.data_ptr(), self.main.d_out.data_ptr()
        t1, t2 = self._staged_call(
            self.aux, lib().smx_screen_ex_workspace_bytes, (L, tot, P, flags), lay2, (), (("conf_off", conf_off),),
            lambda c0, x0: _abi.SmxScreen(L, tot, P, d0 + lay["log_off"],
                                          *[d0 + lay[name] for name, _, _ in SCREEN_COLS],
                                          o0 + lay["pair_a"], o0 + lay["pair_b"], x0, c0, x0 + counts_at, 0),
            lambda arg, ws, nbytes, st: lib().smx_screen_ex(arg, ws, nbytes, flags, st))
        res = screen_results(self.aux.hout, 0, counts_at, conf_off, pairs)
        routed = [p for p in range(P) if res[p] is None]
        self.last = _last(pack_s=last["pack_s"] + t1 - t0, device_s=last["device_s"] + t2 - t1,
                          unpack_s=time.perf_counter() - t2, in_bytes=last["in_bytes"] + lay2["in_bytes"],
                          out_bytes=last["out_bytes"] + lay2["out_bytes"], n_candidates=P,
                          retries=last["retries"], routed=len(routed))
        if large:
            self.last["large"] = last["large"]
        self._route_pairs(res, routed, lsoa, pairs)
        return pairs, res


_sessions = {}


def session(device: str = "cuda") -> ComposeSession:
    """The calling thread's ComposeSession on `device`."""
    key = (threading.get_ident(), str(device))
    if key not in _sessions:
        _sessions[key] = ComposeSession(device)
    return _sessions[key]


def _free_session(device: str) -> ComposeSession:
    """The calling thread's session, or a fresh one while a drop-in merge of this thread holds it (busy)."""
    s = session(device)
    return s if not s.busy else ComposeSession(device)


class dropin_session:
    """The thread's session for one drop-in merge whose results are read as views of its
    staging area (marshal into it, compose, materialise): marked busy meanwhile, so that a
    merge started from inside that materialise -- a caller's Op class or deepcopy hook
    composing again -- gets buffers of its own instead of overwriting the views."""

    def __init__(self, device: str = "cuda") -> None:
        self.device = device

    def __enter__(self) -> ComposeSession:
        self.s = _free_session(self.device)
        self.s.busy = True
        return self.s

    def __exit__(self, *exc) -> None:
        self.s.busy = False


def compose_soa(soa: SoA, device: str = "cuda"):
    """ComposeSession.compose on the thread's free session: one merge, computed on the GPU."""
    return _free_session(device).compose(soa)


def compose_soa_many(soas, device: str = "cuda", large: bool = False, large_max: Optional[int] = None):
    """ComposeSession.compose_many on the thread's free session: independent merges in one batch."""
    return _free_session(device).compose_many(soas, large=large, large_max=large_max)


def compose_soa_shared(ssoa, shared_is_b: bool = False, device: str = "cuda", large: bool = False,
                       large_max: Optional[int] = None):
    """ComposeSession.compose_shared on the thread's free session: a SharedSoA's merges in one batch."""
    return _free_session(device).compose_shared(ssoa, shared_is_b, large=large, large_max=large_max)


def compose_pairs_soa(lsoa, pairs, device: str = "cuda", large: bool = False, large_max: Optional[int] = None):
    """ComposeSession.compose_pairs on the thread's free session: the (i, j) of `pairs` over a LogsSoA in one batch."""
    return _free_session(device).compose_pairs(lsoa, pairs, large=large, large_max=large_max)


def compose_trains_soa(lsoa, trains, device: str = "cuda", v1_alt=None, empty_str: int = -1):
    """ComposeSession.compose_trains on the thread's free session: the trains over a LogsSoA in one call."""
    return _free_session(device).compose_trains(lsoa, trains, v1_alt=v1_alt, empty_str=empty_str)


def compose_tree_soa(lsoa, parents, node_log, device: str = "cuda", v1_alt=None, empty_str: int = -1):
    """ComposeSession.compose_tree on the thread's free session: a tree of logs over a LogsSoA in one call."""
    return _free_session(device).compose_tree(lsoa, parents, node_log, v1_alt=v1_alt, empty_str=empty_str)


def screen_soa(lsoa, pairs, device: str = "cuda", large: bool = False):
    """ComposeSession.screen on the thread's free session: [conflict_pairs] of the (i, j) of `pairs`."""
    return _free_session(device).screen(lsoa, pairs, large=large)


def screen_all_soa(lsoa, device: str = "cuda", large: bool = False):
    """ComposeSession.screen_all on the thread's free session: (pairs, [conflict_pairs])."""
    return _free_session(device).screen_all(lsoa, large=large)


def screen_trains_soa(lsoa, trains, device: str = "cuda"):
    """ComposeSession.screen_trains on the thread's free session: the trains' steps screened in one call."""
    return _free_session(device).screen_trains(lsoa, trains)


def screen_tree_soa(lsoa, parents, node_log, device: str = "cuda"):
    """ComposeSession.screen_tree on the thread's free session: a tree's nodes screened in one call."""
    return _free_session(device).screen_tree(lsoa, parents, node_log)
