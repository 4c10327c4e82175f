"""Shapes for smx_rga_replay_onto: bases stored once and jobs (base or None, own events) of
exact lengths, with tie-heavy keys from _rga_shapes' alphabets, and the expected results
from the CPU oracle on the expanded batch (list j = job j's base events, then its own).

Values come from one pool per base, shared by the base and by the own streams of the jobs
that name it, so own moves and deletes reach into the base's elements.  On top of the random
events a few are planted, so that the coverage conditions of tests/test_gpu_rga_onto.py hold
by construction where the lengths allow them (`coverage` checks them on the oracle's output):
a base starts with up to three inserts of values that no random event uses (v0, v1, v2, keys
k0, k1, k2), and a job with a base and at least three own events starts with
  insert(k1 or k0, w)   the full key of a base-created element: it lands after that element
  delete(v0)            tombstones the base's first element
  move(v2 or v0, key)   a value live in the base's final state (v2: pops the base's element;
                        v0, for a base of one or two events: after the delete, pops nothing)
so the base's v1 element (v0's, tombstoned, for a base of one event) is still in the list."""
import ctypes as C

import numpy as np

from oracle import oracle
from semantic_merge_amd import _abi
from semantic_merge_amd.crdt import RgaBatch, RgaOntoBatch, job_columns

import _rga_shapes as shapes

OPS = shapes.OPS
PLANT_OWN = 3      # own events a job needs for the planted three
COVERED_OWN = 8    # own events from which a job with a base must meet the coverage conditions


def build(base_len, jobs, seed, regime, ops=OPS):
    """An RgaOntoBatch: base b has base_len[b] events, job j = (base or None, own length)."""
    rng = np.random.default_rng(seed)
    base_len = np.asarray(base_len, np.int64)
    nb, nj = base_len.size, len(jobs)
    job_base = np.asarray([-1 if b is None else b for b, _ in jobs], np.int32).reshape(nj)
    own_len = np.asarray([n for _, n in jobs], np.int64).reshape(nj)
    base_off = np.concatenate([[0], np.cumsum(base_len)]).astype(np.int64)
    own_off = base_off[-1] + np.concatenate([[0], np.cumsum(own_len)]).astype(np.int64)
    n = int(own_off[-1])
    # the value pool of every column: the base's, or a job's own when it has no base
    pool = np.concatenate([np.repeat(np.arange(nb), base_len),
                           np.repeat(np.where(job_base >= 0, job_base, nb + np.arange(nj)), own_len)]).astype(np.int64)
    size = np.concatenate([base_len, own_len])  # (a pool's size: its base's, or the job's own)
    nv = np.maximum(size // 6, 2)
    anchors, ts = shapes.REGIMES[regime]
    one = regime == "one_key"
    pick = lambda alphabet, dt, k=n: np.asarray(alphabet, dt)[rng.integers(0, len(alphabet), size=k)]
    op = rng.choice(3, size=n, p=np.asarray(ops, np.float64) / sum(ops)).astype(np.uint8)
    anchor, t = pick(anchors, np.uint32), pick(ts, np.int64)
    author = pick(shapes.AUTHORS[:1] if one else shapes.AUTHORS, np.uint32)
    hi = pick(shapes.OPID_HI[:1] if one else shapes.OPID_HI, np.uint64)
    lo = pick(shapes.OPID_LO[:1] if one else shapes.OPID_LO, np.uint64)
    val = pool * (1 << 20) + rng.integers(0, 1 << 20, size=n) % nv[pool] if n else np.zeros(0, np.int64)
    planted = lambda b, k: (nb + nj) * (1 << 20) + 4 * b + k  # v0, v1, v2, w of base b
    keys = (anchor, t, author, hi, lo)
    for b in range(nb):  # the base's first events: inserts of v0, v1, v2
        for k in range(min(3, int(base_len[b]))):
            c = base_off[b] + k
            op[c], val[c] = 0, planted(b, k)
    for j in range(nj):
        b = int(job_base[j])
        if b < 0 or own_len[j] < PLANT_OWN or base_len[b] < 1:
            continue
        c, lb = int(own_off[j]), int(base_len[b])
        tie = base_off[b] + (1 if lb >= 2 else 0)  # the base element whose key the insert repeats
        op[c], val[c] = 0, planted(b, 3)
        for col in keys:
            col[c] = col[tie]
        op[c + 1], val[c + 1] = 2, planted(b, 0)
        op[c + 2], val[c + 2] = 1, planted(b, 2 if lb >= 3 else 0)
    _, inv = np.unique(val, return_inverse=True)
    return RgaOntoBatch(nb, nj, base_off, own_off, job_base, op, inv.astype(np.uint32), anchor, t, author, hi, lo, [])


def expand(batch):
    """(the RgaBatch whose list j is job j's base events followed by its own, the column index
    of each of its events)."""
    idx, starts = job_columns(batch)
    lid = np.repeat(np.arange(batch.n_jobs), np.diff(starts)).astype(np.uint32)
    b = RgaBatch(batch.n_jobs, lid, batch.op[idx], batch.value[idx], batch.anchor[idx], batch.t[idx],
                 batch.author[idx], batch.opid_hi[idx], batch.opid_lo[idx], [])
    return b, idx


def expected(batch):
    """(the expanded batch, its column indices, the oracle's list state of it in the expanded
    batch's own indices, the same state with src as column indices)."""
    b, idx = expand(batch)
    vals, src, offs, tomb = oracle.rga(*shapes.args(b), tombstones=True)
    return b, idx, (vals, src, offs, tomb), (vals, idx[src].astype(np.int32), offs, tomb)


def materialized(state):
    vals, src, offs, tomb = state
    live = np.concatenate([[0], np.cumsum(~tomb)])
    return vals[~tomb], src[~tomb], live[offs]


def base_states(batch):
    """The oracle's list state of every base replayed alone: (values, src as column indices,
    offsets, tombstones)."""
    n = int(batch.base_off[-1])
    lid = np.repeat(np.arange(batch.n_bases), np.diff(batch.base_off)).astype(np.uint32)
    cols = [c[:n] for c in (batch.op, batch.value, batch.anchor, batch.t, batch.author, batch.opid_hi, batch.opid_lo)]
    return oracle.rga(max(batch.n_bases, 1), lid, *cols, tombstones=True)


def coverage(batch, want, min_own=COVERED_OWN):
    """Asserts, on the oracle's output (`want`: the list states, src as column indices), that
    every job with a base and at least min_own own events has
      an own move whose value is live in its base's final state,
      an own delete that tombstones a base-created element (live in the base's final state),
      an own insert whose full key equals a base-created element's and that lands after it,
      a base-created element still in its list: a live one when the base has two events or more.
    Returns the number of jobs checked."""
    vals, src, offs, tomb = want
    bv, bs, bo, bt = base_states(batch)
    key = np.stack([batch.anchor.astype(np.uint64), batch.t.view(np.uint64), batch.author.astype(np.uint64),
                    batch.opid_hi, batch.opid_lo], axis=1)
    n_checked = 0
    for j in range(batch.n_jobs):
        b = int(batch.job_base[j])
        o0, o1 = int(batch.own_off[j]), int(batch.own_off[j + 1])
        if b < 0 or o1 - o0 < min_own:
            continue
        n_checked += 1
        b0, b1 = int(batch.base_off[b]), int(batch.base_off[b + 1])
        live_in_base = set(bv[bo[b]:bo[b + 1]][~bt[bo[b]:bo[b + 1]]].tolist())
        own_op, own_val = batch.op[o0:o1], batch.value[o0:o1]
        assert live_in_base & set(own_val[own_op == 1].tolist()), f"job {j}: no own move of a live base value"
        s, tb, v = (a[offs[j]:offs[j + 1]] for a in (src, tomb, vals))
        from_base = (s >= b0) & (s < b1)
        live_before = np.isin(s, bs[bo[b]:bo[b + 1]][~bt[bo[b]:bo[b + 1]]])
        hit = from_base & tb & live_before & np.isin(v, own_val[own_op == 2])
        assert hit.any(), f"job {j}: no own delete tombstones a base-created element"
        assert from_base.any() and (b1 - b0 < 2 or (from_base & ~tb).any()), f"job {j}: no base-created element left"
        own_ins = np.flatnonzero((s >= o0) & (batch.op[s] == 0))
        base_pos = np.flatnonzero(from_base)
        tied = [p for p in own_ins.tolist()
                if (base_pos < p).any() and (key[s[base_pos[base_pos < p]]] == key[s[p]]).all(axis=1).any()]
        assert tied, f"job {j}: no own insert ties with a base-created element"
    return n_checked


# ---- the C ABI, on device buffers the caller keeps (a workspace shared between calls) ----

def workspace_bytes(lib, n_jobs, n_out):
    size = C.c_size_t(0)
    assert lib.smx_rga_replay_onto_workspace_bytes(n_jobs, n_out, C.byref(size)) == 0, lib.smx_last_error()
    return size.value


def run_onto(lib, batch, tombstones, ws, n_out=None, device="cuda"):
    """smx_rga_replay_onto on `batch` with the workspace tensor `ws`: (return code, results or
    None); the results as _lib.rga_replay_onto_device returns them."""
    import torch
    dev = torch.device(device)
    n_out = batch.n_out if n_out is None else n_out
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    ins = [up(batch.base_off, np.int64), up(batch.own_off, np.int64), up(batch.job_base, np.int32),
           up(batch.op, np.uint8), up(batch.value, np.int32), up(batch.anchor, np.int32), up(batch.t, np.int64),
           up(batch.author, np.int32), up(batch.opid_hi, np.int64), up(batch.opid_lo, np.int64)]
    cap = max(n_out, 1)
    vals, src = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    offs = torch.empty(batch.n_jobs + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    tomb = torch.empty(cap, dtype=torch.uint8, device=dev) if tombstones else None
    onto = _abi.SmxRgaOnto(batch.n, batch.n_bases, batch.n_jobs, n_out, *[t.data_ptr() for t in ins])
    out = _abi.SmxRgaOut(vals.data_ptr(), src.data_ptr(), offs.data_ptr(), counts.data_ptr(),
                         tomb.data_ptr() if tombstones else None)
    rc = lib.smx_rga_replay_onto(C.byref(onto), C.byref(out), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    if rc != 0:
        return rc, None
    k = int(counts.item())
    res = (vals[:k].cpu().numpy().view(np.uint32), src[:k].cpu().numpy(), offs.cpu().numpy())
    return rc, res + (tomb[:k].cpu().numpy().astype(np.bool_),) if tombstones else res


def run_replay_ex(lib, b, tombstones, ws, flags=0, device="cuda"):
    """smx_rga_replay_ex on the RgaBatch `b` with the workspace tensor `ws`: its results."""
    import torch
    dev = torch.device(device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    ins = [up(b.list_id, np.int32), up(b.op, np.uint8), up(b.value, np.int32), up(b.anchor, np.int32),
           up(b.t, np.int64), up(b.author, np.int32), up(b.opid_hi, np.int64), up(b.opid_lo, np.int64)]
    vals, src = (torch.empty(b.n, dtype=torch.int32, device=dev) for _ in range(2))
    offs = torch.empty(b.n_lists + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    tomb = torch.empty(b.n, dtype=torch.uint8, device=dev) if tombstones else None
    ops = _abi.SmxRgaOps(b.n, b.n_lists, *[t.data_ptr() for t in ins])
    out = _abi.SmxRgaOut(vals.data_ptr(), src.data_ptr(), offs.data_ptr(), counts.data_ptr(),
                         tomb.data_ptr() if tombstones else None)
    rc = lib.smx_rga_replay_ex(C.byref(ops), C.byref(out), ws.data_ptr(), ws.numel(), flags,
                               torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, lib.smx_last_error()
    torch.cuda.synchronize(dev)
    k = int(counts.item())
    res = (vals[:k].cpu().numpy().view(np.uint32), src[:k].cpu().numpy(), offs.cpu().numpy())
    return res + (tomb[:k].cpu().numpy().astype(np.bool_),) if tombstones else res
