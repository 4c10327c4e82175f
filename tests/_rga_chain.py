"""Shapes for smx_rga_replay_chain: segments stored once and jobs that are strictly ascending
runs of segment indices, with tie-heavy keys from _rga_shapes' alphabets, and the expected
results from the CPU oracle on the expanded batch (list j = job j's segments' events, one
segment after another).

Segments belong to families (the caller's choice: the segments that jobs combine).  Random
events draw their values from one pool per family, so moves and deletes reach across segments.
On top of them a few events are planted at a segment's start, with values that no random event
uses, so that the coverage conditions of tests/test_gpu_rga_chain.py hold by construction for
every job that `covered` names (`coverage` checks them on the oracle's output).  A segment s
cannot know which jobs it is the first or the last segment of, so the plants do not depend on
its place:
  level A (3 events or more):
    insert(KF, u_s)    KF: one full key per family, u_s a value of s alone that nothing else
                       touches: in any job it ties with the u of every earlier segment, lands
                       after them by creation index, and stays live
    delete(d_s)        d_s, m_s: values that only s deletes / moves ...
    move(m_s, key)
  level B (3 + 2 L events or more, L = the later segments of its family):
    insert(key, d_x), insert(key, m_x) for every later segment x of the family
                       ... and that every level-B segment before it has inserted
so in a job whose first segment is level B and whose last is level A, the last segment's delete
tombstones an element that the first created and that was live until then, and its move finds
its value live with an element that the first created."""
import ctypes as C

import numpy as np

from oracle import oracle
from semantic_merge_amd import _abi
from semantic_merge_amd.crdt import RgaBatch, RgaChainBatch, chain_columns

import _rga_shapes as shapes
from _rga_onto import materialized, run_onto, run_replay_ex  # noqa: F401  (shared with the onto tests)

OPS = shapes.OPS
PLANT_A = 3


def _tables(jobs):
    job_off = np.concatenate([[0], np.cumsum([len(j) for j in jobs])]).astype(np.int64)
    job_seg = np.asarray([s for j in jobs for s in j], np.int32).reshape(int(job_off[-1]))
    return job_off, job_seg


def levels(seg_len, family):
    """(level A, level B) per segment, from the lengths and the families alone."""
    seg_len, family = np.asarray(seg_len, np.int64), np.asarray(family, np.int64)
    later = np.zeros(seg_len.size, np.int64)  # the later segments of s's family
    for f in np.unique(family):
        idx = np.flatnonzero(family == f)
        later[idx] = np.arange(idx.size)[::-1]
    return seg_len >= PLANT_A, seg_len >= PLANT_A + 2 * later


def covered(seg_len, family, jobs):
    """The jobs that must meet the coverage conditions: three segments or more, the first of
    level B, the last of level A."""
    a, b = levels(seg_len, family)
    return [j for j, job in enumerate(jobs) if len(job) >= 3 and b[job[0]] and a[job[-1]]]


def build(seg_len, jobs, seed, regime, family=None, ops=OPS):
    """An RgaChainBatch: segment s has seg_len[s] events, job j is the list jobs[j] of segment
    indices; family[s] (default: one family) names the segments whose values meet."""
    rng = np.random.default_rng(seed)
    seg_len = np.asarray(seg_len, np.int64)
    ns = seg_len.size
    family = np.zeros(ns, np.int64) if family is None else np.asarray(family, np.int64)
    seg_off = np.concatenate([[0], np.cumsum(seg_len)]).astype(np.int64)
    job_off, job_seg = _tables(jobs)
    n = int(seg_off[-1])
    nf = int(family.max()) + 1 if ns else 0
    # values per family: by the longest job that touches it
    nv = np.full(max(nf, 1), 2, np.int64)
    for job in jobs:
        total = int(seg_len[list(job)].sum())
        for f in set(family[list(job)].tolist()):
            nv[f] = max(nv[f], total // 8)
    pool = np.repeat(family, seg_len)
    anchors, ts = shapes.REGIMES[regime]
    one = regime == "one_key"
    pick = lambda alphabet, dt: np.asarray(alphabet, dt)[rng.integers(0, len(alphabet), size=n)]
    op = rng.choice(3, size=n, p=np.asarray(ops, np.float64) / sum(ops)).astype(np.uint8)
    anchor, t = pick(anchors, np.uint32), pick(ts, np.int64)
    author = pick(shapes.AUTHORS[:1] if one else shapes.AUTHORS, np.uint32)
    hi = pick(shapes.OPID_HI[:1] if one else shapes.OPID_HI, np.uint64)
    lo = pick(shapes.OPID_LO[:1] if one else shapes.OPID_LO, np.uint64)
    val = pool * (1 << 20) + rng.integers(0, 1 << 20, size=n) % nv[pool] if n else np.zeros(0, np.int64)
    planted = lambda s, k: (nf + 1) * (1 << 20) + 3 * s + k  # u_s, d_s, m_s
    keys = (anchor, t, author, hi, lo)
    lev_a, lev_b = levels(seg_len, family)
    kf = {}  # family -> the column whose key is KF
    for s in range(ns):
        if not lev_a[s]:
            continue
        c = int(seg_off[s])
        tie = kf.setdefault(int(family[s]), c)
        op[c], val[c] = 0, planted(s, 0)
        for col in keys:
            col[c] = col[tie]
        op[c + 1], val[c + 1] = 2, planted(s, 1)
        op[c + 2], val[c + 2] = 1, planted(s, 2)
        if lev_b[s]:
            c += PLANT_A
            for x in np.flatnonzero((family == family[s]) & (np.arange(ns) > s)).tolist():
                op[c], val[c] = 0, planted(x, 1)
                op[c + 1], val[c + 1] = 0, planted(x, 2)
                c += 2
            assert c <= seg_off[s + 1]
    _, inv = np.unique(val, return_inverse=True)
    return RgaChainBatch(ns, len(jobs), seg_off, job_off, job_seg, op, inv.astype(np.uint32), anchor, t, author, hi,
                         lo, [])


def expand(batch):
    """(the RgaBatch whose list j is job j's segments' events, one segment after another; the
    column index of each of its events)."""
    idx, starts = chain_columns(batch)
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


def job_segments(batch, j):
    return batch.job_seg[int(batch.job_off[j]):int(batch.job_off[j + 1])].tolist()


def coverage(batch, want, which):
    """Asserts, on the oracle's output (`want`: the list states, src as column indices), that
    every job of `which` has
      an insert of a segment at place p >= 2 of the job whose full key equals that of an element
        created by a segment at a place <= p - 2, and that stands after it,
      a delete in its last segment that tombstones an element which its first segment created
        and which was live before the last segment,
      a move in its last segment of a value that was live before the last segment and has an
        element there that the first segment created,
      an element that its first segment created live at the end.
    Returns the number of jobs checked."""
    vals, src, offs, tomb = want
    which = list(which)
    # the same jobs without their last segments: the states before the last segment
    before = RgaChainBatch(batch.n_segs, len(which), batch.seg_off, *_tables([job_segments(batch, j)[:-1] for j in which]),
                           batch.op, batch.value, batch.anchor, batch.t, batch.author, batch.opid_hi, batch.opid_lo, [])
    bv, bs, bo, bt = expected(before)[3]
    key = np.stack([batch.anchor.astype(np.uint64), batch.t.view(np.uint64), batch.author.astype(np.uint64),
                    batch.opid_hi, batch.opid_lo], axis=1)
    seg_of = np.repeat(np.arange(batch.n_segs), np.diff(batch.seg_off))
    for i, j in enumerate(which):
        segs = job_segments(batch, j)
        assert len(segs) >= 3, f"job {j}"
        place = {s: p for p, s in enumerate(segs)}
        first, last = segs[0], segs[-1]
        l0, l1 = int(batch.seg_off[last]), int(batch.seg_off[last + 1])
        last_op, last_val = batch.op[l0:l1], batch.value[l0:l1]
        s, tb, v = (a[offs[j]:offs[j + 1]] for a in (src, tomb, vals))
        ps, pt, pv = (a[bo[i]:bo[i + 1]] for a in (bs, bt, bv))
        from_first = seg_of[s] == first
        assert (from_first & ~tb).any(), f"job {j}: no element of the first segment live at the end"
        live_before = ps[~pt]
        hit = from_first & tb & np.isin(s, live_before) & np.isin(v, last_val[last_op == 2])
        assert hit.any(), f"job {j}: no delete of the last segment tombstones a live element of the first"
        moved = set(last_val[last_op == 1].tolist())
        assert moved & set(pv[~pt & (seg_of[ps] == first)].tolist()), \
            f"job {j}: no move of the last segment finds a live value that the first created"
        pl = np.asarray([place[x] for x in seg_of[s].tolist()])
        tied = False
        for p in np.flatnonzero((pl >= 2) & (batch.op[s] == 0)).tolist():
            early = np.flatnonzero(pl[:p] <= pl[p] - 2)
            if early.size and (key[s[early]] == key[s[p]]).all(axis=1).any():
                tied = True
                break
        assert tied, f"job {j}: no insert ties with an element created two segments earlier"
    return len(which)


# ---- the C ABI, on device buffers the caller keeps (a workspace shared between calls) ----

def workspace_bytes(lib, n_jobs, n_links, n_out):
    size = C.c_size_t(0)
    assert lib.smx_rga_replay_chain_workspace_bytes(n_jobs, n_links, n_out, C.byref(size)) == 0, lib.smx_last_error()
    return size.value


def run_chain(lib, batch, tombstones, ws, n_out=None, device="cuda"):
    """smx_rga_replay_chain on `batch` with the workspace tensor `ws`: (return code, results or
    None); the results as _lib.rga_replay_chain_device returns them."""
    import torch
    dev = torch.device(device)
    n_out = batch.n_out if n_out is None else n_out
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    ins = [up(batch.seg_off, np.int64), up(batch.job_off, np.int64), up(batch.job_seg, np.int32),
           up(batch.op, np.uint8), up(batch.value, np.int32), up(batch.anchor, np.int32), up(batch.t, np.int64),
           up(batch.author, np.int32), up(batch.opid_hi, np.int64), up(batch.opid_lo, np.int64)]
    cap = max(n_out, 1)
    vals, src = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
    offs = torch.empty(batch.n_jobs + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    tomb = torch.empty(cap, dtype=torch.uint8, device=dev) if tombstones else None
    chain = _abi.SmxRgaChain(batch.n, batch.n_segs, batch.n_jobs, batch.n_links, n_out,
                             *[t.data_ptr() if t.numel() else None for t in ins])
    out = _abi.SmxRgaOut(vals.data_ptr(), src.data_ptr(), offs.data_ptr(), counts.data_ptr(),
                         tomb.data_ptr() if tombstones else None)
    rc = lib.smx_rga_replay_chain(C.byref(chain), C.byref(out), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    if rc != 0:
        return rc, None
    k = int(counts.item())
    res = (vals[:k].cpu().numpy().view(np.uint32), src[:k].cpu().numpy(), offs.cpu().numpy())
    return rc, res + (tomb[:k].cpu().numpy().astype(np.bool_),) if tombstones else res
