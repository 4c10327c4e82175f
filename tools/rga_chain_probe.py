"""Jobs that are runs of segments stored once: crdt.replay_chain (smx_rga_replay_chain) against
the best form available without it, crdt.replay_onto with a job's first segment as its base and
its remaining segments concatenated into its own stream, repeated per job.

    python tools/rga_chain_probe.py [--reps 5] [--out profiles/rga_chain/probe.json]

Shapes (Key / string events; moves and deletes reach into the values of a job's other segments):
  grid    the three-way reconcile: 64 bases, each with 8 targets and 8 pull requests (150 + 40 +
          40 events), job = base ++ target ++ pull request, 4096 jobs
  stack   64 stacks of 16 commits of 40 events, every prefix a job, 1024 jobs
  pair    the two-segment equivalence shape: 64 bases of 150 events, 64 own streams of 40 each;
          both forms store the same events, so the device legs compare the two calls alone
Per shape, after a warm-up of both forms and a comparison of their results, alternating the two
forms --reps times, the legs of each:
  marshal   the events to columns on the host (marshal_chain / marshal_onto)
  copy_in   the columns (and the tables) to the device, to the synchronise behind the copies
  device    the library call on the resident columns, between device events on its stream
            (call: the host's time in it, which ends with its error read-back and stream wait)
  unpack    the results to the host and to Python lists of values
each as the median of its repetitions with their minimum and maximum, the events each form
stores and the input bytes it copies in.  Prints one JSON document and writes it to --out.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FIXED = ("in_bytes", "events", "workspace_bytes", "launches")


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "reps": len(ms)}


def make_events(rng, n, values, Key):
    out = []
    for _ in range(n):
        kind = rng.choice((0, 0, 0, 1, 2))
        key = None if kind == 2 else Key(rng.choice(("", "imports", "members")), rng.randrange(1 << 40),
                                         rng.choice(("ann", "bob", "eve")), "%032x" % rng.getrandbits(128))
        out.append((kind, key, rng.choice(values)))
    return out


def shape_grid(rng, Key, n_bases=64, n_targets=8, n_prs=8, lens=(150, 40, 40)):
    values = [["f%d.v%d" % (i, k) for k in range(max(sum(lens) // 6, 2))] for i in range(n_bases)]
    bases = [make_events(rng, lens[0], values[i], Key) for i in range(n_bases)]
    targets = [make_events(rng, lens[1], values[i], Key) for i in range(n_bases) for _ in range(n_targets)]
    prs = [make_events(rng, lens[2], values[i], Key) for i in range(n_bases) for _ in range(n_prs)]
    nb, nt = len(bases), len(targets)
    jobs = [[i, nb + i * n_targets + t, nb + nt + i * n_prs + p]
            for i in range(n_bases) for t in range(n_targets) for p in range(n_prs)]
    return bases + targets + prs, jobs


def shape_stack(rng, Key, n_stacks=64, n_commits=16, n_events=40):
    segments, jobs = [], []
    for i in range(n_stacks):
        values = ["s%d.v%d" % (i, k) for k in range(max(n_commits * n_events // 6, 2))]
        first = len(segments)
        segments += [make_events(rng, n_events, values, Key) for _ in range(n_commits)]
        jobs += [list(range(first, first + k + 1)) for k in range(n_commits)]
    return segments, jobs


def shape_pair(rng, Key, n_bases=64, per_base=64, lens=(150, 40)):
    bases, owns, jobs = [], [], []
    for i in range(n_bases):
        values = ["b%d.v%d" % (i, k) for k in range(max(lens[0] // 6, 2))]
        bases.append(make_events(rng, lens[0], values, Key))
        owns += [make_events(rng, lens[1], values, Key) for _ in range(per_base)]
    jobs = [[j // per_base, n_bases + j] for j in range(len(owns))]
    return bases + owns, jobs


def as_onto(segments, jobs):
    """The same jobs for replay_onto: a job's first segment as its base (each such segment stored
    once), its remaining segments concatenated into its own stream."""
    base_of, bases, out = {}, [], []
    for job in jobs:
        if not job:
            out.append((None, []))
            continue
        if job[0] not in base_of:
            base_of[job[0]] = len(bases)
            bases.append(segments[job[0]])
        out.append((base_of[job[0]], [ev for s in job[1:] for ev in segments[s]]))
    return bases, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="grid,stack,pair")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _abi, crdt
    from semantic_merge_amd._lib import check, lib

    dev = torch.device("cuda")
    st = torch.cuda.current_stream(dev)
    L = lib()

    def up(arrays):
        ts = [torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev, non_blocking=False) for x, dt in arrays]
        torch.cuda.synchronize(dev)
        return ts

    def device_call(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1), 1e3 * (t1 - t0)

    def outputs(n_out, n_lists):
        vals, src = (torch.empty(max(n_out, 1), dtype=torch.int32, device=dev) for _ in range(2))
        offs = torch.empty(n_lists + 1, dtype=torch.int64, device=dev)
        counts = torch.zeros(1, dtype=torch.int64, device=dev)
        return vals, src, offs, counts

    def unpack(values, vals, src, offs, counts, n_lists):
        k = int(counts.item())
        srcl, offl = src[:k].cpu().tolist(), offs.cpu().tolist()
        return [[values[s] for s in srcl[offl[i]:offl[i + 1]]] for i in range(n_lists)]

    def columns(b):
        return [(b.op, np.uint8), (b.value, np.int32), (b.anchor, np.int32), (b.t, np.int64), (b.author, np.int32),
                (b.opid_hi, np.int64), (b.opid_lo, np.int64)]

    def legs(marshal, tables, struct, query, call, launches):
        """One run of a form: marshal() -> batch, tables(batch) -> the offset arrays, struct /
        query / call: the library's struct, workspace query and entry point."""
        t0 = time.perf_counter()
        b = marshal()
        t1 = time.perf_counter()
        arrays = tables(b) + columns(b)
        ins = up(arrays)
        t2 = time.perf_counter()
        n_out = b.n_out
        vals, src, offs, counts = outputs(n_out, b.n_jobs)
        need = C.c_size_t(0)
        check(query(b, n_out, C.byref(need)))
        ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        q = struct(b, n_out, [t.data_ptr() for t in ins])
        out = _abi.SmxRgaOut(vals.data_ptr(), src.data_ptr(), offs.data_ptr(), counts.data_ptr(), None)
        torch.cuda.synchronize(dev)
        d_ms, c_ms = device_call(lambda: check(call(C.byref(q), C.byref(out), ws.data_ptr(), need.value, st.cuda_stream)))
        t3 = time.perf_counter()
        res = unpack(b.values, vals, src, offs, counts, b.n_jobs)
        t4 = time.perf_counter()
        return res, {"marshal": 1e3 * (t1 - t0), "copy_in": 1e3 * (t2 - t1), "device": d_ms, "call": c_ms,
                     "unpack": 1e3 * (t4 - t3), "in_bytes": sum(int(x.nbytes) for x, _ in arrays),
                     "events": b.n, "workspace_bytes": need.value, "launches": launches(b)}

    def legs_chain(segments, jobs):
        return legs(lambda: crdt.marshal_chain(segments, jobs),
                    lambda b: [(b.seg_off, np.int64), (b.job_off, np.int64), (b.job_seg, np.int32)],
                    lambda b, n_out, p: _abi.SmxRgaChain(b.n, b.n_segs, b.n_jobs, b.n_links, n_out, *p),
                    lambda b, n_out, ref: L.smx_rga_replay_chain_workspace_bytes(b.n_jobs, b.n_links, n_out, ref),
                    L.smx_rga_replay_chain,
                    # check, the scan's three, fit, map; the three list kernels; the output stage
                    lambda b: 6 + 3 + (1 if b.n_jobs <= 65536 else 5))

    def legs_onto(bases, ojobs):
        return legs(lambda: crdt.marshal_onto(bases, ojobs),
                    lambda b: [(b.base_off, np.int64), (b.own_off, np.int64), (b.job_base, np.int32)],
                    lambda b, n_out, p: _abi.SmxRgaOnto(b.n, b.n_bases, b.n_jobs, n_out, *p),
                    lambda b, n_out, ref: L.smx_rga_replay_onto_workspace_bytes(b.n_jobs, n_out, ref),
                    L.smx_rga_replay_onto,
                    # jobs, the scan's three, fit; the three list kernels; the output stage
                    lambda b: 5 + 3 + (1 if b.n_jobs <= 65536 else 5))

    makers = {"grid": shape_grid, "stack": shape_stack, "pair": shape_pair}
    rows = []
    for name in a.shapes.split(","):
        rng = random.Random(sum(map(ord, name)) * 1_000_003)
        segments, jobs = makers[name](rng, crdt.Key)
        rng.shuffle(jobs)
        bases, ojobs = as_onto(segments, jobs)
        got, _ = legs_chain(segments, jobs)   # (the warm-up, and the comparison)
        want, _ = legs_onto(bases, ojobs)
        if got != want:
            raise SystemExit(f"replay_chain and replay_onto differ at {name}")
        lc, lo = [], []
        for _ in range(a.reps):   # alternate the two forms
            lc.append(legs_chain(segments, jobs)[1])
            lo.append(legs_onto(bases, ojobs)[1])

        def summary(rs):
            return {k: (stats([r[k] for r in rs]) if k not in FIXED else int(rs[0][k])) for k in rs[0]}

        n_links = sum(map(len, jobs))
        stored_onto = sum(map(len, bases)) + sum(len(own) for _, own in ojobs)
        row = {"shape": name, "segments": len(segments), "jobs": len(jobs), "links": n_links,
               "job_events": sum(len(segments[s]) for job in jobs for s in job),
               "chain": summary(lc), "onto": summary(lo),
               # from the layout: 37 bytes of columns per event stored, plus the tables
               "in_bytes_expected": {"chain": 37 * sum(map(len, segments)) + 8 * (len(segments) + 1)
                                     + 8 * (len(jobs) + 1) + 4 * n_links,
                                     "onto": 37 * stored_onto + 8 * (len(bases) + 1) + 8 * (len(jobs) + 1)
                                     + 4 * len(jobs)}}
        row["device_ratio_onto_over_chain"] = round(row["onto"]["device"]["median_ms"]
                                                    / row["chain"]["device"]["median_ms"], 3)
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
    line = json.dumps({"rga_chain_probe": rows, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
