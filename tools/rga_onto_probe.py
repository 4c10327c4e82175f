"""Many event streams replayed onto base lists: crdt.replay_onto (smx_rga_replay_onto, every
base stored once) against the form available without it, crdt.replay with each base's events
repeated in front of every stream that uses it.

    python tools/rga_onto_probe.py [--bases 64,1,4] [--base-len 150,400,600] [--jobs-per-base 64,4096,8]
                                   [--own-len 40,40,100] [--reps 5] [--out profiles/rga_onto/rga_onto_probe.json]

The four lists are read together, one shape per position: --bases base lists of --base-len
events, each named by --jobs-per-base jobs of --own-len own events (Key / string events; own
moves and deletes reach into the base's values).  Per shape, after a warm-up of both forms and a
comparison of their results, alternating the two forms --reps times, the legs of each:
  marshal   the events to columns on the host (marshal_onto / marshal_streams)
  copy_in   the columns (and the offsets) to the device, to the synchronise behind the copies
  device    the library call on the resident columns, between device events on its stream
            (call: the host's time in it, which ends with its error read-back and stream wait)
  unpack    the results to the host and to Python lists of values
each as the median of its repetitions with their minimum and maximum, and the input bytes each
form copies in.  Prints one JSON document and writes it to --out.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", default="64,1,4")
    ap.add_argument("--base-len", default="150,400,600")
    ap.add_argument("--jobs-per-base", default="64,4096,8")
    ap.add_argument("--own-len", default="40,40,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _abi, crdt
    from semantic_merge_amd._lib import check, lib

    ints = lambda s: [int(x) for x in s.split(",")]
    shapes = list(zip(ints(a.bases), ints(a.base_len), ints(a.jobs_per_base), ints(a.own_len)))
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

    def legs_onto(bases, jobs):
        t0 = time.perf_counter()
        b = crdt.marshal_onto(bases, jobs)
        t1 = time.perf_counter()
        arrays = [(b.base_off, np.int64), (b.own_off, np.int64), (b.job_base, np.int32), (b.op, np.uint8),
                  (b.value, np.int32), (b.anchor, np.int32), (b.t, np.int64), (b.author, np.int32),
                  (b.opid_hi, np.int64), (b.opid_lo, np.int64)]
        ins = up(arrays)
        t2 = time.perf_counter()
        n_out = b.n_out
        vals, src, offs, counts = outputs(n_out, b.n_jobs)
        need = C.c_size_t(0)
        check(L.smx_rga_replay_onto_workspace_bytes(b.n_jobs, n_out, C.byref(need)))
        ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        q = _abi.SmxRgaOnto(b.n, b.n_bases, b.n_jobs, n_out, *[t.data_ptr() for t in ins])
        out = _abi.SmxRgaOut(vals.data_ptr(), src.data_ptr(), offs.data_ptr(), counts.data_ptr(), None)
        torch.cuda.synchronize(dev)
        d_ms, c_ms = device_call(lambda: check(L.smx_rga_replay_onto(C.byref(q), C.byref(out), ws.data_ptr(),
                                                                    need.value, st.cuda_stream)))
        t3 = time.perf_counter()
        res = unpack(b.values, vals, src, offs, counts, b.n_jobs)
        t4 = time.perf_counter()
        return res, {"marshal": 1e3 * (t1 - t0), "copy_in": 1e3 * (t2 - t1), "device": d_ms, "call": c_ms,
                     "unpack": 1e3 * (t4 - t3), "in_bytes": sum(int(x.nbytes) for x, _ in arrays),
                     "events": b.n, "workspace_bytes": need.value}

    def legs_repeated(bases, jobs):
        t0 = time.perf_counter()
        b = crdt.marshal_streams([(bases[i] if i is not None else []) + list(own) for i, own in jobs])
        t1 = time.perf_counter()
        arrays = [(b.list_id, np.int32), (b.op, np.uint8), (b.value, np.int32), (b.anchor, np.int32),
                  (b.t, np.int64), (b.author, np.int32), (b.opid_hi, np.int64), (b.opid_lo, np.int64)]
        ins = up(arrays)
        t2 = time.perf_counter()
        vals, src, offs, counts = outputs(b.n, b.n_lists)
        need = C.c_size_t(0)
        check(L.smx_rga_workspace_bytes(b.n, b.n_lists, C.byref(need)))
        ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        ops = _abi.SmxRgaOps(b.n, b.n_lists, *[t.data_ptr() for t in ins])
        out = _abi.SmxRgaOut(vals.data_ptr(), src.data_ptr(), offs.data_ptr(), counts.data_ptr(), None)
        torch.cuda.synchronize(dev)
        d_ms, c_ms = device_call(lambda: check(L.smx_rga_replay_ex(C.byref(ops), C.byref(out), ws.data_ptr(),
                                                                  need.value, _abi.RGA_GROUPED, st.cuda_stream)))
        t3 = time.perf_counter()
        res = unpack(b.values, vals, src, offs, counts, b.n_lists)
        t4 = time.perf_counter()
        return res, {"marshal": 1e3 * (t1 - t0), "copy_in": 1e3 * (t2 - t1), "device": d_ms, "call": c_ms,
                     "unpack": 1e3 * (t4 - t3), "in_bytes": sum(int(x.nbytes) for x, _ in arrays),
                     "events": b.n, "workspace_bytes": need.value}

    rows = []
    for n_bases, base_len, per_base, own_len in shapes:
        rng = random.Random(n_bases * 1_000_003 + base_len * 1009 + per_base * 31 + own_len)
        bases, jobs = [], []
        for i in range(n_bases):
            values = ["b%d.v%d" % (i, k) for k in range(max(base_len // 6, 2))]
            bases.append(make_events(rng, base_len, values, crdt.Key))
            jobs += [(i, make_events(rng, own_len, values, crdt.Key)) for _ in range(per_base)]
        rng.shuffle(jobs)
        got, _ = legs_onto(bases, jobs)       # (the warm-up, and the comparison)
        want, _ = legs_repeated(bases, jobs)
        if got != want:
            raise SystemExit(f"replay_onto and the repeated replay differ at {(n_bases, base_len, per_base, own_len)}")
        lo, lr = [], []
        for _ in range(a.reps):   # alternate the two forms
            lo.append(legs_onto(bases, jobs)[1])
            lr.append(legs_repeated(bases, jobs)[1])

        def legs(rs):
            return {k: (stats([r[k] for r in rs]) if k not in ("in_bytes", "events", "workspace_bytes") else int(rs[0][k]))
                    for k in rs[0]}

        n_jobs = len(jobs)
        row = {"bases": n_bases, "base_len": base_len, "jobs_per_base": per_base, "own_len": own_len, "jobs": n_jobs,
               "onto": legs(lo), "repeated": legs(lr),
               # 37 bytes of columns per event, + 4 of list id in the repeated form; the offsets and job_base
               "in_bytes_expected": {"onto": 37 * (n_bases * base_len + n_jobs * own_len)
                                     + 8 * (n_bases + 1) + 8 * (n_jobs + 1) + 4 * n_jobs,
                                     "repeated": 41 * n_jobs * (base_len + own_len)}}
        row["device_ratio_repeated_over_onto"] = round(row["repeated"]["device"]["median_ms"]
                                                       / row["onto"]["device"]["median_ms"], 3)
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
    line = json.dumps({"rga_onto_probe": rows, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
