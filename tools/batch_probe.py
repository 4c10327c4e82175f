"""One smx_compose_batch against a loop of smx_compose calls, on device-resident inputs.

    python tools/batch_probe.py [--ops 1000,150] [--merges 1,16,256,1024,4096] [--reps 20]
                                [--loop-reps 5] [--out profiles/batch_probe.json]

Per (ops per merge, M): M synthetic merges of about that many ops (64 distinct ones, sizes
+-10 %, repeated) are uploaded once; then, alternating in the same run after a warm-up,
  batch_ms  one smx_compose_batch of the M merges, device events around the call
  loop_ms   M smx_compose calls on the same columns (each merge's slice; the path a caller
            without the batch takes: a launch, a stream sync and the verdict read per merge),
            device events around the loop
each as the median of its repetitions with their minimum and maximum.  The two paths'
counts are compared before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", default="1000,150")
    ap.add_argument("--merges", default="1,16,256,1024,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _abi, _lib, synth
    L = _lib.lib()
    st = torch.cuda.Stream()
    rows = []
    for n_ops in [int(x) for x in a.ops.split(",")]:
        rng = np.random.default_rng(n_ops)
        distinct = [synth.lift_soa(synth.lift_logs(synth.LiftSpec(int(n), max(int(n) // 100, 10), 1000 + i)))
                    for i, n in enumerate(rng.integers(n_ops - n_ops // 10, n_ops + n_ops // 10 + 1, 64))]
        for M in [int(x) for x in a.merges.split(",")]:
            soas = [distinct[i % len(distinct)] for i in range(M)]
            db = _lib.DeviceBatch(soas)
            # the loop's outputs and workspace: its own arrays, the batch's input columns
            lo = _lib.DeviceBatch(soas)
            ws = C.c_size_t(0)
            need = 0
            for s in distinct:
                _lib.check(L.smx_compose_workspace_bytes(s.n_a, s.n_b, s.n_sym, C.byref(ws)))
                need = max(need, ws.value)
            wst = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
            ins = [t.data_ptr() for t in db._in]
            widths = (1, 8, 8, 8, 4, 4, 4)
            calls = []
            for m, s in enumerate(soas):
                o, c = int(db.off[m]), int(db.conf_off[m])
                ops = _abi.SmxOps(s.n_a, s.n_b, s.n_sym, *[p + o * w for p, w in zip(ins, widths)], 0)
                out = _abi.SmxComposeOut(lo.order.data_ptr() + 4 * o, lo.addr.data_ptr() + 4 * o,
                                         lo.file.data_ptr() + 4 * o, lo.ctx.data_ptr() + 4 * o,
                                         lo.conf.data_ptr() + 8 * c, int(db.conf_off[m + 1]) - c,
                                         lo.counts.data_ptr() + 16 * m)
                calls.append((ops, out))

            def loop():
                for ops, out in calls:
                    _lib.check(L.smx_compose(C.byref(ops), C.byref(out), wst.data_ptr(), need, st.cuda_stream))

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1)

            torch.cuda.synchronize()
            for _ in range(3):
                db.run(st)
            loop()
            st.synchronize()
            same = np.array_equal(db.raw()["counts"], lo.raw()["counts"])
            same = same and all(all(np.array_equal(p, q) for p, q in zip(x, y))
                                for x, y in zip(db.results()[:64], lo.results()[:64]))
            if not same:
                raise SystemExit(f"batch and loop differ at ops={n_ops} M={M}")
            tb, tl = [], []
            per = max(a.reps // max(a.loop_reps, 1), 1)
            for _ in range(a.loop_reps):   # alternate the two paths
                tb += [timed(lambda: db.run(st)) for _ in range(per)]
                tl.append(timed(loop))
            b, l = stats(tb), stats(tl)
            row = {"ops_per_merge": n_ops, "merges": M, "total_ops": db.n_total, "batch": b, "loop": l,
                   "speedup": round(l["median_ms"] / b["median_ms"], 2),
                   "batch_us_per_merge": round(1e3 * b["median_ms"] / M, 3)}
            rows.append(row)
            print(row, file=sys.stderr, flush=True)
    line = json.dumps({"batch_probe": rows, "device": torch.cuda.get_device_name(0), "classes": list(_abi.BATCH_CLASSES)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
