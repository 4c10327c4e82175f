"""All pairs of N logs: smx_compose_pairs (every log stored once) against smx_compose_batch on
the repeated layout (each pair's two logs in front of each other, once per pair).

    python tools/pairs_probe.py [--logs 8,32,64] [--min-ops 100] [--max-ops 500] [--reps 20]
                                [--wall-reps 5] [--out profiles/pairs/pairs_probe.json]

Per N: N logs of --min-ops to --max-ops ops as Op objects and all i < j pairs.  After a warm-up,
alternating in the same run:
  device   device events around one smx_compose_pairs and around one smx_compose_batch of the
           same pairs on device-resident columns (the batch call alone, no copies)
  wall     compose_pairs(logs) and compose_many([(logs[i], logs[j]) ...]) on the Op objects, and
           their legs timed step by step on the same session: marshal, compose (pack, copy in,
           batch call, copy back, sync) and materialise; the bytes copied in
each as the median of its repetitions with their minimum and maximum.  The two paths' results
are compared before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4),
            "max_ms": round(float(np.max(ms)), 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="8,32,64")
    ap.add_argument("--min-ops", type=int, default=100)
    ap.add_argument("--max-ops", type=int, default=500)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _lib, synth
    from semantic_merge_amd.compose import compose_many, compose_pairs
    from semantic_merge_amd.marshal import marshal_logs, marshal_native
    from semantic_merge_amd.materialize import materialize_conflicts, materialize_ops_native
    from semantic_merge_amd.ops import Op

    n_sym = 40
    kw = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)

    def ops_of(n, seed, side):
        d = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **kw)))[side]
        return [Op.from_dict(x) for x in d]

    st = torch.cuda.Stream()
    sess = _lib.ComposeSession()
    rows = []
    for N in [int(x) for x in a.logs.split(",")]:
        rng = np.random.default_rng(N)
        logs = [ops_of(int(n), 1000 + i, i % 2) for i, n in enumerate(rng.integers(a.min_ops, a.max_ops + 1, N))]
        ij = [(i, j) for i in range(N) for j in range(i + 1, N)]
        P = len(ij)
        op_pairs = [(logs[i], logs[j]) for i, j in ij]
        lsoa = marshal_logs(logs)
        dp = _lib.DevicePairs(lsoa, ij)
        dr = _lib.DeviceBatch([lsoa.pair(i, j) for i, j in ij], n_sym=lsoa.n_sym)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        torch.cuda.synchronize()
        for _ in range(3):
            dp.run(st)
            dr.run(st)
        st.synchronize()
        same = all(all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(dp.results(), dr.results()))
        if not same:
            raise SystemExit(f"the pairs and the repeated layout differ at N={N}")
        tp_, tr_ = [], []
        per = max(a.reps // 5, 1)
        for _ in range(5):   # alternate the two paths
            tp_ += [timed(lambda: dp.run(st)) for _ in range(per)]
            tr_ += [timed(lambda: dr.run(st)) for _ in range(per)]

        def legs_pairs():
            t0 = time.perf_counter()
            s = marshal_logs(logs, sess.staging_pairs(sum(map(len, logs)), N, P))
            kind, off = s.kind.copy(), s.log_off.tolist()
            t1 = time.perf_counter()
            res = sess.compose_pairs(s, ij, copy=False)
            t2 = time.perf_counter()
            for (i, j), (order, addr, file, ctx, cp) in zip(ij, res):
                ops = logs[i] + logs[j]
                k = np.concatenate([kind[off[i]: off[i + 1]], kind[off[j]: off[j + 1]]])
                materialize_ops_native(ops, k, s.strings, order, addr, file, ctx)
                materialize_conflicts(ops, cp)
            t3 = time.perf_counter()
            return {"marshal": t1 - t0, "compose": t2 - t1, "copy_device": sess.last["device_s"],
                    "materialise": t3 - t2, "in_bytes": sess.last["in_bytes"]}

        def legs_many():
            t0 = time.perf_counter()
            ns = [len(x) + len(y) for x, y in op_pairs]
            cols = sess.staging_many(ns)
            ss = [marshal_native(x, y, c) for (x, y), c in zip(op_pairs, cols)]
            t1 = time.perf_counter()
            res = sess.compose_many(ss, copy=False)
            t2 = time.perf_counter()
            for (x, y), s, (order, addr, file, ctx, cp) in zip(op_pairs, ss, res):
                materialize_ops_native(x + y, s.kind, s.strings, order, addr, file, ctx)
                materialize_conflicts(x + y, cp)
            t3 = time.perf_counter()
            return {"marshal": t1 - t0, "compose": t2 - t1, "materialise": t3 - t2,
                    "in_bytes": sess._batch_layout(ns)["in_bytes"]}

        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return 1e3 * (time.perf_counter() - t0)

        got, want = compose_pairs(logs), compose_many(op_pairs)   # (also the warm-up)
        for (go, gc), (wo, wc) in zip(got[:64], want[:64]):
            if [o.to_dict() for o in go] != [o.to_dict() for o in wo] or len(gc) != len(wc):
                raise SystemExit(f"compose_pairs and compose_many differ at N={N}")
        legs_pairs(), legs_many()
        wp_, wm_, lp_, lm_ = [], [], [], []
        for _ in range(a.wall_reps):   # alternate the two paths
            wp_.append(wall(lambda: compose_pairs(logs)))
            wm_.append(wall(lambda: compose_many(op_pairs)))
            lp_.append(legs_pairs())
            lm_.append(legs_many())

        def legs(rows_):
            return {k: (stats([1e3 * r[k] for r in rows_]) if k != "in_bytes" else int(rows_[0][k])) for k in rows_[0]}

        p, r = stats(tp_), stats(tr_)
        n_total, n_rep = sum(map(len, logs)), sum(len(x) + len(y) for x, y in op_pairs)
        index = 8 * (N + 1) + 8 * P + 16 * (P + 1)
        row = {"logs": N, "pairs": P, "n_total": n_total, "ops_over_pairs": n_rep,
               "device": {"pairs": p, "repeated": r, "ratio": round(r["median_ms"] / p["median_ms"], 3)},
               "wall": {"compose_pairs": stats(wp_), "compose_many": stats(wm_),
                        "ratio": round(float(np.median(wm_) / np.median(wp_)), 3)},
               "legs": {"pairs": legs(lp_), "repeated": legs(lm_)},
               "in_bytes_expected": {"pairs": 37 * n_total + index, "repeated": 37 * n_rep + 8 * P + 16 * (P + 1)},
               "marshals_per_log": {"pairs": 1, "repeated": N - 1}}
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
    line = json.dumps({"pairs_probe": rows, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
