"""One shared log against M branch logs: smx_compose_batch_shared (the shared log stored once)
against smx_compose_batch on the repeated layout (the shared log in front of every merge).

    python tools/shared_probe.py [--shared 900] [--own 100] [--merges 16,256,1024] [--reps 20]
                                 [--wall-reps 5] [--out profiles/shared/shared_probe.json]

Per M: a shared log of about --shared ops and M own logs of about --own ops (64 distinct ones,
sizes +-10 %, repeated), as Op objects.  After a warm-up, alternating in the same run:
  device   device events around one smx_compose_batch_shared and around one smx_compose_batch
           of the same merges on device-resident columns (the batch call alone, no copies)
  wall     compose_against(shared, branches) and compose_many([(shared, b) ...]) on the Op
           objects, and their legs timed step by step on the same session: marshal, compose
           (pack, copy in, batch call, copy back, sync) and materialise; the bytes copied in
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
    ap.add_argument("--shared", type=int, default=900)
    ap.add_argument("--own", type=int, default=100)
    ap.add_argument("--merges", default="16,256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _lib, synth
    from semantic_merge_amd.compose import compose_against, compose_many
    from semantic_merge_amd.marshal import marshal_native, marshal_shared
    from semantic_merge_amd.materialize import materialize_conflicts, materialize_ops_native
    from semantic_merge_amd.ops import Op

    n_sym = max(a.shared // 20, 10)
    kw = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)

    def ops_of(n, seed, side):
        d = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **kw)))[side]
        return [Op.from_dict(x) for x in d]

    shared = ops_of(a.shared, 1, 0)
    rng = np.random.default_rng(a.own)
    distinct = [ops_of(int(n), 1000 + i, 1)
                for i, n in enumerate(rng.integers(a.own - a.own // 10, a.own + a.own // 10 + 1, 64))]
    st = torch.cuda.Stream()
    sess = _lib.ComposeSession()
    rows = []
    for M in [int(x) for x in a.merges.split(",")]:
        branches = [distinct[i % len(distinct)] for i in range(M)]
        pairs = [(shared, b) for b in branches]
        ssoa = marshal_shared(shared, branches)
        soas = [ssoa.merge(m) for m in range(M)]
        ds = _lib.DeviceBatchShared(ssoa)
        dr = _lib.DeviceBatch(soas)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        torch.cuda.synchronize()
        for _ in range(3):
            ds.run(st)
            dr.run(st)
        st.synchronize()
        same = all(all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(ds.results(), dr.results()))
        if not same:
            raise SystemExit(f"the shared and the repeated layout differ at M={M}")
        ts_, tr_ = [], []
        per = max(a.reps // 5, 1)
        for _ in range(5):   # alternate the two paths
            ts_ += [timed(lambda: ds.run(st)) for _ in range(per)]
            tr_ += [timed(lambda: dr.run(st)) for _ in range(per)]

        def legs_shared():
            t0 = time.perf_counter()
            s = marshal_shared(shared, branches, sess.staging_shared(len(shared) + sum(map(len, branches)),
                                                                     len(shared), M))
            kind = s.kind.copy()
            t1 = time.perf_counter()
            res = sess.compose_shared(s, copy=False)
            t2 = time.perf_counter()
            for m, (order, addr, file, ctx, cp) in enumerate(res):
                ops = shared + branches[m]
                k = np.concatenate([kind[: len(shared)], kind[int(s.off[m]): int(s.off[m + 1])]])
                materialize_ops_native(ops, k, s.strings, order, addr, file, ctx)
                materialize_conflicts(ops, cp)
            t3 = time.perf_counter()
            return {"marshal": t1 - t0, "compose": t2 - t1, "copy_device": sess.last["device_s"],
                    "materialise": t3 - t2, "in_bytes": sess.last["in_bytes"]}

        def legs_many():
            t0 = time.perf_counter()
            ns = [len(x) + len(y) for x, y in pairs]
            cols = sess.staging_many(ns)
            ss = [marshal_native(x, y, c) for (x, y), c in zip(pairs, cols)]
            t1 = time.perf_counter()
            res = sess.compose_many(ss, copy=False)
            t2 = time.perf_counter()
            for (x, y), s, (order, addr, file, ctx, cp) in zip(pairs, ss, res):
                materialize_ops_native(x + y, s.kind, s.strings, order, addr, file, ctx)
                materialize_conflicts(x + y, cp)
            t3 = time.perf_counter()
            return {"marshal": t1 - t0, "compose": t2 - t1, "materialise": t3 - t2,
                    "in_bytes": sess._batch_layout(ns)["in_bytes"]}

        def wall(fn):
            t0 = time.perf_counter()
            fn()
            return 1e3 * (time.perf_counter() - t0)

        got, want = compose_against(shared, branches), compose_many(pairs)   # (also the warm-up)
        for (go, gc), (wo, wc) in zip(got[:64], want[:64]):
            if [o.to_dict() for o in go] != [o.to_dict() for o in wo] or len(gc) != len(wc):
                raise SystemExit(f"compose_against and compose_many differ at M={M}")
        legs_shared(), legs_many()
        ws_, wm_, ls_, lm_ = [], [], [], []
        for _ in range(a.wall_reps):   # alternate the two paths
            ws_.append(wall(lambda: compose_against(shared, branches)))
            wm_.append(wall(lambda: compose_many(pairs)))
            ls_.append(legs_shared())
            lm_.append(legs_many())

        def legs(rows_):
            return {k: (stats([1e3 * r[k] for r in rows_]) if k != "in_bytes" else int(rows_[0][k])) for k in rows_[0]}

        s, r = stats(ts_), stats(tr_)
        n_own = sum(len(b) for b in branches)
        row = {"merges": M, "n_shared": len(shared), "own_ops": n_own,
               "device": {"shared": s, "repeated": r, "ratio": round(r["median_ms"] / s["median_ms"], 3)},
               "wall": {"compose_against": stats(ws_), "compose_many": stats(wm_),
                        "ratio": round(float(np.median(wm_) / np.median(ws_)), 3)},
               "legs": {"shared": legs(ls_), "repeated": legs(lm_)},
               "column_bytes_saved_expected": len(shared) * (M - 1) * 37,
               "marshals_of_shared_log": {"shared": 1, "repeated": M}}
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
    line = json.dumps({"shared_probe": rows, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
