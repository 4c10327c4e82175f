"""The conflict screen (smx_screen: every log stored and sorted once, conflicts only) against
the parent's way of asking the same question: compose every pair in full and drop the ops.

    python tools/screen_probe.py [--merges 16,256,1024] [--logs 32,128] [--big 50000] [--reps 20]
                                 [--wall-reps 3] [--out profiles/screen/screen_probe.json]

After a warm-up, alternating the two paths in the same run:
  against one log  a shared log of 900 ops and M own logs of 90-110 ops (64 distinct ones,
                   repeated); the parent's way is smx_compose_batch_shared / compose_against
  all pairs        N logs of about 500 ops, all N (N - 1) / 2 pairs; the parent's way is
                   smx_compose_batch / compose_many on the repeated layout
  one big pair     two logs of --big ops with about 1 % renames; the parent's way is smx_compose
Per case: device events around the call alone on device-resident columns; the whole drop-in
calls on Op objects; the new path's legs (marshal, pack, copy + call + copy back, conflict
build) and the bytes copied in and out; each as the median of its repetitions with their
minimum and maximum.  The two paths' conflicts are compared before anything is timed.
Prints one JSON line and writes it to --out.
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
    ap.add_argument("--merges", default="16,256,1024")
    ap.add_argument("--logs", default="32,128")
    ap.add_argument("--big", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _lib, synth
    from semantic_merge_amd.compose import compose_against, compose_many, screen_conflicts
    from semantic_merge_amd.marshal import marshal_logs, marshal_shared
    from semantic_merge_amd.materialize import conflict_factory
    from semantic_merge_amd.ops import Op

    kw = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
    st = torch.cuda.Stream()
    sess = _lib.ComposeSession()

    def ops_of(n, seed, side, n_sym, **k):
        d = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **(k or kw))))[side]
        return [Op.from_dict(x) for x in d]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def device_ab(new, old):
        torch.cuda.synchronize()
        for _ in range(3):
            new()
            old()
        st.synchronize()
        tn, to = [], []
        per = max(a.reps // 5, 1)
        for _ in range(5):   # alternate the two paths
            tn += [timed(new) for _ in range(per)]
            to += [timed(old) for _ in range(per)]
        n, o = stats(tn), stats(to)
        return {"screen": n, "parent": o, "ratio": round(o["median_ms"] / n["median_ms"], 3)}

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    def wall_ab(new, old):
        new(), old()
        wn, wo = [], []
        for _ in range(a.wall_reps):   # alternate the two paths
            wn.append(wall(new))
            wo.append(wall(old))
        return {"screen_conflicts": stats(wn), "parent": stats(wo), "ratio": round(float(np.median(wo) / np.median(wn)), 3)}

    def legs(logs, pairs):
        """The new path step by step on one session."""
        make = conflict_factory()
        rows = []
        for _ in range(a.wall_reps + 1):
            t0 = time.perf_counter()
            lsoa = marshal_logs(logs, sess.staging_logs(sum(map(len, logs)), len(logs), len(pairs)))
            t1 = time.perf_counter()
            found = sess.screen(lsoa, pairs)
            t2 = time.perf_counter()
            for (i, j), cp in zip(pairs, found):
                x, y, na = logs[i], logs[j], len(logs[i])
                [make(x[p], y[q - na]) for p, q in cp.tolist()]
            t3 = time.perf_counter()
            rows.append({"marshal": t1 - t0, "pack": sess.last["pack_s"], "copy_device": sess.last["device_s"],
                         "unpack": sess.last["unpack_s"], "conflict_build": t3 - t2})
        out = {k: stats([1e3 * r[k] for r in rows[1:]]) for k in rows[0]}
        out.update(in_bytes=sess.last["in_bytes"], out_bytes=sess.last["out_bytes"], routed=sess.last["routed"],
                   column_bytes_expected=33 * sum(map(len, logs)))
        return out

    def same(x, y, what):
        if [[c.to_dict() for c in p] for p in x] != [[c.to_dict() for c in p] for p in y]:
            raise SystemExit(f"the screen and the parent's way differ: {what}")

    res = {"against_one_log": [], "all_pairs": [], "one_big_pair": []}

    # -- against one log -----------------------------------------------------------------------
    shared = ops_of(900, 1, 0, 45)
    rng = np.random.default_rng(100)
    distinct = [ops_of(int(n), 1000 + i, 1, 45) for i, n in enumerate(rng.integers(90, 111, 64))]
    for M in [int(x) for x in a.merges.split(",") if x]:
        branches = [distinct[i % 64] for i in range(M)]
        logs = [shared] + branches
        pairs = [(0, m + 1) for m in range(M)]
        same(screen_conflicts(logs, pairs), [c for _, c in compose_against(shared, branches)], f"M={M}")
        dn = _lib.DeviceScreen(marshal_logs(logs), pairs)
        do = _lib.DeviceBatchShared(marshal_shared(shared, branches))
        row = {"merges": M, "n_total": sum(map(len, logs)),
               "device": device_ab(lambda: dn.run(st), lambda: do.run(st)),
               "wall": wall_ab(lambda: screen_conflicts(logs, pairs), lambda: compose_against(shared, branches)),
               "legs": legs(logs, pairs)}
        res["against_one_log"].append(row)
        print(row, file=sys.stderr, flush=True)

    # -- all pairs ---------------------------------------------------------------------------------
    sizes = np.random.default_rng(500).integers(450, 551, 128)
    pool = [ops_of(int(n), 2000 + i, i % 2, 100) for i, n in enumerate(sizes)]
    for N in [int(x) for x in a.logs.split(",") if x]:
        logs = pool[:N]
        pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
        oppairs = [(logs[i], logs[j]) for i, j in pairs]
        same(screen_conflicts(logs), [c for _, c in compose_many(oppairs)], f"N={N}")
        lsoa = marshal_logs(logs)
        dn = _lib.DeviceScreen(lsoa, pairs)
        do = _lib.DeviceBatch([lsoa.pair(i, j) for i, j in pairs])
        ns = [len(x) + len(y) for x, y in oppairs]
        row = {"logs": N, "pairs": len(pairs), "n_total": sum(map(len, logs)),
               "device": device_ab(lambda: dn.run(st), lambda: do.run(st)),
               "wall": wall_ab(lambda: screen_conflicts(logs), lambda: compose_many(oppairs)),
               "legs": legs(logs, pairs),
               "parent_in_bytes": sess._batch_layout(ns)["in_bytes"],
               "extract_runs": {"screen": N, "parent_sorts_of_a_log": N * (N - 1)}}
        res["all_pairs"].append(row)
        print(row, file=sys.stderr, flush=True)
        del do

    # -- one big pair ------------------------------------------------------------------------------
    if a.big:
        mix = (("renameSymbol", 0.01), ("moveDecl", 0.30), ("editStmtBlock", 0.60), ("addDecl", 0.09))
        k = dict(mix=mix, divergent=0.5, rename_overlap=1.0)
        soa = synth.lift_soa(synth.lift_logs(synth.LiftSpec(2 * a.big, 200, 9, **k)))
        from semantic_merge_amd.marshal import LogsSoA
        lsoa = LogsSoA(np.asarray([0, soa.n_a, soa.n], np.int64), soa.kind, soa.ts, soa.oid_hi, soa.oid_lo, soa.sym,
                       soa.v0, soa.v1, soa.n_sym)
        dn = _lib.DeviceScreen(lsoa, [(0, 1)])
        do = _lib.DeviceCompose(soa)
        dn.run(st)
        do.run(st)
        if not np.array_equal(dn.results()[0], do.results()[4]):
            raise SystemExit("the screen and smx_compose differ on the big pair")
        row = {"ops_per_log": a.big, "renames": int((soa.kind == 1).sum()), "conflicts": len(dn.results()[0]),
               "device": device_ab(lambda: dn.run(st), lambda: do.run(st))}
        res["one_big_pair"].append(row)
        print(row, file=sys.stderr, flush=True)

    line = json.dumps({"screen_probe": res, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
