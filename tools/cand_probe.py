"""screen_all (candidate pairs on the device, then the screen of those alone, on columns copied
once) against the parent's way of asking which of N logs conflict with each other:
screen_conflicts(logs) over all i < j.

    python tools/cand_probe.py [--logs 32,128] [--space 200000] [--reps 20] [--wall-reps 3]
                               [--out profiles/cand/cand_probe.json]

Two workloads, N logs of 450-550 ops each:
  all pairs   DESIGN.md §13's shape: one small symbol space, so nearly every pair is a candidate
  sparse      the same logs with every log's symbols drawn from a space of --space symbols, so
              that a small share of the pairs shares a renamed symbol (the share is reported)
Per case, after a warm-up, alternating the two paths in the same run: device events around the
calls alone on device-resident columns (new: smx_screen_candidates, then smx_screen on the
candidates with their exact count; parent: smx_screen on all pairs); the whole calls on Op
objects; the new path's byte counts and candidates; each as the median of its repetitions with
their minimum and maximum.  The two paths' conflicts are compared before anything is timed.
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
    ap.add_argument("--logs", default="32,128")
    ap.add_argument("--space", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _lib, synth
    from semantic_merge_amd.compose import screen_all, screen_conflicts
    from semantic_merge_amd.marshal import marshal_logs
    from semantic_merge_amd.ops import Op

    kw = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
    st = torch.cuda.Stream()
    sess = _lib.ComposeSession()

    def dicts_of(n, seed, side, n_sym):
        return synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **kw)))[side]

    def respread(d, rng, space):
        """The log's symbols mapped one to one into a space of `space` symbol ids."""
        names = sorted({x["target"]["symbolId"] for x in d})
        m = dict(zip(names, (f"sym-{int(i)}" for i in rng.choice(space, len(names), replace=False))))
        out = []
        for x in d:
            y = dict(x)
            y["target"] = dict(x["target"], symbolId=m[x["target"]["symbolId"]])
            out.append(y)
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def ab(new, old, reps, t):
        new(), old()
        tn, to = [], []
        per = max(reps // 5, 1)
        for _ in range(5 if reps >= 5 else reps):   # alternate the two paths
            tn += [t(new) for _ in range(per)]
            to += [t(old) for _ in range(per)]
        n, o = stats(tn), stats(to)
        return {"screen_all": n, "parent": o, "ratio": round(o["median_ms"] / n["median_ms"], 3)}

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    def case(label, logs):
        N = len(logs)
        every = [(i, j) for i in range(N) for j in range(i + 1, N)]
        dense = screen_conflicts(logs)
        got = screen_all(logs)
        want = {p: c for p, c in zip(every, dense) if c}
        if list(got) != list(want) or any([c.to_dict() for c in got[p]] != [c.to_dict() for c in want[p]] for p in want):
            raise SystemExit(f"screen_all and screen_conflicts differ: {label} N={N}")
        lsoa = marshal_logs(logs)
        pairs, _ = sess.screen_all(lsoa)
        last = dict(sess.last)
        sess.screen(lsoa, every)
        parent_last = dict(sess.last)
        dc = _lib.DeviceCandidates(lsoa, pair_cap=max(len(pairs), 1))
        dn = _lib.DeviceScreen(lsoa, pairs) if len(pairs) else None
        do = _lib.DeviceScreen(lsoa, every)

        def new():
            dc.run(st)
            if dn is not None:
                dn.run(st)

        row = {"workload": label, "logs": N, "pairs": len(every), "n_total": int(lsoa.n_total),
               "candidates": len(pairs), "candidate_share": round(len(pairs) / len(every), 4),
               "pairs_with_conflicts": len(want),
               "device": ab(new, lambda: do.run(st), a.reps, timed),
               "device_candidates_alone": stats([timed(lambda: dc.run(st)) for _ in range(a.reps)]),
               "wall": ab(lambda: screen_all(logs), lambda: screen_conflicts(logs), a.wall_reps, wall),
               "screen_all_last": {k: last[k] for k in ("in_bytes", "out_bytes", "n_candidates", "retries", "routed")},
               "parent_last": {k: parent_last[k] for k in ("in_bytes", "out_bytes", "routed")},
               "column_bytes_expected": 33 * int(lsoa.n_total)}
        print(row, file=sys.stderr, flush=True)
        return row

    sizes = np.random.default_rng(500).integers(450, 551, 128)
    pool = [dicts_of(int(n), 2000 + i, i % 2, 100) for i, n in enumerate(sizes)]
    rng = np.random.default_rng(77)
    sparse = [respread(d, rng, a.space) for d in pool]
    rows = []
    for N in [int(x) for x in a.logs.split(",") if x]:
        rows.append(case("all pairs", [[Op.from_dict(x) for x in d] for d in pool[:N]]))
        rows.append(case("sparse", [[Op.from_dict(x) for x in d] for d in sparse[:N]]))
    line = json.dumps({"cand_probe": rows, "space": a.space, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
