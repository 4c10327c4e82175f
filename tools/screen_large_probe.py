"""The screen's large mode (smx_screen_ex with SMX_SCREEN_LARGE: pairs of more than 2048 renames
screened in the same call) against the parent's way for such pairs: smx_screen, which sends
them back (counts -2), and one full smx_compose per pair sent back.

    python tools/screen_large_probe.py [--merges 16,256,1024] [--shared 100000] [--big 50000]
                                       [--reps 10] [--wall-reps 3] [--parent-wall-max 16]
                                       [--out profiles/screen_large/screen_large_probe.json]

After a warm-up, alternating the two paths in the same run:
  just over   one pair of 1100 + 1100 renames
  queue       one shared log of --shared ops with about 5 % renames against M own logs of about
              100 ops (64 distinct ones, repeated)
  big pair    two logs of --big renames each
Per case: device events around the calls alone on device-resident columns (the parent's way:
smx_screen, then smx_compose on every pair it sent back), and the whole drop-in calls on Op
objects (screen_conflicts with large=True against large=False, which routes through
compose()); each as the median of its repetitions with their minimum and maximum.  The
parent's whole call costs a full composition of the shared log per pair: above
--parent-wall-max pairs it runs once, unrepeated, and the row says so.  The two paths' conflicts
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
    ap.add_argument("--merges", default="16,256,1024")
    ap.add_argument("--shared", type=int, default=100000)
    ap.add_argument("--big", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--parent-wall-max", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from semantic_merge_amd import _lib, synth
    from semantic_merge_amd.compose import screen_conflicts
    from semantic_merge_amd.marshal import marshal_logs
    from semantic_merge_amd.ops import Op

    st = torch.cuda.Stream()

    def ops_of(n, seed, side, n_sym, **k):
        d = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **k)))[side]
        return [Op.from_dict(x) for x in d]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def device_ab(new, old, reps):
        torch.cuda.synchronize()
        new(), old()
        st.synchronize()
        tn, to = [], []
        for _ in range(reps):   # alternate the two paths
            tn.append(timed(new))
            to.append(timed(old))
        n, o = stats(tn), stats(to)
        return {"large": n, "parent": o, "ratio": round(o["median_ms"] / n["median_ms"], 3)}

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    def wall_ab(new, old, parent_reps):
        new()
        wn, wo = [], []
        if parent_reps > 1:
            old()
        for r in range(a.wall_reps):   # alternate the two paths
            wn.append(wall(new))
            if r < parent_reps:
                wo.append(wall(old))
        return {"large": stats(wn), "parent": stats(wo), "parent_warmed_up": parent_reps > 1,
                "ratio": round(float(np.median(wo) / np.median(wn)), 3)}

    def case(logs, pairs, reps, parent_reps):
        """One shape: the results compared, then device events and whole calls."""
        new = screen_conflicts(logs, pairs, large=True)
        if parent_reps:
            old = screen_conflicts(logs, pairs)
            if [[c.to_dict() for c in p] for p in new] != [[c.to_dict() for c in p] for p in old]:
                raise SystemExit("the large mode and the routed path differ")
        lsoa = marshal_logs(logs)
        dn = _lib.DeviceScreen(lsoa, pairs, large=True)
        do = _lib.DeviceScreen(lsoa, pairs)
        do.run(st)
        sent_back = [p for p, r in enumerate(do.results()) if isinstance(r, int) and r == -2]
        dn.run(st)
        got = dn.results()
        # one DeviceCompose per distinct pair sent back (the queue repeats 64 own logs)
        dc, runs = {}, []
        for p in sent_back:
            key = tuple(pairs[p]) if len(pairs) <= 64 else (pairs[p][0], (pairs[p][1] - 1) % 64 + 1)
            if key not in dc:
                dc[key] = _lib.DeviceCompose(lsoa.pair(*key))
                dc[key].run(st)
                if not np.array_equal(dc[key].results()[4], got[p]):
                    raise SystemExit(f"the large mode and smx_compose differ on pair {pairs[p]}")
            runs.append(dc[key])

        def parent():
            do.run(st)
            for c in runs:
                c.run(st)

        ren = _lib._rename_counts(lsoa.kind, lsoa.log_off)
        row = {"pairs": len(pairs), "n_total": int(lsoa.n_total), "renames_per_log_max": int(ren.max()),
               "sent_back": len(sent_back), "conflicts": int(sum(len(g) for g in got)),
               "device": device_ab(lambda: dn.run(st), parent, reps)}
        if parent_reps:
            row["wall"] = wall_ab(lambda: screen_conflicts(logs, pairs, large=True),
                                  lambda: screen_conflicts(logs, pairs), parent_reps)
        else:
            row["wall"] = {"large": stats([wall(lambda: screen_conflicts(logs, pairs, large=True))
                                           for _ in range(a.wall_reps + 1)][1:]), "parent": "not measured"}
        print(row, file=sys.stderr, flush=True)
        return row

    adv = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)
    res = {}

    # -- one pair just over the limit: 1100 + 1100 renames ------------------------------------
    def first_renames(ops, r):
        out, k = [], 0
        for o in ops:
            if o.type == "renameSymbol":
                k += 1
                if k > r:
                    break
            out.append(o)
        assert k > r, "too few renames"
        return out

    pa, pb = first_renames(ops_of(2600, 60, 0, 40, **adv), 1100), first_renames(ops_of(2600, 61, 1, 40, **adv), 1100)
    res["just_over"] = case([pa, pb], [(0, 1)], a.reps, a.wall_reps)

    # -- the queue: one large shared log against M small own logs ------------------------------
    mix = (("renameSymbol", 0.05), ("moveDecl", 0.30), ("editStmtBlock", 0.56), ("addDecl", 0.09))
    shared = ops_of(a.shared, 1, 0, 3000, mix=mix, divergent=0.5, rename_overlap=1.0)
    rng = np.random.default_rng(100)
    distinct = [ops_of(int(n), 1000 + i, 1, 3000, **adv) for i, n in enumerate(rng.integers(90, 111, 64))]
    res["queue"] = []
    for M in [int(x) for x in a.merges.split(",") if x]:
        logs = [shared] + [distinct[i % 64] for i in range(M)]
        pairs = [(0, m + 1) for m in range(M)]
        row = case(logs, pairs, max(a.reps // (1 + M // 64), 2),
                   a.wall_reps if M <= a.parent_wall_max else (1 if M <= 16 * a.parent_wall_max else 0))
        row["merges"] = M
        res["queue"].append(row)

    # -- one pair of two large logs -------------------------------------------------------------
    if a.big:
        hot = dict(mix=(("renameSymbol", 1.0),), divergent=0.5, rename_overlap=1.0)
        la, lb = ops_of(a.big, 7, 0, 5000, **hot), ops_of(a.big, 7, 1, 5000, **hot)
        res["big_pair"] = case([la, lb], [(0, 1)], a.reps, a.wall_reps)

    line = json.dumps({"screen_large_probe": res, "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
