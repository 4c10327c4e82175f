"""Host legs of ComposeSession's calls, for comparing two trees of the package (a parent commit's
and this one's) in runs that alternate: bench.py's small_merge figures (dropin_ms and its
compose_soa leg, as `bench.py --full` reports them) and the pack / copy_device / unpack legs
(`last[...]`) of screen, compose_shared and screen_all on the workloads of screen_probe.py,
shared_probe.py and cand_probe.py.

    python tools/host_legs_probe.py run PKG_ROOT OUT.json      one process, one tree (PKG_ROOT holds
                                                               semantic_merge_amd/ with its built libraries)
    python tools/host_legs_probe.py verdict OUT.json PARENT_RUNS... -- NEW_RUNS...

The verdict's rule: per figure the margin is the parent's own spread (largest minus smallest of
its runs); the new tree's median must not exceed the parent's largest plus that margin."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 15


def run(pkg_root: str, out_path: str) -> None:
    import numpy as np
    sys.path[:0] = [os.path.abspath(pkg_root), REPO]
    import semantic_merge_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(semantic_merge_amd.__file__))) == os.path.abspath(pkg_root)
    import bench
    from semantic_merge_amd import _lib, synth
    from semantic_merge_amd.marshal import marshal_logs, marshal_shared
    from semantic_merge_amd.ops import Op

    kw = dict(mix=synth.ADVERSARIAL_MIX, divergent=0.3, rename_overlap=1.0)

    def ops_of(n, seed, side, n_sym):
        d = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n, n_sym, seed, **kw)))[side]
        return [Op.from_dict(x) for x in d]

    def med(rows):
        return {k: round(float(np.median([1e3 * r[k] for r in rows])), 5) for k in rows[0]}

    def legs_of(last):
        return {"pack": last["pack_s"], "copy_device": last["device_s"], "unpack": last["unpack_s"]}

    small = bench.small_merge(1000, 50)
    out = {"pkg": os.path.abspath(pkg_root), "dropin_ms": small["dropin_ms"],
           "compose_soa_ms": small["dropin_legs_ms"]["compose_soa"]}
    sess = _lib.ComposeSession()
    shared = ops_of(900, 1, 0, 45)
    rng = np.random.default_rng(100)
    branches = [ops_of(int(n), 1000 + i, 1, 45) for i, n in enumerate(rng.integers(90, 111, 64))]
    branches = [branches[i % 64] for i in range(256)]
    logs = [shared] + branches
    pairs = [(0, m + 1) for m in range(256)]
    tot = sum(map(len, logs))

    rows = []
    for _ in range(REPS + 2):
        lsoa = marshal_logs(logs, sess.staging_logs(tot, len(logs), len(pairs)))
        sess.screen(lsoa, pairs)
        rows.append(legs_of(sess.last))
    out["screen"] = med(rows[2:])

    rows = []
    for _ in range(REPS + 2):
        s = marshal_shared(shared, branches, sess.staging_shared(tot, len(shared), len(branches)))
        t0 = time.perf_counter()
        sess.compose_shared(s, copy=False)
        rows.append(dict(legs_of(sess.last), compose=time.perf_counter() - t0))
    out["shared"] = med(rows[2:])

    cl = [ops_of(int(n), 5000 + i, i % 2, 400) for i, n in enumerate(rng.integers(60, 141, 128))]
    ctot = sum(map(len, cl))
    rows = []
    for _ in range(REPS + 2):
        lsoa = marshal_logs(cl, sess.staging_logs(ctot, len(cl), max(9 * len(cl), 2048)))
        p, _f = sess.screen_all(lsoa)
        rows.append(legs_of(sess.last))
    out["cand"] = dict(med(rows[2:]), n_candidates=int(len(p)), retries=int(sess.last["retries"]))

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh)
        fh.write("\n")
    print(json.dumps(out))


def figures(r: dict) -> dict:
    d = {"dropin_ms": r["dropin_ms"], "dropin_legs_ms.compose_soa": r["compose_soa_ms"]}
    for call in ("screen", "shared", "cand"):
        for leg in ("pack", "copy_device", "unpack"):
            d[f"{call}.{leg}_ms"] = r[call][leg]
    return d


def verdict(out_path: str, parent_paths, new_paths) -> None:
    runs = {"parent": [figures(json.load(open(p))) for p in parent_paths],
            "new": [figures(json.load(open(p))) for p in new_paths]}
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps_per_run": REPS,
           "runs": {k: len(v) for k, v in runs.items()}, "rule": __doc__.split("\n\n")[-1].replace("\n", " "),
           "figures": {}}
    ok = True
    for k in runs["parent"][0]:
        p, n = [r[k] for r in runs["parent"]], [r[k] for r in runs["new"]]
        spread = max(p) - min(p)
        within = statistics.median(n) <= max(p) + spread
        ok &= within
        out["figures"][k] = {"parent": p, "new": n, "parent_median": statistics.median(p),
                             "new_median": statistics.median(n), "parent_spread": round(spread, 5),
                             "limit": round(max(p) + spread, 5), "within": within}
        print(f"{k:30s} parent {statistics.median(p):.4f} [{min(p):.4f}, {max(p):.4f}]  new "
              f"{statistics.median(n):.4f}  limit {max(p) + spread:.4f}  {'ok' if within else 'SLOWER'}")
    out["verdict"] = "every leg within the margin" if ok else "a leg is slower than the margin"
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(out["verdict"])


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        split = sys.argv.index("--")
        verdict(sys.argv[2], sys.argv[3:split], sys.argv[split + 1:])
