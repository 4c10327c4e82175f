"""Time merge trains on the GPU: compose_train (one smx_compose_train call for all the trains)
against the per-step way it replaces -- a host loop per train through the session, each step a
compose, a materialise and a marshal again (compose_oplogs(acc, log) with eviction).

The two forms alternate, ROUNDS times each after one warm-up; medians with min to max, of the
whole call and, for compose_train, of its device leg (copy in, smx_compose_train, copy back, one
sync: ComposeSession.last).  Both forms' results are compared once.

    python tools/train_probe.py [--out profiles/train/train_probe.json] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_merge_amd import compose as C  # noqa: E402
from semantic_merge_amd import synth  # noqa: E402
from semantic_merge_amd._session import session  # noqa: E402
from semantic_merge_amd.ops import Op  # noqa: E402

SHAPES = (("256 trains x 8 logs x 100 ops", 256, 8, 100), ("1 train x 16 logs x 120 ops", 1, 16, 120))


def make_logs(n_trains, n_logs, n_ops, seed=5):
    """n_trains * n_logs logs of n_ops ops (lift logs' branches over many symbols: few conflict)."""
    logs = []
    for k in range(n_trains * n_logs // 2 + 1):
        a, b = synth.lift_op_dicts(synth.lift_logs(synth.LiftSpec(2 * n_ops, 50 * n_ops, seed + k)))
        logs += [[Op.from_dict(d) for d in a], [Op.from_dict(d) for d in b]]
    logs = logs[: n_trains * n_logs]
    return logs, [list(range(r * n_logs, (r + 1) * n_logs)) for r in range(n_trains)]


def stat(xs):
    return {"median_ms": round(1e3 * statistics.median(xs), 3), "min_ms": round(1e3 * min(xs), 3),
            "max_ms": round(1e3 * max(xs), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for label, n_trains, n_logs, n_ops in SHAPES:
        logs, trains = make_logs(n_trains, n_logs, n_ops)
        new = C.compose_train(logs, trains)
        old = [C._train_on_host(logs, tr) for tr in trains]
        same = all([o.to_dict() for o in a[0]] == [o.to_dict() for o in b[0]] and
                   [[c.to_dict() for c in s] for s in a[1]] == [[c.to_dict() for c in s] for s in b[1]]
                   for a, b in zip(new, old))
        t_new, t_dev, t_old = [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            C.compose_train(logs, trains)
            t_new.append(time.perf_counter() - t0)
            t_dev.append(session().last["device_s"])
            t0 = time.perf_counter()
            for tr in trains:
                C._train_on_host(logs, tr)
            t_old.append(time.perf_counter() - t0)
        steps = [s for _, st in new for s in st]
        row = {"shape": label, "steps": len(steps), "evicted": sum(1 for s in steps if s), "equal": same,
               "rounds": args.rounds, "compose_train": stat(t_new), "compose_train_device_leg": stat(t_dev),
               "per_step_host_loop": stat(t_old),
               "speedup_median": round(statistics.median(t_old) / statistics.median(t_new), 2)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
