"""Time the screen of merge trains on the GPU: screen_train (one smx_screen_train call for all the
trains, from the logs' renames alone) against what answers the same question today --
compose_train (one smx_compose_train call, every step composed in full), and for a shape that
compose_train refuses (a step over 2048 ops) the host loop over compose_oplogs it falls back to.

The forms alternate, ROUNDS times each after one warm-up; medians with min to max, of the whole
call and of its device leg (copy in, the library call, copy back, one sync: ComposeSession.last).
Both forms' answers are compared once: which steps conflict, and over which ops.

    python tools/screen_train_probe.py [--out profiles/screen_train/probe.json] [--rounds 5]
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
from semantic_merge_amd._session import session  # noqa: E402

from train_probe import make_logs, stat  # noqa: E402

# (label, trains, logs per train, ops per log, the other form)
SHAPES = (("256 trains x 8 logs x 100 ops", 256, 8, 100, "compose_train"),
          ("1 train x 16 logs x 120 ops", 1, 16, 120, "compose_train"),
          ("1 train x 16 logs x 1000 ops", 1, 16, 1000, "host_loop"))


def positions(logs, steps):
    """Per step the conflicts' ops as ((log, index), (log, index)), by op id."""
    at = {o.id: (l, i) for l, log in enumerate(logs) for i, o in enumerate(log)}
    return [[(at[c.opA["id"]], at[c.opB["id"]]) for c in step] for step in steps]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for label, n_trains, n_logs, n_ops, other in SHAPES:
        logs, trains = make_logs(n_trains, n_logs, n_ops)

        def old():
            if other == "compose_train":
                return C.compose_train(logs, trains)
            return [C._train_on_host(logs, tr) for tr in trains]

        new = C.screen_train(logs, trains)
        same = new == [positions(logs, steps) for _, steps in old()]
        t_new, t_new_dev, t_old, t_old_dev = [], [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            C.screen_train(logs, trains)
            t_new.append(time.perf_counter() - t0)
            t_new_dev.append(session().last["device_s"])
            t0 = time.perf_counter()
            old()
            t_old.append(time.perf_counter() - t0)
            if other == "compose_train":
                t_old_dev.append(session().last["device_s"])
        steps = [s for tr in new for s in tr]
        row = {"shape": label, "steps": len(steps), "evicted": sum(1 for s in steps if s), "equal": same,
               "renames": sum(o.type == "renameSymbol" for log in logs for o in log), "rounds": args.rounds,
               "screen_train": stat(t_new), "screen_train_device_leg": stat(t_new_dev), other: stat(t_old),
               "speedup_median": round(statistics.median(t_old) / statistics.median(t_new), 2)}
        if t_old_dev:
            row[other + "_device_leg"] = stat(t_old_dev)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
