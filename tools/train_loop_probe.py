"""Time merge trains with steps over 2048 ops on the GPU: compose_train(..., large=True) -- the
train's steps as smx_train_stage, smx_compose and smx_train_land over columns that stay on the
device, materialised once -- against compose_train as it was, which finds the -2 step and runs
the train again as the host loop (_train_on_host: compose_oplogs(acc, log) with eviction, every
step materialised, marshalled and copied in again).

The two forms alternate, ROUNDS times each after one warm-up; medians with min to max, of the
whole call and, for large=True, of its device legs: the smx_compose_train call that reports the
-2 step (both forms pay it) and the loop (copy in, the steps, copy back: ComposeSession.last).
Both forms' results are compared once.

    python tools/train_loop_probe.py [--out profiles/train_loop/probe.json] [--rounds 5]
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
from semantic_merge_amd._session import ComposeSession  # noqa: E402

from train_probe import make_logs, stat  # noqa: E402

SHAPES = (("1 train x 16 logs x 1000 ops", 1, 16, 1000), ("1 train x 8 logs x 20000 ops", 1, 8, 20000))


def as_dicts(res):
    return [([o.to_dict() for o in out], [[c.to_dict() for c in s] for s in steps]) for out, steps in res]


def timed_legs():
    """ComposeSession.compose_trains and .compose_train_loop wrapped to note their device legs."""
    legs = {"compose_trains": [], "compose_train_loop": []}
    for name in legs:
        real = getattr(ComposeSession, name)

        def wrapped(self, *a, _real=real, _name=name, **kw):
            out = _real(self, *a, **kw)
            legs[_name].append(self.last["device_s"])
            return out
        setattr(ComposeSession, name, wrapped)
    return legs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    legs = timed_legs()
    rows = []
    for label, n_trains, n_logs, n_ops in SHAPES:
        logs, trains = make_logs(n_trains, n_logs, n_ops)
        new = C.compose_train(logs, trains, large=True)
        same = as_dicts(new) == as_dicts(C.compose_train(logs, trains))
        t_new, t_screen, t_loop, t_old = [], [], [], []
        for _ in range(args.rounds):
            for v in legs.values():
                v.clear()
            t0 = time.perf_counter()
            C.compose_train(logs, trains, large=True)
            t_new.append(time.perf_counter() - t0)
            t_screen.append(sum(legs["compose_trains"]))
            t_loop.append(sum(legs["compose_train_loop"]))
            t0 = time.perf_counter()
            C.compose_train(logs, trains)
            t_old.append(time.perf_counter() - t0)
        steps = [s for _, st in new for s in st]
        row = {"shape": label, "steps": len(steps), "evicted": sum(1 for s in steps if s),
               "ops_left": sum(len(out) for out, _ in new), "equal": same, "rounds": args.rounds,
               "large": stat(t_new), "large_compose_trains_device_leg": stat(t_screen),
               "large_loop_device_leg": stat(t_loop), "host_loop": stat(t_old),
               "speedup_median": round(statistics.median(t_old) / statistics.median(t_new), 2)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
