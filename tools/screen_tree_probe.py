"""Time smx_screen_tree on the GPU against the two calls that answer the same question today:
smx_screen_train on the root paths spelled out as trains, and smx_compose_tree where it serves the
shape.  The same LogsSoA is resident on the device once, all rigs (DeviceScreenTree,
DeviceScreenTrains, DeviceTree) live in one process, and the device time is taken between two
events around INNER calls on one stream.  Three shapes:

    stack    every prefix of a 32-log stack of ~40-op logs: a path of 32 nodes and 32 levels,
             against 32 trains of 1 .. 32 steps (32 steps against 528)
    window   a 16-log window of ~100-op logs with every drop-one fallback: the prefixes 1..k and,
             per dropped member i, the prefixes without it; against the same paths as trains
    deep     every prefix of a 32-log stack of ~100-op logs: the path sum passes 2048 ops, so
             smx_compose_tree reports -2 from that node down and is not timed

The forms alternate, ROUNDS times each after WARM warm-up rounds; per call the median with min to
max, in microseconds.  The results are compared once, node by node.  The step and launch counts
of each form are exact.

    python tools/screen_tree_probe.py [--out profiles/screen_tree/probe.json] [--rounds 15] [--inner 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_merge_amd._lib import DeviceScreenTrains, DeviceScreenTree, DeviceTree, _torch  # noqa: E402
from semantic_merge_amd._session import tree_levels  # noqa: E402
from semantic_merge_amd.marshal import marshal_logs, move_file_alt  # noqa: E402

from train_probe import make_logs  # noqa: E402
from tree_probe import per_call_us, stack, stat, window  # noqa: E402

WARM = 3
SHAPES = (("stack: prefixes of 32 logs x 40 ops", stack, 32, 40),
          ("window: 16 logs x 100 ops, drop-one fallbacks", window, 16, 100),
          ("deep: prefixes of 32 logs x 100 ops (path sum over 2048)", stack, 32, 100))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    torch = _torch()
    rows = []
    for label, make, k, n_ops in SHAPES:
        logs, _ = make_logs(1, k, n_ops)
        nodes = make(k)
        lsoa = marshal_logs(logs)
        alt, empty = move_file_alt([o for x in logs for o in x], lsoa.kind, lsoa.strings)
        order, level_off, back = tree_levels([p for p, _ in nodes])
        parents = np.asarray([-1 if nodes[n][0] is None else back[nodes[n][0]] for n in order], np.int32)
        node_log = np.asarray([nodes[n][1] for n in order], np.int32)
        paths = []
        for n in range(len(nodes)):
            path, up = [], n
            while up >= 0:
                path.append(int(node_log[up]))
                up = int(parents[up])
            paths.append(path[::-1])
        levels = len(level_off) - 1
        screen = DeviceScreenTree(lsoa, parents, node_log, level_off)
        trains = DeviceScreenTrains(lsoa, paths)
        tree = DeviceTree(lsoa, parents, node_log, level_off, v1_alt=alt, empty_str=empty)
        for rig in (screen, trains, tree):
            rig.run()
        got, want, full = screen.results(), trains.results(), tree.results()
        same = all(g[:2] == w[2][-1][:2] and np.array_equal(g[2], w[2][-1][2]) for g, w in zip(got, want))
        served = all(f[6] != -2 for f in full)   # smx_compose_tree sends no node back
        same_tree = all(f[6] == -2 or (g[1] == f[6] and np.array_equal(g[2], f[7][:, :2])) for g, f in zip(got, full))
        forms = [("screen_tree", screen), ("screen_train", trains)] + ([("compose_tree", tree)] if served else [])
        times = {name: [] for name, _ in forms}
        for r in range(WARM + args.rounds):
            for name, rig in forms:
                t = per_call_us(torch, rig, args.inner)
                if r >= WARM:
                    times[name].append(t)
        med = {name: statistics.median(v) for name, v in times.items()}
        row = {"shape": label, "nodes": len(nodes), "levels": levels, "ops": int(lsoa.n_total),
               "launches": {"screen_tree": 4 + 3 * levels, "screen_train": 7, "compose_tree": 1 + 3 * levels},
               "steps": {"screen_tree": len(nodes), "screen_train": sum(len(p) for p in paths),
                         "compose_tree": len(nodes)},
               "acc_records": {"screen_tree": int(screen.n_acc), "screen_train": 2 * int(trains.n_acc)},
               "conflicting_nodes": sum(1 for g in got if g[1] > 0),
               "nodes_compose_tree_sends_back": sum(1 for f in full if f[6] == -2),
               "equal_to_screen_train": same, "equal_to_compose_tree_where_it_answers": same_tree,
               "rounds": args.rounds, "inner": args.inner, **{name: stat(v) for name, v in times.items()},
               "screen_train_over_screen_tree_median": round(med["screen_train"] / med["screen_tree"], 2)}
        if served:
            row["compose_tree_over_screen_tree_median"] = round(med["compose_tree"] / med["screen_tree"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
