#!/usr/bin/env python3
"""Sweep of the block-splitting rule's two constants over tests/support/realdata.py on the CPU model (tests/support/split_model.c):
chunks per 64 KiB parent (= largest number of pieces) x bytes charged per piece.  Prints, per setting and level, the sum over all items
of split-on bytes / split-off bytes, the worst item, and the number of items that got larger.  No GPU involved.
  python tools/split_sweep.py [--levels 3,9] [--chunks 4,8,16] [--costs 48,96,160,256]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import harness  # noqa: E402
import realdata  # noqa: E402
import splitmodel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", default="3,9")
ap.add_argument("--chunks", default="4,8,16")
ap.add_argument("--costs", default="48,96,160,256")
ap.add_argument("--items", default="")
a = ap.parse_args()
oracle, model = harness.Oracle(), splitmodel.SplitModel()
items = {k: v for k, v in realdata.items().items() if v is not None and (not a.items or k in a.items.split(","))}
for level in [int(x) for x in a.levels.split(",")]:
    off = {k: len(oracle.zge_encode(v, oracle.params(level=level))) for k, v in items.items()}
    print("level %d, split off: %d bytes over %d items" % (level, sum(off.values()), len(off)))
    for chunks in [int(x) for x in a.chunks.split(",")]:
        for cost in [int(x) for x in a.costs.split(",")]:
            model.tune(chunks, cost)
            on = {k: len(model.encode(v, level)) for k, v in items.items()}
            rel = {k: on[k] / off[k] for k in items}
            worse = [k for k in items if on[k] > off[k]]
            best = min(rel, key=rel.get)
            print("  chunks %2d cost %3d: sum %.5f  best %s %.4f  larger: %s" % (
                chunks, cost, sum(on.values()) / sum(off.values()), best, rel[best], ", ".join("%s %+d" % (k, on[k] - off[k]) for k in worse) or "none"))
            sys.stdout.flush()
