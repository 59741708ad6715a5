#!/usr/bin/env python3
"""Write tests/golden/stattests_exact.json: for the hard rows of tests/stattests_ref.py (level
1e4 / 1e6, drift 0 / 1 / 10 per step, noise 1e-2 / 1e-1, walk / stationary, T = 390 / 2520) the
ADF and KPSS statistics evaluated from the reference's formulas in 60-digit mpmath, as hex floats.
The rows themselves are regenerated from their seeds (tests/stattests_ref.hard_row).

Needs mpmath; the GPU tests read only the JSON.  --check compares instead of writing."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import stattests_ref as ref  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "stattests_exact.json")


def build():
    rows = []
    for i, (level, drift, noise, kind, T) in enumerate(ref.HARD_ROWS):
        x = ref.hard_row(i)
        rows.append({
            "seed": ref.HARD_SEED + i, "level": level, "drift": drift, "noise": noise, "kind": kind, "T": T,
            "x0": float(x[0]).hex(), "xlast": float(x[-1]).hex(),
            "exact": {"%s_%d_%s" % st: float(ref.exact_stat(st[0], st[1], st[2], x)).hex() for st in ref.HARD_STATS},
        })
    return {"dps": 60, "stats": ["%s_%d_%s" % st for st in ref.HARD_STATS], "rows": rows}


def dumps(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = dumps(build())
    if a.check:
        sys.exit(0 if open(PATH).read() == text else 1)
    with open(PATH, "w") as f:
        f.write(text)
    print("wrote %s (%d bytes)" % (PATH, len(text)))
