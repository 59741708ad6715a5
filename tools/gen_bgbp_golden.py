#!/usr/bin/env python3
"""Write tests/golden/bgbp_exact.json: for the hard rows of tests/bgbp_ref.py (residuals at level
1e4, factors at level 1e6, two factors collinear to 1e-6, a trending factor, white-noise residuals;
T = 390 / 2520, k = 3)
the Breusch-Pagan statistic and the Breusch-Godfrey statistic at maxLag 5 evaluated from the
reference's formulas in 60-digit mpmath, as hex floats.  The rows themselves are regenerated from
their seeds (tests/bgbp_ref.hard_row).

Needs mpmath; the GPU tests read only the JSON.  --check compares instead of writing."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import bgbp_ref as br  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "bgbp_exact.json")


def build():
    rows = []
    for i, (name, T) in enumerate(br.HARD_ROWS):
        e, F = br.hard_row(i)
        rows.append({
            "seed": br.HARD_SEED + i, "name": name, "T": T,
            "e0": float(e[0]).hex(), "elast": float(e[-1]).hex(), "f_last": float(F[-1, -1]).hex(),
            "exact": {"bp": float(br.exact_bp(e, F)).hex(), "bg_%d" % br.HARD_LAG: float(br.exact_bg(e, F, br.HARD_LAG)).hex()},
        })
    return {"dps": 60, "k": br.HARD_K, "max_lag": br.HARD_LAG, "rows": rows}


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
