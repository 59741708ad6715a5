#!/usr/bin/env python3
"""Write tests/golden/factor_ols_exact.json: for the hard rows of tests/factor_ols_ref.py (bgbp_ref's
ten -- a response at level 1e4, factors at level 1e6, two factors collinear to 1e-6, a trending
factor, white noise; T = 390 / 2520, k = 3 -- and a near-exact fit at level 1e4) the OLS
coefficients (to 106 bits: the float64 value and what its rounding left), standard errors, RSS, TSS,
R^2 and error variance evaluated from the normal equations in 60-digit mpmath, as hex floats; the
exact residuals follow from the coefficients (factor_ols_ref.exact_resid).  The rows themselves are
regenerated from their seeds (factor_ols_ref.hard_row).

Needs mpmath; the GPU tests read only the JSON.  --check compares instead of writing."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import factor_ols_ref as fr  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "factor_ols_exact.json")


def hexes(v):
    return [float(x).hex() for x in v]


def build():
    rows = []
    for i, (name, T) in enumerate(fr.HARD_ROWS):
        y, F = fr.hard_row(i)
        ex = fr.exact(y, F)
        rows.append({
            "name": name, "T": T, "y0": float(y[0]).hex(), "ylast": float(y[-1]).hex(), "f_last": float(F[-1, -1]).hex(),
            "exact": {"beta": hexes(ex.beta), "beta_lo": hexes(ex.beta_lo), "se": hexes(ex.se), "stats": hexes(ex.stats)},
        })
    return {"dps": 60, "k": fr.HARD_K, "rows": rows}


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
