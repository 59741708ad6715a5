#!/usr/bin/env python3
"""Time sts_factor_ols and sts_factor_remove (include/sts_regress.h) at the flagship panel shapes
(1 M x 390, 500 k x 2520; k = 3 factors, shared by the panel and per series), each next to a yardstick
measured in the SAME process, alternating call by call with the case being measured:

  fit only (resid == NULL)   sts_bp_test on the same panel and factors: the same reads, slightly
                             less arithmetic
  fit + residuals            two one-read-one-write kernels of the library on the same panel:
                             sts_factor_remove itself, and sts_fill (linear) on the NaN-free panel
  sts_factor_remove          sts_diff_at_lag (lag 1)

--other-lib PATH adds the same call in ANOTHER build of the library as the yardstick, alternating in
this one process (e.g. tools/variant.sh ... -DSTS_OLS_WAVES=0: one 64-thread workgroup per series,
or the parent commit's build), for shared and per-series factors; --cases other runs only those.

--parent-lib PATH adds the fit-only cases against sts_bp_test of THAT build (the parent commit's
library: the yardstick the comparison is defined against); --cases parent runs only those.

HIP events around every call, every shape warmed up first, --reps timed calls per case (>= 20).
One JSON line per case: median / min ms, the yardstick's, their ratio, achieved bytes/s over the
algorithmic bytes (8 S T read, plus 8 S T where a panel is written) and the library's sha256.

    python tools/factor_ols_timing.py [--reps 20] [--out profiles/factor_ols_timing.jsonl] [--append]
                                      [--other-lib PATH] [--parent-lib PATH] [--cases all|parent|other]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

SHAPES = [(1_000_000, 390), (500_000, 2520)]


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="scale S (a quick look on a busy machine)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--other-lib", default=None, help="another build of the library: the same calls in it")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's build: its sts_bp_test as the yardstick")
    ap.add_argument("--cases", choices=["all", "parent", "other"], default="all")
    a = ap.parse_args()
    assert a.cases != "parent" or a.parent_lib, "--cases parent needs --parent-lib"
    assert a.cases != "other" or a.other_lib, "--cases other needs --other-lib"
    assert a.reps >= 20 or a.scale != 1.0, "at least 20 timed calls per case"
    import torch
    from sparkts import _native
    _native.ensure_device(0)
    lib = _native.lib()
    lib_hash = sha(_native.LIB_PATH)
    other = _native.load_variant(a.other_lib) if a.other_lib else None
    other_hash = sha(a.other_lib) if a.other_lib else None
    parent = None
    if a.parent_lib:      # a build from before include/sts_regress.h: bind the one entry point used
        import ctypes
        parent = ctypes.CDLL(a.parent_lib)
        parent.sts_bp_test.restype, parent.sts_bp_test.argtypes = _native.SIGNATURES["sts_bp_test"]
    parent_hash = sha(a.parent_lib) if a.parent_lib else None
    sp = torch.cuda.current_stream().cuda_stream
    out = open(a.out, "a" if a.append else "w") if a.out else None

    def timed_pair(fn, yard, reps):
        """Alternate fn / yard, one event pair per call -> (list of ms, list of ms)."""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
        for _ in range(3):
            assert fn() == 0
            assert yard() == 0
        torch.cuda.synchronize()
        for e in ev:
            e[0].record()
            assert fn() == 0
            e[1].record()
            e[2].record()
            assert yard() == 0
            e[3].record()
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in ev], [e[2].elapsed_time(e[3]) for e in ev]

    def med(v):
        return sorted(v)[len(v) // 2]

    k = 3
    for S, T in SHAPES:
        S = max(1, int(S * a.scale))
        x = torch.empty((S, T), dtype=torch.float64, device="cuda")
        assert lib.sts_gen_panel(x.data_ptr(), 0, S, T, T, 6, 0.0, sp) == 0
        res = torch.empty((S, T), dtype=torch.float64, device="cuda")
        beta = torch.empty((S, k + 1), dtype=torch.float64, device="cuda")
        se = torch.empty((S, k + 1), dtype=torch.float64, device="cuda")
        st4 = torch.empty((S, 4), dtype=torch.float64, device="cuda")
        stat = torch.empty(S, dtype=torch.float64, device="cuda")
        err = torch.zeros(S, dtype=torch.int32, device="cuda")
        fshared = torch.randn((k, T), dtype=torch.float64, device="cuda")
        fper = torch.randn((S, k, T), dtype=torch.float64, device="cuda")
        X, R, FS, FP = x.data_ptr(), res.data_ptr(), fshared.data_ptr(), fper.data_ptr()

        def ols(L, f, fs, resid):
            return lambda: L.sts_factor_ols(X, S, T, T, f, k, T, fs, beta.data_ptr(), k + 1, se.data_ptr(), st4.data_ptr(),
                                            R if resid else None, T, err.data_ptr(), sp)

        def bp(f, fs, L=lib):
            return lambda: L.sts_bp_test(X, S, T, T, f, k, T, fs, stat.data_ptr(), None, err.data_ptr(), sp)

        def remove(f, fs):
            return lambda: lib.sts_factor_remove(X, R, S, T, T, T, f, k, T, fs, beta.data_ptr(), k + 1, sp)

        def fill():
            return lib.sts_fill(X, R, S, T, T, T, 0, err.data_ptr(), sp)

        def diff():
            return lib.sts_diff_at_lag(X, R, S, T, T, T, 1, 1, sp)

        assert ols(lib, FS, 0, False)() == 0     # beta for the effects cases
        cases = []
        for tag, f, fs in (("shared", FS, 0), ("per_series", FP, k * T)):
            cases += [
                ("ols_fit_%s" % tag, ols(lib, f, fs, False), bp(f, fs), "sts_bp_test", 1),
                ("ols_fit_resid_%s_vs_remove" % tag, ols(lib, f, fs, True), remove(f, fs), "sts_factor_remove", 2),
                ("ols_fit_resid_%s_vs_fill" % tag, ols(lib, f, fs, True), fill, "sts_fill(linear)", 2),
                ("remove_%s" % tag, remove(f, fs), diff, "sts_diff_at_lag", 2),
            ]
        if a.cases != "all":
            cases = []
        if parent and a.cases != "other":
            cases += [("ols_fit_%s_vs_parent_bp" % tag, ols(lib, f, fs, False), bp(f, fs, parent),
                       "sts_bp_test of parent lib " + parent_hash, 1) for tag, f, fs in (("shared", FS, 0), ("per_series", FP, k * T))]
        if other and a.cases != "parent":
            for tag, f, fs in (("shared", FS, 0), ("per_series", FP, k * T)):
                cases += [
                    ("ols_fit_%s_vs_other_form" % tag, ols(lib, f, fs, False), ols(other, f, fs, False),
                     "other lib " + other_hash, 1),
                    ("ols_fit_resid_%s_vs_other_form" % tag, ols(lib, f, fs, True), ols(other, f, fs, True),
                     "other lib " + other_hash, 2),
                ]
        for name, fn, yard, yname, panels in cases:
            ms, yms = timed_pair(fn, yard, a.reps)
            rec = {"case": name, "S": S, "T": T, "k": k, "reps": a.reps, "ms_median": med(ms), "ms_min": min(ms),
                   "yardstick": yname, "yard_ms_median": med(yms), "yard_ms_min": min(yms),
                   "ratio_to_yardstick": med(ms) / med(yms), "yard_min_to_median": min(yms) / med(yms),
                   "GBps": 8.0 * panels * S * T / (med(ms) * 1e-3) / 1e9, "lib_sha256": lib_hash}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del x, res, beta, se, st4, stat, err, fshared, fper, cases
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
