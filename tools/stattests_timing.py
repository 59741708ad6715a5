#!/usr/bin/env python3
"""Time the batched statistical tests (sts_dw_test, sts_kpss_test, sts_adf_test, sts_lb_test,
sts_bp_test, sts_bg_test) at the flagship panel shapes, next to three yardsticks measured in the SAME process, alternating
call by call with the case being measured:

  sts_series_stats   the one-read kernel on the same panel (the rate a one-sweep kernel can reach)
  sts_autocorr       at the Ljung-Box K (what sts_lb_test adds is the epilogue)
  torch              Durbin-Watson composed from torch ops on the device
  sts_dw_test        for Breusch-Pagan (the other one-read residual test)
  sts_adf_test       (5, ct) for Breusch-Godfrey at maxLag 5 (the other lag-Gram kernel)

Breusch-Pagan and Breusch-Godfrey (maxLag 1 and 5) run with k = 3 factors, once shared by the panel
and once per series.

--other-lib PATH adds the ADF (1, c) and (5, ct), Breusch-Pagan and Breusch-Godfrey cases with the
same call in ANOTHER build of the library (e.g. the parent commit's) as the yardstick, alternating
in this one process; --cases other runs only those.

HIP events around every call, every shape warmed up first, --reps timed calls per case (>= 20).
One JSON line per case: median / min ms, the yardstick's, their ratio, achieved bytes/s
(8 S T over the median) and the library's sha256.

    python tools/stattests_timing.py [--reps 20] [--cases all|t1t4|bgbp|other] [--append]
                                     [--out profiles/stattests_timing.jsonl] [--other-lib PATH]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

SHAPES = [(1_000_000, 390), (500_000, 2520)]
REG_C, REG_CT = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="scale S (a quick look on a busy machine)")
    ap.add_argument("--cases", choices=["all", "t1t4", "bgbp", "other"], default="all")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--other-lib", default=None, help="another build of the library: the same calls in it")
    a = ap.parse_args()
    assert a.cases != "other" or a.other_lib, "--cases other needs --other-lib"
    assert a.reps >= 20 or a.scale != 1.0, "at least 20 timed calls per case"
    import torch
    from sparkts import _native
    _native.ensure_device(0)
    lib = _native.lib()
    with open(_native.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    other, other_name = None, None
    if a.other_lib:
        other = _native.load_variant(a.other_lib)
        with open(a.other_lib, "rb") as f:
            other_name = "other lib " + hashlib.sha256(f.read()).hexdigest()[:16]
    sp = torch.cuda.current_stream().cuda_stream
    out = open(a.out, "a" if a.append else "w") if a.out else None

    def timed_pair(fn, yard, reps):
        """Alternate fn / yard, one event pair per call -> (list of ms, list of ms)."""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
        for _ in range(3):
            assert fn() == 0
            yard()
        torch.cuda.synchronize()
        for e in ev:
            e[0].record()
            assert fn() == 0
            e[1].record()
            e[2].record()
            yard()
            e[3].record()
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in ev], [e[2].elapsed_time(e[3]) for e in ev]

    def med(v):
        return sorted(v)[len(v) // 2]

    for S, T in SHAPES:
        S = max(1, int(S * a.scale))
        x = torch.empty((S, T), dtype=torch.float64, device="cuda")
        assert lib.sts_gen_panel(x.data_ptr(), 0, S, T, T, 6, 0.0, sp) == 0
        stat = torch.empty(S, dtype=torch.float64, device="cuda")
        pv = torch.empty(S, dtype=torch.float64, device="cuda")
        st4 = torch.empty((S, 4), dtype=torch.float64, device="cuda")
        K = 20
        acf = torch.empty((S, K), dtype=torch.float64, device="cuda")
        err = torch.zeros(S, dtype=torch.int32, device="cuda")
        X = x.data_ptr()

        def series_stats():
            assert lib.sts_series_stats(X, S, T, T, st4.data_ptr(), sp) == 0

        def autocorr():
            assert lib.sts_fill_autocorr(X, None, S, T, T, T, -1, K, acf.data_ptr(), err.data_ptr(), sp) == 0

        def torch_dw():
            d = x[:, 1:] - x[:, :-1]
            return (d * d).sum(dim=1) / (x * x).sum(dim=1)

        cases = [
            ("dw", lambda: lib.sts_dw_test(X, S, T, T, stat.data_ptr(), sp), series_stats, "sts_series_stats"),
            ("dw_vs_torch", lambda: lib.sts_dw_test(X, S, T, T, stat.data_ptr(), sp), torch_dw, "torch"),
            ("kpss_c", lambda: lib.sts_kpss_test(X, S, T, T, REG_C, stat.data_ptr(), sp), series_stats, "sts_series_stats"),
            ("kpss_ct", lambda: lib.sts_kpss_test(X, S, T, T, REG_CT, stat.data_ptr(), sp), series_stats, "sts_series_stats"),
            ("adf_1_c", lambda: lib.sts_adf_test(X, S, T, T, 1, REG_C, stat.data_ptr(), pv.data_ptr(), err.data_ptr(), sp),
             series_stats, "sts_series_stats"),
            ("adf_5_ct", lambda: lib.sts_adf_test(X, S, T, T, 5, REG_CT, stat.data_ptr(), pv.data_ptr(), err.data_ptr(), sp),
             series_stats, "sts_series_stats"),
            ("lb_20", lambda: lib.sts_lb_test(X, S, T, T, K, stat.data_ptr(), pv.data_ptr(), sp), autocorr, "sts_autocorr"),
            ("lb_20_vs_stats", lambda: lib.sts_lb_test(X, S, T, T, K, stat.data_ptr(), pv.data_ptr(), sp), series_stats,
             "sts_series_stats"),
        ]
        if a.cases in ("bgbp", "other"):
            cases = []
        if other:
            def adf(L, p, reg):
                return lambda: L.sts_adf_test(X, S, T, T, p, reg, stat.data_ptr(), pv.data_ptr(), err.data_ptr(), sp)

            cases += [("adf_1_c_vs_other", adf(lib, 1, REG_C), adf(other, 1, REG_C), other_name),
                      ("adf_5_ct_vs_other", adf(lib, 5, REG_CT), adf(other, 5, REG_CT), other_name)]
        if a.cases != "t1t4":
            k = 3
            fshared = torch.randn((k, T), dtype=torch.float64, device="cuda")
            fper = torch.randn((S, k, T), dtype=torch.float64, device="cuda")
            FS, FP = fshared.data_ptr(), fper.data_ptr()

            def dw():
                assert lib.sts_dw_test(X, S, T, T, stat.data_ptr(), sp) == 0

            def adf_5_ct():
                assert lib.sts_adf_test(X, S, T, T, 5, REG_CT, stat.data_ptr(), pv.data_ptr(), err.data_ptr(), sp) == 0

            def bp(f, fs, L=lib):
                return lambda: L.sts_bp_test(X, S, T, T, f, k, T, fs, stat.data_ptr(), pv.data_ptr(), err.data_ptr(), sp)

            def bg(f, fs, lag, L=lib):
                return lambda: L.sts_bg_test(X, S, T, T, f, k, T, fs, lag, stat.data_ptr(), pv.data_ptr(),
                                               err.data_ptr(), sp)

            if other:
                for tag, f, fs in (("shared", FS, 0), ("per_series", FP, k * T)):
                    cases += [("bp_3_%s_vs_other" % tag, bp(f, fs), bp(f, fs, other), other_name),
                              ("bg_1_3_%s_vs_other" % tag, bg(f, fs, 1), bg(f, fs, 1, other), other_name),
                              ("bg_5_3_%s_vs_other" % tag, bg(f, fs, 5), bg(f, fs, 5, other), other_name)]
            bgbp = [
                ("bp_3_shared", bp(FS, 0), series_stats, "sts_series_stats"),
                ("bp_3_shared_vs_dw", bp(FS, 0), dw, "sts_dw_test"),
                ("bp_3_per_series", bp(FP, k * T), series_stats, "sts_series_stats"),
                ("bp_3_per_series_vs_dw", bp(FP, k * T), dw, "sts_dw_test"),
                ("bg_1_3_shared", bg(FS, 0, 1), series_stats, "sts_series_stats"),
                ("bg_1_3_per_series", bg(FP, k * T, 1), series_stats, "sts_series_stats"),
                ("bg_5_3_shared", bg(FS, 0, 5), series_stats, "sts_series_stats"),
                ("bg_5_3_shared_vs_dw", bg(FS, 0, 5), dw, "sts_dw_test"),
                ("bg_5_3_shared_vs_adf", bg(FS, 0, 5), adf_5_ct, "sts_adf_test(5, ct)"),
                ("bg_5_3_per_series", bg(FP, k * T, 5), series_stats, "sts_series_stats"),
                ("bg_5_3_per_series_vs_adf", bg(FP, k * T, 5), adf_5_ct, "sts_adf_test(5, ct)"),
            ]
            if a.cases != "other":
                cases += bgbp
        for name, fn, yard, yname in cases:
            ms, yms = timed_pair(fn, yard, a.reps)
            rec = {"case": name, "S": S, "T": T, "reps": a.reps, "ms_median": med(ms), "ms_min": min(ms),
                   "yardstick": yname, "yard_ms_median": med(yms), "yard_ms_min": min(yms),
                   "ratio_to_yardstick": med(ms) / med(yms), "GBps": 8.0 * S * T / (med(ms) * 1e-3) / 1e9,
                   "yard_min_to_median": min(yms) / med(yms), "lib_sha256": lib_hash}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del x, stat, pv, st4, acf, err, cases
        if a.cases != "t1t4":
            del fshared, fper
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
