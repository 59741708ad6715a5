"""Timing of ARIMA.fitModelCSS: fitModelCSS(1, 0, 1) and (2, 1, 2) over a
100 000 x 250 panel of sts_gen_ar_panel rows, device events around the call, median of 5 after a
warm-up; and the host build of the same state machine (tests/native/arima_sm_harness.cpp, built
here with g++) over the first 1 000 of those rows from the device's start, on one core.

    python tools/arima_timing.py [--out FILE]      prints one JSON document
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "spark-timeseries_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
from sparkts import _native
from sparkts.models.ARIMA import ARIMA

S, T = 100000, 250
_native.ensure_device(0)
lib = _native.lib()
x = torch.empty((S, T), dtype=torch.float64, device="cuda:0")
c = torch.empty(S, dtype=torch.float64, device="cuda:0")
phi = torch.empty((S, 2), dtype=torch.float64, device="cuda:0")
assert lib.sts_gen_ar_panel(x.data_ptr(), c.data_ptr(), phi.data_ptr(), 0, S, T, T, 1234, 2, None) == 0
torch.cuda.synchronize()
res = {"S": S, "T": T}
harness = os.path.join(tempfile.mkdtemp(prefix="arima_timing_"), "arima_sm")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                       "-I", os.path.join(ROOT, "spark-timeseries_amd", "csrc"),
                       os.path.join(ROOT, "tests", "native", "arima_sm_harness.cpp"), "-o", harness])
for p, d, q in ((1, 0, 1), (2, 1, 2)):
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    times = []
    for rep in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = ARIMA.fitModelCSS(p, d, q, x, errors=err)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ev = m.evaluations.cpu().numpy()
    eh = err.cpu().numpy()
    key = "fit_%d%d%d" % (p, d, q)
    res[key] = {"ms_warmup": times[0], "ms_median_of_5": statistics.median(times[1:]), "ms_all": times[1:],
                "evals_min": int(ev.min()), "evals_median": float(np.median(ev)), "evals_p99": float(np.percentile(ev, 99)),
                "evals_max": int(ev.max()), "evals_sum": int(ev.sum()),
                "status_counts": {str(k): int((eh == k).sum()) for k in np.unique(eh)}}
    # per-wave maximum vs mean: what the slowest lane costs
    w = ev[: S // 64 * 64].reshape(-1, 64)
    res[key]["wave_max_mean"] = float(w.max(axis=1).mean())
    res[key]["lane_mean"] = float(ev.mean())
    # host harness, one core, first 1000 rows
    n = 1000
    xs = x[:n].cpu().numpy()
    for _ in range(d):
        xs = np.diff(xs, axis=1)
    init = m.initParams[:n].cpu().numpy()
    ok = np.isfinite(init).all(axis=1)
    xs, init = np.ascontiguousarray(xs[ok]), np.ascontiguousarray(init[ok])
    inp = "%d %d 1 %d %d\n" % (p, q, xs.shape[0], xs.shape[1])
    inp += " ".join("%x" % v for v in xs.view(np.uint64).ravel()) + "\n" + " ".join("%x" % v for v in init.view(np.uint64).ravel())
    t0 = time.perf_counter()
    r = subprocess.run([harness, "time"], input=inp, capture_output=True, text=True, check=True)
    res[key]["harness_rows"] = int(xs.shape[0])
    res[key]["harness_stderr"] = r.stderr.strip()
    res[key]["harness_wall_s_with_parse"] = time.perf_counter() - t0
    hev = np.array([int(l.split()[-2]) for l in r.stdout.splitlines()])
    res[key]["harness_evals_sum"] = int(hev.sum())
print(json.dumps(res))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(res, f, indent=1)
