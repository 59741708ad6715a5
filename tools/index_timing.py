#!/usr/bin/env python3
"""Time the entry points of include/sts_index.h: one JSON line per case with the median / min ms,
the bytes the result needs and the achieved TB/s over the median, and the library's sha256.

  At S x 390 (S = 1 M at full scale), each against sts_fill_with_default at the same shape IN THE SAME
  PROCESS, alternating call by call -- it moves the same S*T read + S*T write, so it is the yardstick:
    rebase_shift start_loc 0, 1, -5         (rows that stay 16-byte aligned, and rows that do not)
    rebase_map   identity, 5 % holes
  align_uniform  S ragged series of mean length 390 onto 390 instants
  index_locs     64 M timestamps (scaled) against a business-day index and an irregular index of
                 100 000 instants, beside the host path the lookup had before: the np.searchsorted
                 block of io.timeSeriesRDDFromObservations plus the upload of loc (--host-reps calls).

HIP events around every call on one side stream, every case warmed up first, --reps timed calls per
case (>= 20 at full scale).

    python tools/index_timing.py [--reps 20] [--scale 1.0] [--out profiles/index_timing.jsonl]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

S_FULL, T = 1_000_000, 390
Q_FULL, N_INSTANTS = 64_000_000, 100_000
DAY = 86400000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale S and the timestamp count (a quick look)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20 or a.scale != 1.0, "at least 20 timed calls per case"
    import torch
    from sparkts import _native
    from sparkts import datetimeindex as dti
    _native.ensure_device(0)
    lib = _native.lib()
    with open(_native.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    S = max(64, int(S_FULL * a.scale))
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    fout = open(a.out, "w") if a.out else None
    nan = float("nan")

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def ok(st):
        assert st == 0, lib.sts_last_error()

    def timed(fns, reps):
        """Alternate the callables of `fns`, one event pair per call -> {name: [ms]}"""
        with torch.cuda.stream(side):
            for _ in range(3):
                for fn in fns.values():
                    fn()
            side.synchronize()
            ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
                  for k in fns}
            for i in range(reps):
                for k, fn in fns.items():
                    ev[k][i][0].record(side)
                    fn()
                    ev[k][i][1].record(side)
            side.synchronize()
        return {k: [b.elapsed_time(e) for b, e in v] for k, v in ev.items()}

    def emit(op, ms, nbytes, **extra):
        med = statistics.median(ms)
        rec = {"op": op, "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_max": round(max(ms), 4), "bytes": int(nbytes), "TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
               "lib_sha256": lib_hash}
        rec.update(extra)
        line = json.dumps(rec)
        print(line, flush=True)
        if fout:
            fout.write(line + "\n")
            fout.flush()

    # ---- the copies against fillWithDefault ----
    x = torch.randn((S, T), dtype=torch.float64, device="cuda:0")
    out = torch.empty_like(x)
    j = torch.arange(T, dtype=torch.int64, device="cuda:0")
    ident = j.clone()
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    holes = torch.where(torch.rand(T, device="cuda:0", generator=gen) < 0.05, torch.full_like(j, -1), j)
    torch.cuda.synchronize()
    fns = {"fill_with_default": lambda: ok(lib.sts_fill_with_default(p(x), p(out), S, T, T, T, 0.0, sp))}
    for start in (0, 1, -5):
        fns["rebase_shift_%d" % start] = (lambda s: lambda: ok(lib.sts_rebase_shift(p(x), p(out), S, T, T, T, T, s, nan, sp)))(start)
    fns["rebase_map_identity"] = lambda: ok(lib.sts_rebase_map(p(x), p(out), S, T, T, T, T, p(ident), nan, sp))
    fns["rebase_map_holes5pct"] = lambda: ok(lib.sts_rebase_map(p(x), p(out), S, T, T, T, T, p(holes), nan, sp))
    ms = timed(fns, a.reps)
    base = statistics.median(ms["fill_with_default"])
    for k, v in ms.items():
        emit(k, v, 16 * S * T, S=S, T=T, ratio_to_fill_with_default=round(statistics.median(v) / base, 3))

    # ---- align_uniform: ragged series of mean length T ----
    lengths = torch.randint(0, 2 * T + 1, (S,), dtype=torch.int64, device="cuda:0", generator=gen)
    offsets = torch.zeros(S + 1, dtype=torch.int64, device="cuda:0")
    offsets[1:] = torch.cumsum(lengths, 0)
    total = int(offsets[-1].item())
    del x
    vals = torch.randn((total,), dtype=torch.float64, device="cuda:0")
    starts = torch.randint(-T // 2, T // 2, (S,), dtype=torch.int64, device="cuda:0", generator=gen)
    torch.cuda.synchronize()
    ms = timed({"align_uniform": lambda: ok(lib.sts_align_uniform(p(vals), p(offsets), p(starts), S, T, p(out), T, nan, sp))},
               a.reps)
    emit("align_uniform", ms["align_uniform"], 8 * S * T, S=S, T=T, values=total,
         ratio_to_fill_with_default=round(statistics.median(ms["align_uniform"]) / base, 3))
    del vals, out

    # ---- locAtDateTime: the device against the host path it replaces ----
    n = max(1024, int(Q_FULL * a.scale))
    rng = np.random.default_rng(6)
    bdays = dti.uniform("1990-01-01", periods=N_INSTANTS, freq=dti.BusinessDayFrequency(1))
    inst_b = bdays.toMillisArray()
    inst_i = np.sort(rng.integers(inst_b[0], inst_b[-1], size=N_INSTANTS)) // 1000 * 1000
    for name, inst, index in (("business_days", inst_b, bdays), ("irregular", inst_i, dti.irregular(inst_i))):
        ts = inst[rng.integers(0, N_INSTANTS, size=n)] + rng.integers(0, 2, size=n) * DAY // 2     # half present
        ts_d = torch.as_tensor(ts, device="cuda:0")
        loc = torch.empty_like(ts_d)
        inst_d = index._device_instants(ts_d.device)
        args = index._c_args(inst_d)
        torch.cuda.synchronize()
        ms = timed({"index_locs": lambda: ok(lib.sts_index_locs(p(ts_d), n, *args, p(loc), sp))}, a.reps)
        host = []
        for _ in range(a.host_reps):            # the block of io.timeSeriesRDDFromObservations, and the upload
            t0 = time.perf_counter()
            pos = np.searchsorted(inst, ts)
            pos_c = np.minimum(pos, max(len(inst) - 1, 0))
            h = np.where((len(inst) > 0) & (inst[pos_c] == ts), pos_c, -1).astype(np.int64)
            up = torch.as_tensor(h, device="cuda:0")
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        want = torch.where(loc < 0, torch.full_like(loc, -1), loc)
        assert bool(torch.equal(want, up)), "device and host lookups disagree"
        emit("index_locs_" + name, ms["index_locs"], 16 * n, n=n, instants=N_INSTANTS,
             host_searchsorted_upload_ms_median=round(statistics.median(host), 2),
             host_over_device=round(statistics.median(host) / statistics.median(ms["index_locs"]), 1))
        del ts_d, loc, up, want
    if fout:
        fout.close()


if __name__ == "__main__":
    main()
