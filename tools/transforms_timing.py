#!/usr/bin/env python3
"""Time the panel transforms of include/sts_transforms.h on the C2 shape (1 M x 390, lag 1, an
sts_gen_panel panel with 5 % NaN): one JSON line per operator with the median / min ms, the bytes
the operator has to move (panel elements read + output elements written, from the shapes) and the
achieved TB/s over the median, and the library's sha256.

For the fused fill("previous") -> returnRates call, three routes to the same array are timed in
the SAME process, alternating call by call:

  fused        sts_fill_quotients(previous, lag 1, minus one): the one-pass kernel
  two_calls    sts_fill("previous") into a panel, then sts_quotients on it (this build's composition)
  parent       sts_fill("previous"), then the torch expression x[:, 1:] / x[:, :-1] - 1 (the only
               route before this header existed)

and their outputs are compared bit for bit (NaN where NaN) before anything is timed.

HIP events around every call on one side stream, every case warmed up first, --reps timed calls
per case (>= 20 at full scale).

    python tools/transforms_timing.py [--reps 20] [--scale 1.0] [--out profiles/transforms_timing.jsonl]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

S_FULL, T = 1_000_000, 390
PREVIOUS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="scale S (a quick look on a busy machine)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20 or a.scale != 1.0, "at least 20 timed calls per case"
    import torch
    from sparkts import _native
    _native.ensure_device(0)
    lib = _native.lib()
    with open(_native.LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    S = max(64, int(S_FULL * a.scale))
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    fout = open(a.out, "w") if a.out else None

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def new(*shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device="cuda:0")

    x = new(S, T)
    assert lib.sts_gen_panel(p(x), 0, S, T, T, 2024, 0.05, None) == 0
    torch.cuda.synchronize()
    x += 100.0                                    # price levels: no zero divisors in the timed data
    torch.cuda.synchronize()

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
        rec = {"op": op, "S": S, "T": T, "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_max": round(max(ms), 4), "bytes": int(nbytes), "TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
               "lib_sha256": lib_hash}
        rec.update(extra)
        line = json.dumps(rec)
        print(line, flush=True)
        if fout:
            fout.write(line + "\n")
            fout.flush()

    def ok(st):
        assert st == 0, lib.sts_last_error()

    E = 8 * S                                     # bytes per panel column
    err = new(S, dtype=torch.int32)
    o = new(S, 2 * T)                             # the widest output (upsample by 2)
    first, last = new(S, dtype=torch.int64), new(S, dtype=torch.int64)
    y = x.clone()

    singles = [
        ("quotients", lambda: ok(lib.sts_quotients(p(x), p(o), S, T, T, T - 1, 1, 0, sp)), E * (T + T - 1)),
        ("price2ret", lambda: ok(lib.sts_quotients(p(x), p(o), S, T, T, T - 1, 1, 1, sp)), E * (T + T - 1)),
        ("fill_with_default", lambda: ok(lib.sts_fill_with_default(p(x), p(o), S, T, T, T, 0.0, sp)), E * 2 * T),
        ("downsample_n2", lambda: ok(lib.sts_downsample(p(x), p(o), S, T, T, T // 2, 2, 0, sp)), E * (T // 2) * 2),
        ("upsample_n2", lambda: ok(lib.sts_upsample(p(x), p(o), S, T, T, 2 * T, 2, 0, 0, sp)), E * 3 * T),
        ("first_last_not_nan", lambda: ok(lib.sts_first_last_not_nan(p(x), S, T, T, p(first), p(last), sp)), None),
        ("inverse_diff_at_lag_1", lambda: ok(lib.sts_inverse_diff_at_lag(p(x), p(o), S, T, T, T, 1, 1, sp)), E * 2 * T),
        ("inverse_diff_at_lag_1_inplace", lambda: ok(lib.sts_inverse_diff_at_lag(p(y), p(y), S, T, T, T, 1, 1, sp)), E * 2 * T),
        ("diff_order_d_2", lambda: ok(lib.sts_diff_order_d(p(x), p(o), S, T, T, T, 2, sp)), E * 2 * T),
        ("inverse_diff_order_d_2", lambda: ok(lib.sts_inverse_diff_order_d(p(x), p(o), S, T, T, T, 2, sp)), E * 2 * T),
    ]
    for op, fn, nbytes in singles:
        if op == "inverse_diff_at_lag_1_inplace":
            y.copy_(x)
            y.nan_to_num_(nan=0.0)
            y *= 1e-3                              # a running sum of it stays finite over the timed calls
            torch.cuda.synchronize()
        ms = timed({op: fn}, a.reps)[op]
        if nbytes is None:                        # the 128-byte lines the two scans touch, counted from the results
            torch.cuda.synchronize()
            f, l = first.cpu().numpy(), last.cpu().numpy()
            steps = (np.minimum(f // 64 + 1, -(-T // 64)) + np.minimum((T - 1 - l) // 64 + 1, -(-T // 64))) * 64
            nbytes = int(steps.sum()) * 8 + 16 * S
        emit(op, ms, nbytes)

    # ---- the fused call against the two other routes to the same array ----
    filled = new(S, T)
    r_fused, r_two, r_parent = new(S, T - 1), new(S, T - 1), None

    def fused():
        ok(lib.sts_fill_quotients(p(x), p(r_fused), S, T, T, T - 1, PREVIOUS, 1, 1, p(err), sp))

    def two_calls():
        ok(lib.sts_fill(p(x), p(filled), S, T, T, T, PREVIOUS, p(err), sp))
        ok(lib.sts_quotients(p(filled), p(r_two), S, T, T, T - 1, 1, 1, sp))

    def parent():
        nonlocal r_parent
        ok(lib.sts_fill(p(x), p(filled), S, T, T, T, PREVIOUS, p(err), sp))
        r_parent = filled[:, 1:] / filled[:, :-1] - 1

    with torch.cuda.stream(side):
        fused(), two_calls(), parent()
        side.synchronize()
        for name, r in (("two_calls", r_two), ("parent", r_parent)):
            same = (r.view(torch.int64) == r_fused.view(torch.int64)) | (r.isnan() & r_fused.isnan())
            assert bool(same.all()), "%s differs from the fused call" % name
    ms = timed({"fused": fused, "two_calls": two_calls, "parent": parent}, a.reps)
    need = E * (T + T - 1)                        # what the result needs: the panel read, the returns written
    moved = {"fused": need, "two_calls": E * (2 * T + T + T - 1),
             "parent": E * (2 * T + 2 * (T - 1) + 2 * (T - 1))}      # fill; divide (2 reads, 1 write, L2 aside); subtract
    for k in ("fused", "two_calls", "parent"):
        emit("fill_previous_return_rates/" + k, ms[k], need, bytes_route_moves=int(moved[k]),
             ratio_to_fused=round(statistics.median(ms[k]) / statistics.median(ms["fused"]), 3))
    if fout:
        fout.close()


if __name__ == "__main__":
    main()
