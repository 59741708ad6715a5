#!/usr/bin/env python3
"""Time the samplers of include/sts_sample.h at 1 M x 390: one JSON line per case with the median /
min ms, the bytes the result needs (S x n doubles written; the parameter arrays are noise) and the
achieved TB/s over the median, and the library's sha256.

  sample_normal          the raw panel of draws
  garch_sample           the fused GARCHModel.sample kernel
  argarch_sample         the fused ARGARCHModel.sample kernel
  normal_then_garch_add  sts_sample_normal into a panel + in-place sts_garch_add: the yardstick.  It is
                         NOT the same array (addTimeDependentEffects is another recurrence than
                         sampleWithVariances) but the same work done in two passes: the draws written,
                         read back and written again, three times the fused kernel's bytes.

The three GARCH cases are timed in the SAME process, alternating call by call.  HIP events around
every call on one side stream, every case warmed up first, --reps timed calls per case (>= 20 at
full scale).

    python tools/sample_timing.py [--reps 20] [--scale 1.0] [--out profiles/sample_timing.jsonl]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

S_FULL, N = 1_000_000, 390
SEED = 2024


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

    def ok(st):
        assert st == 0, lib.sts_last_error()

    out = torch.empty((S, N), dtype=torch.float64, device="cuda:0")
    two = torch.empty_like(out)
    # a spread of stationary models, one per series
    gen = torch.Generator(device="cuda:0").manual_seed(SEED)
    u = torch.rand((5, S), dtype=torch.float64, device="cuda:0", generator=gen)
    om, al, be = (0.05 + 0.25 * u[0]).contiguous(), (0.05 + 0.4 * u[1]).contiguous(), (0.05 + 0.4 * u[2]).contiguous()
    c, phi = (u[3] - 0.5).contiguous(), (0.8 * (u[4] - 0.5)).contiguous()
    torch.cuda.synchronize()
    tail = (0, ctypes.c_uint64(SEED), sp)

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
        rec = {"op": op, "S": S, "n": N, "reps": len(ms), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_max": round(max(ms), 4), "bytes": int(nbytes), "TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
               "Gdraws_per_s": round(S * N / (med * 1e-3) / 1e9, 2), "lib_sha256": lib_hash}
        rec.update(extra)
        line = json.dumps(rec)
        print(line, flush=True)
        if fout:
            fout.write(line + "\n")
            fout.flush()

    need = 8 * S * N
    ms = timed({"sample_normal": lambda: ok(lib.sts_sample_normal(p(out), 0, S, N, N, *tail))}, a.reps)
    emit("sample_normal", ms["sample_normal"], need)

    def fused():
        ok(lib.sts_garch_sample(p(out), 0, S, N, N, p(om), p(al), p(be), *tail))

    def fused_ar():
        ok(lib.sts_argarch_sample(p(out), 0, S, N, N, p(c), p(phi), p(om), p(al), p(be), *tail))

    def two_calls():
        ok(lib.sts_sample_normal(p(two), 0, S, N, N, *tail))
        ok(lib.sts_garch_add(p(two), p(two), S, N, N, N, p(om), p(al), p(be), sp))

    ms = timed({"garch_sample": fused, "argarch_sample": fused_ar, "normal_then_garch_add": two_calls}, a.reps)
    base = statistics.median(ms["normal_then_garch_add"])
    for k, moved in (("garch_sample", need), ("argarch_sample", need), ("normal_then_garch_add", 3 * need)):
        emit(k, ms[k], need, bytes_route_moves=int(moved), ratio_to_two_calls=round(statistics.median(ms[k]) / base, 3))
    if fout:
        fout.close()


if __name__ == "__main__":
    main()
