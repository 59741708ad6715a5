#!/usr/bin/env python3
"""Time sts_cross_moments (include/sts_cross.h) next to what a user does today, torch on the same
device tensor in the same process, alternating call by call:

  sym_c1      the symmetric covariance at the C1 shape, 10 000 x 2 520      vs torch.cov(x)
  sym_long    the symmetric covariance at 1 000 x 100 000 (the split plan)  vs torch.cov(x)
  cross_k8    10 000 series x 2 520 against 8 factors                        vs the centred matmul
                                                                             (x - mean) @ (f - mean).T / (T - 1)

HIP events around every call, every shape warmed up first, --reps timed calls per case (>= 20), the
shader clock (rocm-smi --showclocks, read only) noted before and after each case.  One JSON line per
case: median / min ms, torch's, their ratio, achieved FLOP/s over the algorithmic operations
(Sx Sy T 2, halved for the symmetric form, which computes one triangle), its share of the 73 TF/s
FP64 MFMA rate measured with register operands, the largest difference from
torch's result in units of the bar, and the library's sha256.

    python tools/cross_timing.py [--reps 20] [--out profiles/cross_timing.jsonl] [--append] [--scale 1.0]
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

PIPE_TFLOPS = 73.0


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def sclk():
    """the current shader clock as rocm-smi prints it (MHz), or None"""
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
    except (OSError, subprocess.SubprocessError):
        return None
    m = re.search(r"sclk clock level:?\s*\d*:?\s*\(?(\d+)\s*Mhz", text, flags=re.I)
    return int(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--scale", type=float, default=1.0, help="scale the series counts (a quick look)")
    a = ap.parse_args()
    assert a.reps >= 20 or a.scale != 1.0, "at least 20 timed calls per case"
    import torch
    from sparkts import _native
    _native.ensure_device(0)
    lib = _native.lib()
    lib_hash = sha(_native.LIB_PATH)
    sp = torch.cuda.current_stream().cuda_stream
    out_f = open(a.out, "a" if a.append else "w") if a.out else None

    def timed_pair(fn, yard, reps):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
        for _ in range(3):
            fn()
            yard()
        torch.cuda.synchronize()
        for e in ev:
            e[0].record()
            fn()
            e[1].record()
            e[2].record()
            yard()
            e[3].record()
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in ev], [e[2].elapsed_time(e[3]) for e in ev]

    med = lambda v: sorted(v)[len(v) // 2]
    scaled = lambda s: max(1, int(s * a.scale))
    for name, Sx, T, Sy in (("sym_c1", scaled(10_000), 2520, 0), ("sym_long", scaled(1_000), 100_000, 0),
                            ("cross_k8", scaled(10_000), 2520, 8)):
        x = torch.empty((Sx, T), dtype=torch.float64, device="cuda")
        assert lib.sts_gen_panel(x.data_ptr(), 0, Sx, T, T, 6, 0.0, sp) == 0
        y = torch.randn((Sy, T), dtype=torch.float64, device="cuda") if Sy else None
        cols = Sy or Sx
        out = torch.empty((Sx, cols), dtype=torch.float64, device="cuda")
        keep = {}

        def ours():
            st = lib.sts_cross_moments(x.data_ptr(), Sx, T, T, y.data_ptr() if Sy else None, Sy, T, 0, out.data_ptr(), cols,
                                       None, None, sp)
            assert st == 0, lib.sts_last_error()

        def theirs():
            if Sy:
                keep["t"] = (x - x.mean(dim=1, keepdim=True)) @ (y - y.mean(dim=1, keepdim=True)).T / (T - 1)
            else:
                keep["t"] = torch.cov(x)

        clk0 = sclk()
        ms, yms = timed_pair(ours, theirs, a.reps)
        clk1 = sclk()
        # the two results, in the bar's unit (sqrt(C_ii C_jj) / (T - 1)); torch's own rounding is in there
        vx = x.var(dim=1)
        vy = y.var(dim=1) if Sy else vx
        diff = float(((out - keep["t"]).abs() / (vx[:, None] * vy[None, :]).sqrt()).max())
        flop = 2.0 * Sx * cols * T * (0.5 if not Sy else 1.0)
        tf = flop / (med(ms) * 1e-3) / 1e12
        rec = {"case": name, "Sx": Sx, "Sy": Sy, "T": T, "reps": a.reps, "ms_median": med(ms), "ms_min": min(ms),
               "yardstick": "centred matmul (torch)" if Sy else "torch.cov", "yard_ms_median": med(yms), "yard_ms_min": min(yms),
               "ratio_to_yardstick": med(ms) / med(yms), "TFLOPs": tf, "share_of_73_TFLOPs": tf / PIPE_TFLOPS,
               "max_diff_from_torch_in_bar_units": diff, "sclk_MHz_before": clk0, "sclk_MHz_after": clk1,
               "lib_sha256": lib_hash}
        line = json.dumps(rec)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()
        del x, y, out, keep, vx, vy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
