"""Record the optimizer paths of the EWMA, GARCH and ARIMA fits into tests/golden/cg_paths.json
(test infrastructure only).

    python tests/golden/make_cg_paths.py        # rewrites cg_paths.json from the checked-out tree

The three host harnesses (tests/native/{ewma,garch,arima}_sm_harness.cpp) run the very state
machines the device kernels run and print, per series, status, point bits, commons-math3's
evaluation count and the number of real passes over the series.  The state-machine tests compare
the first three with the straight-line optimizers; the passes are what the evaluation caches
decide, and nothing else pins them.  This file records the complete lines for the inputs those
tests already use (each test module's path_cases()), and one test per module requires the
harness to reproduce them character for character.

A recording states the commit it was made from (the tree must be clean, so that the commit names
the code that ran).  Re-record only when a change is MEANT to alter an optimizer's path; a
refactor must reproduce the file as it stands.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "spark-timeseries_amd")]

import test_arima  # noqa: E402
import test_ewma_state_machine as test_ewma  # noqa: E402
import test_garch  # noqa: E402


def recorded_from():
    """the commit whose csrc/ and harnesses ran, refusing a tree that differs from it there"""
    code = ["spark-timeseries_amd/csrc", "include", "tests/native", "oracle"]
    if subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", *code]).returncode != 0:
        sys.exit("the optimizer sources differ from HEAD: commit or stash them before recording")
    return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()


def main():
    gxx = shutil.which("g++")
    if gxx is None:
        sys.exit("g++ not available")
    doc = {"recorded_from": recorded_from(),
           "format": {"ewma": "status smoothing_bits evaluations passes",
                      "garch": "status omega_bits alpha_bits beta_bits evaluations passes",
                      "arima": "status coefficient_bits... evaluations passes"}}
    with tempfile.TemporaryDirectory() as d:
        for name, mod in (("ewma", test_ewma), ("garch", test_garch), ("arima", test_arima)):
            exe = os.path.join(d, name + "_sm")
            mod.build_harness(gxx, exe)
            doc[name] = {}
            for case, args in mod.path_cases().items():
                if name == "arima":
                    p, q, icpt, y, init = args
                    doc[name][case] = mod.harness_lines(exe, p, q, icpt, y[None, :], init[None, :])
                else:
                    doc[name][case] = mod.harness_lines(exe, args)
    with open(os.path.join(HERE, "cg_paths.json"), "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
