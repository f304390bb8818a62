"""Report only: what replicated count draws and the count PIT cost on the device.  A -> B -> C with A measured
and V B counted (tests/count_chain.py), 4 x 30 x 2 cells; engines of the variants alternating in one process, median of 9 calls,
kernel_ms from events.
  bands     HipEngine.predictive_summary's "summary" time: noise=False, noise="family" with the count Poisson, noise="family" with
            it negative binomial, and the ratio to noise=False (all the library could do on such a model before)
  pit       HipEngine.pointwise_summary's "pointwise" time with and without count_pit (negative binomial)
  gaussian  the "summary" time of the same source with every family 0 under noise=True: the kernel instantiation without the
            sampler, for a comparison with another build of the library (SMC_HIP_LIB) on the same box

    python tools/count_draw_bench.py [out.json] [N ...]        (default profiles/count_draw_bench.json, N = 1e5 1e6)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import __graft_entry__ as g
import count_chain as CC

REPEATS = 9


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1][0].isdigit() else os.path.join(ROOT, "profiles", "count_draw_bench.json")
    sizes = [int(float(v)) for v in sys.argv[1:] if v[0].isdigit()] or [100_000, 1_000_000]
    pkg = g.load_package()
    pri = {nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(CC.NAMES, CC.PRIOR_HIGH)}
    gauss_noise = {"additive": [("param", 2), ("fixed", 1.0)], "proportional": [("fixed", 0.0), ("param", 3)]}
    models = {"poisson": ((0, 1), CC.NOISE_POISSON, 0.0), "negbin": ((0, 2), CC.NOISE_NB, CC.B_TRUE), "gaussian": ((0, 0), gauss_noise, CC.B_TRUE)}
    rows = []
    for n in sizes:
        rs = np.random.RandomState(1)
        th = np.ascontiguousarray(CC.THETA_TRUE * np.exp(0.05 * rs.standard_normal((n, 4))))
        engines = {}
        for name, (fam, noise, b) in models.items():
            t, obs = CC.make_data(0, b=b)
            eng = pkg.HipEngine(n, 4, device=0)
            eng.set_prior(pri)
            eng.set_model_user(CC.source(fam), 2, t, obs, cond=CC.COND, noise=noise)
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            engines[name] = eng
        calls = {
            "bands_mean_poisson": lambda: engines["poisson"].predictive_summary(noise=False)["kernel_ms"]["summary"],
            "bands_family_poisson": lambda: engines["poisson"].predictive_summary(noise="family", seed=1)["kernel_ms"]["summary"],
            "bands_mean_negbin": lambda: engines["negbin"].predictive_summary(noise=False)["kernel_ms"]["summary"],
            "bands_family_negbin": lambda: engines["negbin"].predictive_summary(noise="family", seed=1)["kernel_ms"]["summary"],
            "bands_gaussian_noise_true": lambda: engines["gaussian"].predictive_summary(noise=True, seed=1)["kernel_ms"]["summary"],
            "pit_without": lambda: engines["negbin"].pointwise_summary()["kernel_ms"]["pointwise"],
            "pit_with_count_pit": lambda: engines["negbin"].pointwise_summary(count_pit=True, seed=1)["kernel_ms"]["pointwise"],
        }
        for f in calls.values():                                     # warm-up: the prediction kernel's first launch
            f()
        ms = {k: [] for k in calls}
        for _ in range(REPEATS):                                     # alternating
            for k, f in calls.items():
                ms[k].append(f())
        for eng in engines.values():
            eng.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        row = {"n": n, "cells": 240, "repeats": REPEATS, "median_kernel_ms": med, "min_max_kernel_ms": {k: [float(min(v)), float(max(v))] for k, v in ms.items()},
               "ratio_family_to_mean": {"poisson": med["bands_family_poisson"] / med["bands_mean_poisson"],
                                        "negbin": med["bands_family_negbin"] / med["bands_mean_negbin"]},
               "ratio_count_pit": med["pit_with_count_pit"] / med["pit_without"]}
        rows.append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": "MI355X", "library": os.environ.get("SMC_HIP_LIB", "in-tree"),
                   "model": "A -> B -> C, A Gaussian and V B a count, 4 x 30 x 2 cells (tests/count_chain.py)", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
