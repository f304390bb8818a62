"""Report only: what the per-observation statistics of a resident posterior cost on the device (HipEngine.pointwise_summary:
kernel_ms split into the prediction sweep and the pointwise kernels) against the way without them - download the set,
predict_user of it, user_models.pointwise_loglik / pointwise_stats in NumPy on 16 threads (blocks of particles, merged with
pointwise_merge).  A -> B -> C with A and B measured on the 4 x 30 data design of tests/noise_model_chain.py.

    python tools/pointwise_bench.py [out.json] [N ...]        (default profiles/pointwise_summary_bench.json, N = 1e5 1e6)"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import __graft_entry__ as g
import noise_model_chain as NC

THREADS, BLOCK = 16, 12_500


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pointwise_summary_bench.json")
    sizes = [int(float(v)) for v in sys.argv[2:]] or [100_000, 1_000_000]
    pkg = g.load_package()
    um = pkg.user_models
    t, obs = NC.make_data(0)
    pri = {k: {"dist": "uniform", "low": 0, "high": 3} for k in ("k1", "k2", "a0", "a1", "b0")}
    rows = []
    for n in sizes:
        rs = np.random.RandomState(1)
        th = NC.THETA_TRUE * (1.0 + 0.05 * rs.standard_normal((n, 5)))
        with pkg.HipEngine(n, 5, device=0) as eng:
            eng.set_prior(pri)
            eng.set_model_user(um.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], noise=NC.NOISE)
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.pointwise_summary()                                  # warm-up: the prediction kernel's first launch
            best = None
            for _ in range(3):
                t0 = time.perf_counter()
                dev = eng.pointwise_summary()
                wall = time.perf_counter() - t0
                if best is None or wall < best[0]:
                    best = (wall, dev)
            wall, dev = best
            t0 = time.perf_counter()
            down = eng.download_particles(pkg.SMC_SET_FILT)
            _, pred, _ = eng.predict_user(down)
            t_pred = time.perf_counter() - t0

        def block(lo):
            ll = um.pointwise_loglik(pred[lo:lo + BLOCK], t, obs, down[lo:lo + BLOCK], NC.NOISE)
            return um.pointwise_stats(ll)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(THREADS) as pool:
            host = um.pointwise_merge(list(pool.map(block, range(0, n, BLOCK))))
        t_host = time.perf_counter() - t0
        seen = dev["n"] > 0
        rows.append({"n": n, "cells": int(obs.size), "device_kernel_ms": dev["kernel_ms"], "device_wall_s": wall,
                     "host_download_and_predict_s": t_pred, "host_numpy_terms_and_stats_s": t_host, "host_threads": THREADS,
                     "bytes_over_the_bus_host_way": int(pred.nbytes + down.nbytes),
                     "max_abs_lpd_difference": float(np.max(np.abs(dev["lpd"][seen] - host["lpd"][seen])))})
        print(json.dumps(rows[-1]))
    with open(out_path, "w") as f:
        json.dump({"device": "MI355X", "model": "CONSECUTIVE_REACTIONS_AB, noise model, 4 x 30 x 2 cells", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
