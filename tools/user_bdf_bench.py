"""Throughput of a BDF user model (method="BDF", include/smc_hip.h) against SciPy: Robertson's kinetics (user_models.ROBERTSON,
analytic Jacobian) at n particles x 4 experiments on the GPU, next to solve_ivp(method="BDF") on 16 CPU processes over a
subsample of the same particles.  Prints one JSON line.

    python tools/user_bdf_bench.py [n_particle] [n_cpu_subsample]

fp64_share: the Newton iterations and LU factorisations the device counted, at their algorithmic FP64 operation counts for
NS = 3 (a Newton iteration: the residual c f - psi - d, the LU solve, the scaled norm and the update - 2 NS^2 + 8 NS; an LU
factorisation: I - c J and the elimination - 2 NS^2 + 2 NS^3 / 3 rounded up to whole operations), over the 78.6 TFLOP/s
FP64 peak - the user's own right-hand side and Jacobian are not counted."""
import json
import multiprocessing
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import __graft_entry__ as g
import robertson_bdf_bound as RB

NS = 3
FLOPS_NEWTON = 2 * NS * NS + 8 * NS
FLOPS_LU = 2 * NS * NS + (2 * NS ** 3 + 2) // 3
PEAK = 78.6e12


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    n_cpu = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    pkg = g.load_package()
    _, obs = RB.population(n=1)
    rs = np.random.RandomState(7)
    th = np.column_stack([RB.K_TRUE[0] * 10.0 ** rs.uniform(-1, 1, n), RB.K_TRUE[1] * 10.0 ** rs.uniform(-1, 1, n),
                          rs.uniform(0.005, 0.05, n)])
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior({"k1": {"dist": "uniform", "low": 0, "high": 1}, "k3": {"dist": "uniform", "low": 0, "high": 1e6},
                       "sigma": {"dist": "uniform", "low": 0, "high": 1}})
        eng.set_model_user(pkg.user_models.ROBERTSON, 3, RB.T, obs, cond=RB.A0[:, None], rtol=RB.RTOL, atol=RB.ATOL, method="BDF")
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        eng.loglik(pkg.SMC_SET_PRED)                 # warm-up
        eng.synchronize()
        reps, t0 = 3, time.perf_counter()
        for _ in range(reps):
            info = eng.loglik(pkg.SMC_SET_PRED)
        eng.synchronize()
        dt = (time.perf_counter() - t0) / reps
        ctr = eng.user_sweep_counters()
        dev = eng.device_info()
    solves = n * len(RB.A0)
    sub = th[:n_cpu]
    n_proc = min(16, len(os.sched_getaffinity(0)))
    with ProcessPoolExecutor(max_workers=n_proc, mp_context=multiprocessing.get_context("spawn")) as ex:
        list(ex.map(RB.scipy_row, [(a, b, True) for a, b, _ in sub[:n_proc]]))      # start-up of the workers
        t0 = time.perf_counter()
        rows = list(ex.map(RB.scipy_row, [(a, b, True) for a, b, _ in sub], chunksize=4))
        dt_cpu = time.perf_counter() - t0
    flops = ctr["newton_iters"] * FLOPS_NEWTON + ctr["lu_factorisations"] * FLOPS_LU
    print(json.dumps({
        "workload": "robertson_bdf_loglik", "device": dev["name"], "arch": dev["arch"], "n_particle": n, "n_ex": len(RB.A0),
        "rtol": RB.RTOL, "atol": RB.ATOL, "gpu_sweep_s": dt, "gpu_solves_per_s": solves / dt, "n_failed": info["n_failed"],
        "step_attempts": info["rk_attempts"], "steps": ctr["steps"], "newton_iters": ctr["newton_iters"],
        "lu_factorisations": ctr["lu_factorisations"], "jacobian_evals": ctr["jacobian_evals"],
        "fp64_tflops_algorithmic": flops / dt / 1e12, "fp64_share": flops / dt / PEAK,
        "cpu_scipy_bdf_processes": n_proc, "cpu_subsample_particles": len(sub),
        "cpu_solves_per_s": len(sub) * len(RB.A0) / dt_cpu, "cpu_steps_per_solve": sum(r[1] for r in rows) / (len(sub) * len(RB.A0)),
        "speedup": (solves / dt) / (len(sub) * len(RB.A0) / dt_cpu)}))


if __name__ == "__main__":
    main()
