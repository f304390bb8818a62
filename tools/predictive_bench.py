"""Posterior predictive summaries (include/smc_hip.h: smc_user_predict_summary) against the route they replace, on one box in
one call: CONSECUTIVE_REACTIONS_ABC, N particles resident on the device, the 4 x 30 data design and a 4 x 200 design.

  new     HipEngine.predictive_summary: wall time of the call and its split (kernel_ms) into prediction sweeps and summary kernels
  parent  download the set, predict_user of it, np.nanmean / nanstd / nanquantile("lower", "higher") over the particle axis on
          the usable CPUs (a thread per block of cells).  predict_user knows the data's design only, so the 4 x 200 design is
          reached the old way: the model set again with the grid as all-NaN "data"; above 2e5 particles one experiment at a time,
          which keeps the host array of predictions below 5 GB

Usage: python tools/predictive_bench.py [--sizes 100000,1000000] [--out profiles/predictive_summary_bench.json]
Every step runs in a process of its own under its own time limit; the first step that fails or runs out of time ends the run
(what was measured until then is still written).  --step is the child's entry."""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PROBS = (0.025, 0.5, 0.975)
LIMITS = {"new": 180, "parent": 300}        # seconds per step


def designs():
    t = np.tile(np.linspace(0.0, 10.0, 30), (4, 1))
    A0 = np.array([1.0, 2.0, 0.5, 1.5])
    return {"data_4x30": (t, A0[:, None]), "grid_4x200": (np.tile(np.linspace(0.0, 15.0, 200), (4, 1)), np.array([[0.75], [1.25], [2.75], [4.0]]))}


def population(n):
    rs = np.random.RandomState(0)      # a posterior-like cloud around the generating constants
    return np.column_stack([0.8 * (1 + 0.02 * rs.standard_normal(n)), 0.3 * (1 + 0.02 * rs.standard_normal(n)), rs.uniform(0.008, 0.012, n)])


def usable_cpus():
    n = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, round(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    return min(n, 16)


def host_summary(pred, workers):
    """pred (n, cells): the parent's reduction, a thread per block of cells."""
    cells = pred.shape[1]
    edges = np.linspace(0, cells, min(workers, cells) + 1).astype(int)

    def one(k):
        x = pred[:, edges[k]:edges[k + 1]]
        return (np.nanmean(x, axis=0), np.nanstd(x, axis=0), np.nanquantile(x, PROBS, axis=0, method="lower"),
                np.nanquantile(x, PROBS, axis=0, method="higher"))
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(one, range(len(edges) - 1)))
    return [np.concatenate([p[i] for p in parts], axis=-1) for i in range(4)]


def step(which, n, design):
    import __graft_entry__ as g
    pkg = g.load_package()
    t, cond = designs()["data_4x30"]
    t_new, cond_new = designs()[design]
    is_data = design == "data_4x30"
    th = population(n)
    priors = {"k1": {"dist": "uniform", "low": 0, "high": 3}, "k2": {"dist": "uniform", "low": 0, "high": 3},
              "sigma": {"dist": "uniform", "low": 0, "high": 1}}
    res = {"path": which, "particles": n, "design": design, "cells": int(t_new.size * 3)}
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(priors)

        def set_model(tt, cc):
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_ABC, 2, tt, np.full(tt.shape + (3,), np.nan), cond=cc,
                               obs_scale=(1.0, 3.0, 1.0))
        set_model(t, cond)
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        if which == "new":
            kw = {} if is_data else {"t": t_new, "cond": cond_new}
            eng.predictive_summary(probs=PROBS, **kw)          # first call: allocations, lazy initialisation
            runs = []
            for _ in range(3):
                eng.synchronize()
                t0 = time.perf_counter()
                out = eng.predictive_summary(probs=PROBS, **kw)
                runs.append((time.perf_counter() - t0, out["kernel_ms"]["predict"], out["kernel_ms"]["summary"]))
            runs.sort()
            wall, pms, sms = runs[1]
            res.update({"wall_s": round(wall, 4), "predict_kernel_ms": round(pms, 3), "summary_kernel_ms": round(sms, 3),
                        "walls_s": [round(r[0], 4) for r in runs], "n_failed": out["n_failed"],
                        "summary_ns_per_cell_particle": round(sms * 1e6 / (res["cells"] * n), 4),
                        "median_checksum": float(np.nansum(out["quantile"][1]))})
        else:
            workers = usable_cpus()
            eng.synchronize()
            t0 = time.perf_counter()
            particles = eng.download_particles(pkg.SMC_SET_FILT)
            rows = [slice(0, 4)] if n <= 200_000 else [slice(e, e + 1) for e in range(4)]
            t_predict = t_reduce = 0.0
            med = []
            for r in rows:
                t1 = time.perf_counter()
                if not (is_data and len(rows) == 1):
                    set_model(t_new[r], cond_new[r])         # the old way to another design: all-NaN "data"
                _, pred, info = eng.predict_user(particles)
                t2 = time.perf_counter()
                _, _, lower, upper = host_summary(pred.reshape(n, -1), workers)
                med.append(lower[1])
                t_predict += t2 - t1
                t_reduce += time.perf_counter() - t2
                del pred
            res.update({"wall_s": round(time.perf_counter() - t0, 3), "predict_and_copy_s": round(t_predict, 3),
                        "numpy_reduce_s": round(t_reduce, 3), "cpu_threads": workers, "host_array_gb": round(n * t_new[rows[0]].size * 3 * 8 / 1e9, 2),
                        "n_failed": info["n_failed"], "median_checksum_lower": float(np.nansum(np.concatenate(med)))})
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_summary_bench.json"))
    ap.add_argument("--step", nargs=3, metavar=("PATH", "N", "DESIGN"))
    a = ap.parse_args()
    if a.step:
        return step(a.step[0], int(a.step[1]), a.step[2])
    results, note = [], "complete"
    for n in [int(x) for x in a.sizes.split(",")]:
        for design in designs():
            for which in ("new", "parent"):
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", which, str(n), design], capture_output=True,
                                       text=True, timeout=LIMITS[which])
                except subprocess.TimeoutExpired:
                    note = f"stopped: {which} {n} {design} exceeded {LIMITS[which]} s"
                    break
                line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    note = f"stopped: {which} {n} {design} exited with {r.returncode}: {r.stderr[-400:]}"
                    break
                results.append(json.loads(line[-1][7:]))
                print(line[-1][7:], flush=True)
            else:
                continue
            break
        else:
            continue
        break
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/predictive_bench.py", "model": "CONSECUTIVE_REACTIONS_ABC", "probs": PROBS, "status": note,
                   "results": results}, f, indent=1)
        f.write("\n")
    print(note)
    return 0 if note == "complete" else 1


if __name__ == "__main__":
    sys.exit(main())
