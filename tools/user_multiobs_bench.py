"""Cost of a second observed output (include/smc_hip.h: smc_set_model_user3): solves/s of the likelihood sweep of the one-output
and the two-output consecutive-reaction model (RK45) and of ROBERTSON against ROBERTSON_AC (BDF), same particles and data times.
Usage: python tools/user_multiobs_bench.py [n_particles]   (one JSON line per model)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

import __graft_entry__ as g
import robertson_bdf_bound as RB

pkg = g.load_package()
um = pkg.user_models
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
rs = np.random.RandomState(0)
n_ex, n_t = 4, 30
t = np.tile(np.linspace(0.0, 10.0, n_t), (n_ex, 1))
A0 = np.array([1.0, 2.0, 0.5, 1.5])
obs2 = rs.uniform(0, 1, (n_ex, n_t, 2))
th_ab = np.column_stack([0.8 * (1 + 0.1 * rs.standard_normal(n)), 0.3 * (1 + 0.1 * rs.standard_normal(n)), rs.uniform(0.005, 0.05, n)])
_, obs_rob = RB.population(n=1)
th_rob = np.column_stack([RB.K_TRUE[0] * 10.0 ** rs.uniform(-1, 1, n), RB.K_TRUE[1] * 10.0 ** rs.uniform(-1, 1, n), rs.uniform(0.005, 0.05, n)])
obs_rob2 = np.stack([np.full_like(obs_rob, 0.5), obs_rob], axis=2)
cases = [("CONSECUTIVE_REACTIONS", um.CONSECUTIVE_REACTIONS, 2, t, obs2[..., 1], A0, th_ab, {}),
         ("CONSECUTIVE_REACTIONS_AB", um.CONSECUTIVE_REACTIONS_AB, 2, t, obs2, A0, th_ab, {}),
         ("ROBERTSON", um.ROBERTSON, 3, RB.T, obs_rob, RB.A0, th_rob, dict(rtol=RB.RTOL, atol=RB.ATOL, method="BDF")),
         ("ROBERTSON_AC", um.ROBERTSON_AC, 3, RB.T, obs_rob2, RB.A0, th_rob, dict(rtol=RB.RTOL, atol=RB.ATOL, method="BDF", obs_scale=(1.0, 0.02)))]
for name, src, ns, tt, obs, a0, th, kw in cases:
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior({"a": {"dist": "uniform", "low": 0, "high": 1e9}, "b": {"dist": "uniform", "low": 0, "high": 1e9},
                       "s": {"dist": "uniform", "low": 0, "high": 1}})
        eng.set_model_user(src, ns, tt, obs, cond=a0[:, None], **kw)
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        eng.loglik(pkg.SMC_SET_PRED)
        times = []
        for _ in range(5):
            eng.synchronize()
            t0 = time.perf_counter()
            info = eng.loglik(pkg.SMC_SET_PRED)
            eng.synchronize()
            times.append(time.perf_counter() - t0)
        dt = float(np.median(times))
        print(json.dumps({"model": name, "n_obs": 1 if obs.ndim == 2 else obs.shape[2], "particles": n, "experiments": tt.shape[0],
                          "median_s": round(dt, 5), "solves_per_s": round(n * tt.shape[0] / dt), "rk_attempts": info["rk_attempts"],
                          "n_failed": info["n_failed"]}), flush=True)
