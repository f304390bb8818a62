"""A STIFF model of your own: Robertson's kinetics (A -> B, B + B -> C + B, B + C -> A + C; k2 = 3e7 fixed), the product C
observed in four experiments, k1, k3 and sigma estimated.  Explicit RK45 would run on its stability limit here (tens of
thousands of step attempts per solve), so the model is set with method="BDF" and its analytic Jacobian.

    python examples/stiff_user_model_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scipy.integrate import solve_ivp

import __graft_entry__ as g

pkg = g.load_package()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32_768
rs = np.random.RandomState(0)
t = np.tile(np.linspace(0.0, 40.0, 30), (4, 1))
A0 = np.array([1.0, 0.5, 2.0, 1.5])
k1, k3, sigma = 0.04, 1e4, 0.01
rtol, atol = 1e-4, 1e-8


def rhs(_t, y):
    return [-k1 * y[0] + k3 * y[1] * y[2], k1 * y[0] - k3 * y[1] * y[2] - 3e7 * y[1] ** 2, 3e7 * y[1] ** 2]


C = np.array([solve_ivp(rhs, [0.0, 40.0], [a, 0.0, 0.0], method="BDF", t_eval=t[0], rtol=1e-8, atol=1e-12).y[2] for a in A0])
obs = C + sigma * rs.standard_normal(C.shape)
priors = {"k1": {"dist": "uniform", "low": 0, "high": 0.2}, "k3": {"dist": "uniform", "low": 0, "high": 5e4},
          "sigma": {"dist": "uniform", "low": 0, "high": 0.1}}
with pkg.HipEngine(n, 3, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(pkg.user_models.ROBERTSON, n_states=3, t=t, obs=obs, cond=A0[:, None], rtol=rtol, atol=atol, method="BDF")
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors, rtol=rtol, atol=atol), rng="device", verbose=True)
    work = eng.user_sweep_counters()
print("posterior mean", out["p_pred"].mean(axis=0), "sd", out["p_pred"].std(axis=0), "(generated with", (k1, k3, sigma), ")")
print("last sweep:", work)
