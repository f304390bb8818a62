"""STATE-TRIGGERED EVENTS: a level that decays, dC/dt = -k C, and is re-dosed by D whenever it falls to a threshold L - a controller
that keeps a trough.  When the doses happen is not data: the fire times, log(C0 / L) / k and then one every log((L + D) / L) / k,
follow from the parameters that are being estimated, so neither events= nor a steep input can express them.  The source says it
as a solve_ivp user would (include/smc_hip.h: STATE-TRIGGERED EVENTS): smc_user_root is the event function C - L, smc_user_root_dir
says "falling", smc_user_root_event adds the dose; the solve stops at the root, jumps and starts afresh
(user_models.root_chain is the same chain in SciPy).  Two subjects with different thresholds give pseudo-data; theta = (k, D, sigma)
- the rate AND the dose - is estimated; then the posterior predicts, with bands, a subject with a lower threshold on a finer grid.

    python examples/threshold_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
REDOSED = pkg.user_models.THRESHOLD_REDOSED      # g = y[0] - cond[1], falling; the event: y[0] += theta[1]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_384
rs = np.random.RandomState(0)
t = np.tile(np.linspace(0.0, 24.0, 49), (2, 1))
cond = np.array([[1.0, 0.4], [1.5, 0.6]])           # (C0, L) per subject
truth = np.array([0.25, 0.9, 0.03])
# the dose from 0.3 on: a solve may fire 256 times (SMC_USER_MAX_ROOT_FIRES), and a dose near 0 at a high rate would need more
priors = {"k": {"dist": "uniform", "low": 0, "high": 2}, "D": {"dist": "uniform", "low": 0.3, "high": 3},
          "sigma": {"dist": "uniform", "low": 0, "high": 0.5}}
grid = np.linspace(0.0, 36.0, 73)[None, :]
with pkg.HipEngine(n, 3, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(REDOSED, n_states=1, t=t, obs=np.zeros(t.shape + (1,)), cond=cond)
    clean = eng.predict_user(truth[None, :])[1][0]                       # pseudo-data: the model itself at the truth + noise
    obs = clean + truth[2] * rs.standard_normal(clean.shape)
    eng.set_model_user(REDOSED, n_states=1, t=t, obs=obs, cond=cond)
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=True,
                      predictive={"probs": (0.025, 0.5, 0.975), "t": grid, "cond": [[1.0, 0.25]]})
print("posterior mean", np.round(out["p_pred"].mean(axis=0), 4), "sd", np.round(out["p_pred"].std(axis=0), 4), "generated with", truth)
k, D = truth[:2]
print(f"at the truth subject 0 is re-dosed first at t = {np.log(1.0 / 0.4) / k:.3f}, then every {np.log((0.4 + D) / 0.4) / k:.3f}")
band = out["predictive"]
print("C(t) of a subject with C0 = 1 and the threshold 0.25 (never run): median and 95 % band")
for i in range(0, 73, 4):
    lo, med, hi = band["quantile"][:, 0, i, 0]
    print(f"  t = {grid[0, i]:6.2f}: C = {med:.4f}  [{lo:.4f}, {hi:.4f}]")
