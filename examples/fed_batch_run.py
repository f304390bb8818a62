"""A TIME-VARYING MEASURED INPUT: Michaelis-Menten consumption of a substrate that is fed while it reacts,
dS/dt = -Vmax S / (Km + S) + F(t).  The feed rate F is not a constant of the experiment but a logged profile: knots (time,
rate), linear in between, which the model reads as smc_input(cond, 0, t) (include/smc_hip.h: smc_set_model_user5;
user_models.input_value is the definition).  Two experiments with different feed profiles - a ramp that is switched off, and
two pulses - give pseudo-data; theta = (Vmax, Km, sigma) is estimated; then the posterior predicts, with bands, what a THIRD
profile nobody ran would give ("what if I feed like this instead").  The integrators do not stop at knots: a switch is a steep
ramp between two close knots, stepped over under the solver's own step control, as solve_ivp does with np.interp inside f.

    python examples/fed_batch_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

FED_BATCH = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = smc_div((-theta[0]) * y[0], theta[1] + y[0]) + smc_input(cond, 0, t);
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[0]; }
"""

pkg = g.load_package()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_384
rs = np.random.RandomState(0)
nan = np.nan
t = np.tile(np.linspace(0.0, 12.0, 25), (2, 1))
S0 = np.array([[2.0], [0.5]])
# feed profiles: a row is (knot times, rates), NaN-padded to the longest; a switch is two knots 1e-3 apart
feed = {"t": np.array([[0.0, 4.0, 4.001, nan, nan, nan, nan, nan],                  # ramp up to 0.6, then off
                       [0.0, 1.999, 2.0, 3.0, 3.001, 7.0, 8.0, 9.0]]),              # a pulse, then a triangle
        "u": np.array([[0.0, 0.6, 0.0, nan, nan, nan, nan, nan],
                       [0.0, 0.0, 0.8, 0.8, 0.0, 0.0, 0.5, 0.0]])}
print("knots per experiment:", pkg.user_models.input_layout(feed["t"], feed["u"], 2))
truth = np.array([1.2, 0.5, 0.03])
priors = {"Vmax": {"dist": "uniform", "low": 0, "high": 5}, "Km": {"dist": "uniform", "low": 0, "high": 5},
          "sigma": {"dist": "uniform", "low": 0, "high": 0.5}}
# a third profile for the prediction: a constant feed from t = 1 on, on a finer time grid, from S0 = 1
grid = np.linspace(0.0, 12.0, 49)[None, :]
what_if = {"t": np.array([[1.0, 1.001]]), "u": np.array([[0.0, 0.4]])}
with pkg.HipEngine(n, 3, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(FED_BATCH, n_states=1, t=t, obs=np.zeros(t.shape + (1,)), cond=S0, inputs=feed)
    clean = eng.predict_user(truth[None, :])[1][0]                       # pseudo-data: the model itself at the truth + noise
    obs = clean + truth[2] * rs.standard_normal(clean.shape)
    eng.set_model_user(FED_BATCH, n_states=1, t=t, obs=obs, cond=S0, inputs=feed)
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=True,
                      predictive={"probs": (0.025, 0.5, 0.975), "t": grid, "cond": [[1.0]], "inputs": what_if})
print("posterior mean", np.round(out["p_pred"].mean(axis=0), 4), "sd", np.round(out["p_pred"].std(axis=0), 4), "generated with", truth)
band = out["predictive"]
print("S(t) under a constant feed of 0.4 from t = 1 on, S0 = 1 (an experiment that was never run): median and 95 % band")
for i in range(0, 49, 6):
    lo, med, hi = band["quantile"][:, 0, i, 0]
    print(f"  t = {grid[0, i]:6.2f}: feed {float(pkg.user_models.input_value(what_if['t'][0], what_if['u'][0], grid[0, i])):.2f}, "
          f"S = {med:.4f}  [{lo:.4f}, {hi:.4f}]")
