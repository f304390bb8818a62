"""SCHEDULED EVENTS: a one-compartment model under repeated bolus doses, dC/dt = -k C with C += dose / V at the dosing times.
The doses are not part of the right-hand side: at each dosing time the integrator stops, the model's smc_user_event changes the
state by a jump, and the solve starts afresh from there - the chain of solve_ivp calls a SciPy user would write (include/smc_hip.h:
smc_set_model_user6; user_models.event_layout states the data rules).  Two subjects dosed on different schedules give
pseudo-data; theta = (k, sigma) is estimated; then the posterior predicts, with bands, the concentration under a regimen that
was never run: a loading dose followed by smaller maintenance doses every 6 h ("what if we dose like this instead").  The design's
events go to the compiled model as data: nothing is compiled again.

    python examples/dosing_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
DOSED = pkg.user_models.ONE_COMPARTMENT_DOSED      # smc_user_event: y[0] += smc_event_value(cond, j, 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_384
rs = np.random.RandomState(0)
nan = np.nan
t = np.tile(np.linspace(0.0, 24.0, 25), (2, 1))
C0 = np.array([[1.0], [0.0]])                       # subject 1 starts empty: its first dose is an event, at t = 0.5
# dosing schedules: a row is (times, amounts), NaN-padded to the longest; room for 4 events per row is compiled in
doses = {"t": np.array([[8.0, 16.0, nan, nan],                      # 1.0 at t = 0 (the initial state), then every 8 h
                        [0.5, 6.5, 12.5, 18.5]]),                   # every 6 h
         "values": np.array([[0.8, 0.8, nan, nan],
                             [0.6, 0.6, 0.6, 0.6]])[:, :, None]}
print("events per subject:", pkg.user_models.event_layout(t, doses["t"], doses["values"]))
truth = np.array([0.15, 0.03])
priors = {"k": {"dist": "uniform", "low": 0, "high": 2}, "sigma": {"dist": "uniform", "low": 0, "high": 0.5}}
# the regimen for the prediction: from empty, a loading dose of 1.5 at t = 1, then 0.5 every 6 h, on a finer grid over 36 h
grid = np.linspace(0.0, 36.0, 73)[None, :]
what_if = {"t": np.array([[1.0, 7.0, 13.0, 19.0]]), "values": np.array([[1.5, 0.5, 0.5, 0.5]])[:, :, None]}
with pkg.HipEngine(n, 2, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(DOSED, n_states=1, t=t, obs=np.zeros(t.shape + (1,)), cond=C0, events=doses)
    clean = eng.predict_user(truth[None, :])[1][0]                       # pseudo-data: the model itself at the truth + noise
    obs = clean + truth[1] * rs.standard_normal(clean.shape)
    eng.set_model_user(DOSED, n_states=1, t=t, obs=obs, cond=C0, events=doses)
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=True,
                      predictive={"probs": (0.025, 0.5, 0.975), "t": grid, "cond": [[0.0]], "events": what_if})
print("posterior mean", np.round(out["p_pred"].mean(axis=0), 4), "sd", np.round(out["p_pred"].std(axis=0), 4), "generated with", truth)
band = out["predictive"]
print("C(t) under a loading dose of 1.5 at t = 1 and 0.5 every 6 h from t = 7 (a regimen that was never run): median and 95 % band")
for i in range(0, 73, 4):
    lo, med, hi = band["quantile"][:, 0, i, 0]
    given = float(np.sum(what_if["values"][0, :, 0][what_if["t"][0] < grid[0, i]]))
    print(f"  t = {grid[0, i]:6.2f}: dosed so far {given:.1f}, C = {med:.4f}  [{lo:.4f}, {hi:.4f}]")
