"""CENSORED OBSERVATIONS: the one-compartment dosing model of examples/dosing_run.py, dC/dt = -k C with bolus doses, measured
by an assay with a lower limit of quantification.  The washout tails fall below the limit; the data set then says "below 0.12"
instead of a number.  Three ways to treat such values, and the posterior of the elimination rate k under each:

    dropped       the censored values are NaN: what is known about them (they ARE small) is thrown away
    substituted   the limit itself is passed as if it had been measured: the tails look higher than they were, k comes out low
    censored      each contributes the probability of lying at or below the limit, log Phi((L - f) / sd) (Beal's M3; include/smc_hip.h:
                  smc_set_model_user7; user_models.censored_loglik is the likelihood, censor_data makes the data)

    python examples/censored_run.py [n_particle]"""
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
LOQ = 0.12                                          # the assay's lower limit of quantification
t = np.tile(np.linspace(0.0, 24.0, 25), (2, 1))
C0 = np.array([[1.0], [0.0]])
doses = {"t": np.array([[12.0, nan], [0.5, 12.5]]), "values": np.array([[0.8, nan], [0.6, 0.6]])[:, :, None]}      # long washouts
truth = np.array([0.3, 0.03])
priors = {"k": {"dist": "uniform", "low": 0, "high": 2}, "sigma": {"dist": "uniform", "low": 0, "high": 0.5}}
with pkg.HipEngine(n, 2, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(DOSED, n_states=1, t=t, obs=np.zeros(t.shape + (1,)), cond=C0, events=doses)
    clean = eng.predict_user(truth[None, :])[1][0]                       # pseudo-data: the model itself at the truth + noise
    values = clean + truth[1] * rs.standard_normal(clean.shape)
    obs, censor = pkg.user_models.censor_data(values, lower=LOQ)         # the limit where a value falls below it, and the flag -1
    counts = pkg.user_models.censor_layout(t, obs, censor)
    print(f"lower limit {LOQ}: quantified per subject {counts['quantified'][:, 0]}, below the limit {counts['censored'][:, 0]}")
    ways = {"dropped": (np.where(censor != 0, nan, obs), None), "substituted": (obs, None), "censored": (obs, censor)}
    for name, (o, c) in ways.items():
        eng.set_model_user(DOSED, n_states=1, t=t, obs=o, cond=C0, events=doses, censor=c)
        out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=False)
        m, s = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
        print(f"{name:12s} k = {m[0]:.4f} +- {s[0]:.4f}   sigma = {m[1]:.4f} +- {s[1]:.4f}   (generated with k = {truth[0]}, sigma = {truth[1]})")
