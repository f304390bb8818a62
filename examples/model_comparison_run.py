"""MODEL COMPARISON AND CALIBRATION: two candidate models for one data set, compared by predictive accuracy and checked for
calibration - what one does straight after a fit.  Pseudo-data of A -> B -> C (both A and B measured) whose noise has a
proportional part; candidate 1 fits it with one sigma for both outputs (the sigma rule), candidate 2 with a level per output and
a proportional part on A (a noise model).  run_smc(pointwise=True) forms, on the device, the statistics of every observation's
log-likelihood term over the posterior (include/smc_hip.h: smc_user_pointwise_summary); from them

    logZ        the evidence of the run
    elpd_waic   the expected log predictive density (WAIC), its standard error and p_waic, the effective number of parameters
    PIT         the probability integral transform of every measured value under the posterior predictive: uniform on (0, 1) for a
                calibrated model; a hump in the middle says the predictive is too wide, horns at the ends that it is too narrow

HipEngine.pointwise_loglik(particles) returns the whole (draws x observations) matrix for ArviZ / loo (PSIS-LOO).

    python examples/model_comparison_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
AB = pkg.user_models.CONSECUTIVE_REACTIONS_AB
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_384
rs = np.random.RandomState(0)
t = np.tile(np.linspace(0.0, 10.0, 30), (4, 1))
A0 = np.array([[0.5], [1.0], [1.5], [2.0]])
truth = np.array([0.8, 0.3, 0.01, 0.02, 0.08])         # k1, k2, a_A, a_B, b_A
wide = {"dist": "uniform", "low": 0, "high": 3}
level = {"dist": "uniform", "low": 0, "high": 0.5}
candidates = {
    "one sigma": ({"k1": wide, "k2": wide, "sigma": level}, {}),
    "noise model": ({"k1": wide, "k2": wide, "a_A": level, "a_B": level, "b_A": level},
                    {"noise": {"additive": [("param", 2), ("param", 3)], "proportional": [("param", 4), ("fixed", 0.0)]}}),
}
obs = None
for name, (priors, kw) in candidates.items():
    with pkg.HipEngine(n, len(priors), device=0) as eng:
        eng.set_prior(priors)
        if obs is None:                                # pseudo-data: the model itself at the truth + its noise
            eng.set_model_user(AB, n_states=2, t=t, obs=np.zeros(t.shape + (2,)), cond=A0)
            clean = eng.predict_user(truth[None, :3])[1][0]
            sd = np.sqrt(truth[2:4] ** 2 + (np.array([truth[4], 0.0]) * clean) ** 2)
            obs = clean + sd * rs.standard_normal(clean.shape)
        eng.set_model_user(AB, n_states=2, t=t, obs=obs, cond=A0, **kw)
        out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=False, pointwise=True)
    pw = out["pointwise"]
    w = pw["waic"]
    pit = pw["pit"][np.isfinite(pw["pit"])]
    print(f"{name:12s} logZ = {out['logZ']:.2f}   elpd_waic = {w['elpd_waic']:.2f} +- {w['se']:.2f}   p_waic = {w['p_waic']:.2f}   "
          f"({w['n_cells']} observations; pointwise kernels {pw['kernel_ms']['pointwise']:.2f} ms after a prediction sweep of "
          f"{pw['kernel_ms']['predict']:.2f} ms)")
    print(f"{'':12s} PIT histogram, ten bins: {np.histogram(pit, 10, (0.0, 1.0))[0]}")
