"""PRIOR FAMILIES: the epidemic of examples/epidemic_run.py with informative priors (include/smc_hip.h: PRIOR FAMILIES; priors.py).

The overdispersion b of the negative-binomial counts is positive by definition and is read by the library itself, so it cannot
be moved to a log scale inside the source: it gets a gamma prior (mean 0.3, no mass at 0) instead of a box that touches 0.  The
transmission rate beta gets a log-normal around 1.2 per week, as a previous outbreak might suggest; the recovery rate keeps its
box.  A prior's DENSITY only acts under prior_mode="ratio_mask" (or "ratio"): under the default "mask" the same dict would only
keep the particles inside the supports.  Prints the posterior beside the one under the boxes of epidemic_run.py, and the prior's
own mean and sd of every parameter (scipy-free: from a NumPy-stream sample_prior).

    python examples/informative_prior_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
SIR = pkg.user_models.SIR_WEEKLY_CASES
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_384
rs = np.random.RandomState(0)
weeks = np.arange(0.0, 16.0)
t = np.tile(weeks, (2, 1))
cond = np.array([[20000.0, 10.0], [8000.0, 5.0]])               # (N, I0)
resets = {"t": np.tile(weeks[1:-1], (2, 1)), "values": None}
noise = {"additive": [("fixed", 1.0)], "proportional": [("param", 2)]}
truth = np.array([1.5, 0.8, 0.25])                              # beta, gamma per week; b
boxes = {"beta": {"dist": "uniform", "low": 0, "high": 5}, "gamma": {"dist": "uniform", "low": 0, "high": 5},
         "b": {"dist": "uniform", "low": 0, "high": 2}}
informative = {"beta": {"dist": "lognormal", "mu": float(np.log(1.2)), "sigma": 0.4}, "gamma": boxes["gamma"],
               "b": {"dist": "gamma", "shape": 3.0, "scale": 0.1}}
pkg.prior_layout(informative)                                   # the rules, before anything touches the device (ValueError with the reason)
np.random.seed(1)
draws = pkg.sample_prior(informative, 100_000)
print("the prior itself:", ", ".join(f"{nm} {draws[:, j].mean():.3f} +- {draws[:, j].std():.3f}" for j, nm in enumerate(informative)))
with pkg.HipEngine(n, 3, device=0) as eng:
    eng.set_prior(boxes)
    nothing = np.full(t.shape + (1,), np.nan)
    eng.set_model_user(SIR, n_states=3, t=t, obs=nothing, cond=cond, events=resets, noise=noise, rtol=1e-6, atol=1e-6)
    mean = eng.predict_user(truth[None, :])[1][0]
    lam = mean * rs.gamma(1.0 / truth[2] ** 2, truth[2] ** 2, size=mean.shape)
    cases = np.where(weeks[None, :, None] > 0, rs.poisson(lam).astype(np.float64), np.nan)
    eng.set_model_user(SIR, n_states=3, t=t, obs=cases, cond=cond, events=resets, noise=noise, rtol=1e-6, atol=1e-6)
    for label, priors, mode in (("boxes, mask", boxes, "mask"), ("informative, ratio_mask", informative, "ratio_mask")):
        eng.set_prior(priors)
        out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors, prior_mode=mode), rng="device", verbose=False)
        m, s = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
        assert np.all(pkg.prior_support(priors, out["p_pred"]))
        print(f"{label}: " + ", ".join(f"{nm} = {m[j]:.4f} +- {s[j]:.4f}" for j, nm in enumerate(priors))
              + f"   (generated with {truth}); logZ = {out.get('logZ', float('nan')):.3f}")
