"""COUNT OBSERVATIONS: an SIR epidemic fitted to weekly case counts (include/smc_hip.h: COUNT OBSERVATIONS; user_models.SIR_WEEKLY_CASES).

    dS/dt = -beta S I / N,   dI/dt = beta S I / N - gamma I,   dA/dt = beta S I / N

A accumulates the new infections; a scheduled event sets it back to 0 at every report time, and a data time equal to an event
time sees the state before the jump - so the model output at a report time is that week's incidence.  The source declares its
one output negative binomial (smc_user_obs_family[] = {2}): the output is the MEAN of the count, the variance is
mean + (b mean)^2 with the overdispersion b = theta[2] estimated beside beta and gamma (the output's proportional entry; its
additive entry is fixed at 1 and not used).  user_models.count_loglik is the likelihood.  Ends with two bands per week - of the
mean incidence (predictive_summary(noise=False)) and of replicated case counts (noise="family": a negative-binomial draw per
particle on the device, csrc/count_draw.h), with the share of the data inside each: the first is too narrow to hold them, the
second should hold 90 % - and with the PIT histogram of the counts (pointwise_summary(count_pit=True), user_models.pit_histogram),
which is flat when the model is calibrated.

    python examples/epidemic_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
SIR = pkg.user_models.SIR_WEEKLY_CASES
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_384
rs = np.random.RandomState(0)
weeks = np.arange(0.0, 16.0)                                    # t[e][0] = 0 is the initial time, reports at weeks 1 .. 15
t = np.tile(weeks, (2, 1))                                      # two towns
cond = np.array([[20000.0, 10.0], [8000.0, 5.0]])               # (N, I0)
resets = {"t": np.tile(weeks[1:-1], (2, 1)), "values": None}    # A = 0 after every report but the last (the row's end)
noise = {"additive": [("fixed", 1.0)], "proportional": [("param", 2)]}
truth = np.array([1.5, 0.8, 0.25])                              # beta, gamma per week; b
priors = {"beta": {"dist": "uniform", "low": 0, "high": 5}, "gamma": {"dist": "uniform", "low": 0, "high": 5},
          "b": {"dist": "uniform", "low": 0, "high": 2}}
with pkg.HipEngine(n, 3, device=0) as eng:
    eng.set_prior(priors)
    nothing = np.full(t.shape + (1,), np.nan)
    eng.set_model_user(SIR, n_states=3, t=t, obs=nothing, cond=cond, events=resets, noise=noise, rtol=1e-6, atol=1e-6)
    mean = eng.predict_user(truth[None, :])[1][0]               # pseudo-data: the model's weekly incidence at the truth ...
    lam = mean * rs.gamma(1.0 / truth[2] ** 2, truth[2] ** 2, size=mean.shape)
    cases = np.where(weeks[None, :, None] > 0, rs.poisson(lam).astype(np.float64), np.nan)      # ... as gamma-mixed Poisson counts
    print("weekly cases, town 0:", cases[0, 1:, 0].astype(int))
    print("weekly cases, town 1:", cases[1, 1:, 0].astype(int))
    eng.set_model_user(SIR, n_states=3, t=t, obs=cases, cond=cond, events=resets, noise=noise, rtol=1e-6, atol=1e-6)
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=False)
    m, s = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
    for j, nm in enumerate(priors):
        print(f"{nm:6s} = {m[j]:.4f} +- {s[j]:.4f}   (generated with {truth[j]})")
    print(f"R0 = beta / gamma = {np.mean(out['p_pred'][:, 0] / out['p_pred'][:, 1]):.3f} (generated with {truth[0] / truth[1]:.3f}); logZ = {out.get('logZ', float('nan')):.3f}")
    band = eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.05, 0.5, 0.95))          # bands of the MEAN weekly incidence
    repl = eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.05, 0.5, 0.95), noise="family", seed=1)      # ... of replicated case counts
    for e in range(2):
        print(f"town {e}: week, cases, 5 % / median / 95 % of the mean, 5 % / median / 95 % of replicated counts")
        for i in range(1, weeks.size):
            q, r = band["quantile"][:, e, i, 0], repl["quantile"][:, e, i, 0]
            print(f"   {int(weeks[i]):2d}  {int(cases[e, i, 0]):5d}   {q[0]:8.1f} {q[1]:8.1f} {q[2]:8.1f}   {r[0]:8.1f} {r[1]:8.1f} {r[2]:8.1f}")
    seen = np.isfinite(cases)
    for name, b in (("mean", band), ("replicated counts", repl)):
        inside = (cases >= b["lower"][0]) & (cases <= b["upper"][2]) & seen
        print(f"share of the {int(seen.sum())} observed counts inside the 5 % - 95 % band of the {name}: {inside.sum() / seen.sum():.2f}")
    pw = eng.pointwise_summary(pkg.SMC_SET_PRED, count_pit=True, seed=1)
    hist = pkg.user_models.pit_histogram(pw["pit_lower"][seen], pw["pit_upper"][seen], bins=5)
    print("PIT histogram of the counts (5 bins, flat = 0.2 each):", np.round(hist, 3), f"; elpd_waic {pw['waic']['elpd_waic']:.1f}")
