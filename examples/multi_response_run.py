"""SEVERAL MEASURED SPECIES with gaps: A -> B -> C, A and B measured in four experiments (A with noise sigma, B with 3 sigma:
obs_scale), some values missing (NaN) and one experiment stopped early (its times end in NaN).  k1, k2 and sigma are
estimated; then the whole resident posterior predicts the product C, which was never measured, with its 95 % band - on a
200-point grid and for an initial concentration that was not among the experiments.  The band is formed on the device
(HipEngine.predictive_summary through run_smc(predictive=...)): only the summaries cross the bus.

    python examples/multi_response_run.py [n_particle]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 32_768
rs = np.random.RandomState(0)
t = np.tile(np.linspace(0.0, 10.0, 30), (4, 1))
t[2, 18:] = np.nan                                       # experiment 2 ended after 18 samples
A0 = np.array([1.0, 2.0, 0.5, 1.5])
k1, k2, sigma, scale = 0.8, 0.3, 0.01, np.array([1.0, 3.0])
tt = np.nan_to_num(t)
A = A0[:, None] * np.exp(-k1 * tt)
B = A0[:, None] * k1 / (k2 - k1) * (np.exp(-k1 * tt) - np.exp(-k2 * tt))
obs = np.stack([A, B], axis=2) + sigma * scale * rs.standard_normal(t.shape + (2,))
obs[rs.uniform(size=obs.shape) < 0.15] = np.nan          # missing values
print("layout:", pkg.user_models.obs_layout(t, obs, scale))
priors = {"k1": {"dist": "uniform", "low": 0, "high": 3}, "k2": {"dist": "uniform", "low": 0, "high": 3},
          "sigma": {"dist": "uniform", "low": 0, "high": 1}}
# C = A0 - A - B as a third output with no data: an all-NaN column adds nothing to the likelihood
obs3 = np.concatenate([obs, np.full(t.shape + (1,), np.nan)], axis=2)
grid = np.linspace(0.0, 15.0, 200)[None, :]              # finer and longer than the data's 30 times to t = 10
A0_new = 2.75                                            # an experiment that was never run
with pkg.HipEngine(n, 3, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_ABC, n_states=2, t=t, obs=obs3, cond=A0[:, None],
                       obs_scale=(1.0, 3.0, 1.0))
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=True,
                      predictive={"t": grid, "cond": [[A0_new]], "probs": (0.025, 0.5, 0.975)})
    # the same band for replicated observations (model + measurement noise sigma), and at the data's own times
    noisy = eng.predictive_summary(pkg.SMC_SET_PRED, t=grid, cond=[[A0_new]], noise=True, seed=1)
    at_data = eng.predictive_summary(pkg.SMC_SET_PRED)
print("posterior mean", out["p_pred"].mean(axis=0), "sd", out["p_pred"].std(axis=0), "(generated with", (k1, k2, sigma), ")")
band = out["predictive"]
tg = grid[0]
C_true = A0_new * (1 - (k2 * np.exp(-k1 * tg) - k1 * np.exp(-k2 * tg)) / (k2 - k1))
print(f"C for A0 = {A0_new} from all {n} particles ({band['kernel_ms']['predict']:.2f} ms predicting, "
      f"{band['kernel_ms']['summary']:.2f} ms summarising on the device):")
for i in (20, 66, 133, 199):
    lo, med, hi = band["quantile"][:, 0, i, 2]
    print(f"  t = {tg[i]:6.3f}: median {med:.4f}, 95 % band [{lo:.4f}, {hi:.4f}] (of an observation [{noisy['quantile'][0, 0, i, 2]:.4f}, "
          f"{noisy['quantile'][2, 0, i, 2]:.4f}]), closed form {C_true[i]:.4f}")
last = [29, 29, 17, 29]                                  # each experiment's last finite time
print("median C at the last time of each experiment:", np.round(at_data["quantile"][1, np.arange(4), last, 2], 4),
      "closed form:", np.round((A0[:, None] - A - B)[np.arange(4), last], 4))
