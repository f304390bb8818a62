"""A NOISE MODEL of your own: A -> B -> C with both A and B measured by two instruments.  Each output has its own noise level,
estimated from the data, and the noise of A grows with the signal: sd^2 = a_k^2 + (b_k f)^2 with b_B = 0 (include/smc_hip.h:
smc_set_model_user4).  theta = (k1, k2, a_A, a_B, b_A) is estimated; the band of replicated observations then widens where A
is large.  user_models.noise_loglik is the likelihood in NumPy, applied here to the engine's own predictions as a check.

    python examples/noise_model_run.py [n_particle]"""
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
k1, k2, a, b = 0.8, 0.3, np.array([0.01, 0.02]), np.array([0.08, 0.0])
tt = np.nan_to_num(t)
A = A0[:, None] * np.exp(-k1 * tt)
B = A0[:, None] * k1 / (k2 - k1) * (np.exp(-k1 * tt) - np.exp(-k2 * tt))
f = np.stack([A, B], axis=2)
obs = f + np.sqrt(a ** 2 + (b * f) ** 2) * rs.standard_normal(f.shape)
obs[rs.uniform(size=obs.shape) < 0.15] = np.nan          # missing values
priors = {"k1": {"dist": "uniform", "low": 0, "high": 3}, "k2": {"dist": "uniform", "low": 0, "high": 3},
          "a_A": {"dist": "uniform", "low": 0, "high": 0.2}, "a_B": {"dist": "uniform", "low": 0, "high": 0.2},
          "b_A": {"dist": "uniform", "low": 0, "high": 0.5}}
# one entry per output: a parameter of the particle, or a fixed number
noise = {"additive": [("param", 2), ("param", 3)], "proportional": [("param", 4), ("fixed", 0.0)]}
print("noise layout:", pkg.user_models.noise_layout(noise, n_obs=2, dim=5))
with pkg.HipEngine(n, 5, device=0) as eng:
    eng.set_prior(priors)
    eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, n_states=2, t=t, obs=obs, cond=A0[:, None], rtol=1e-6, atol=1e-9,
                       noise=noise)
    out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=priors), rng="device", verbose=True,
                      predictive={"probs": (0.025, 0.5, 0.975), "noise": True, "seed": 1})
    lk, pred, _ = eng.predict_user(out["p_pred"][:256])
print("posterior mean", np.round(out["p_pred"].mean(axis=0), 4), "sd", np.round(out["p_pred"].std(axis=0), 4))
print("generated with", (k1, k2, *a, b[0]))
ref = pkg.user_models.noise_loglik(pred, t, obs, out["p_pred"][:256], noise)
print(f"logL of 256 posterior particles against noise_loglik of their predictions: {np.max(np.abs(lk - ref) / np.abs(ref)):.2e} relative")
band = out["predictive"]
print("95 % band of a replicated observation of A in experiment 1 (A0 = 2): it narrows as A falls")
for i in (0, 5, 15, 29):
    lo, med, hi = band["quantile"][:, 1, i, 0]
    print(f"  t = {t[1, i]:6.3f}: A = {A[1, i]:.4f}, median {med:.4f}, band [{lo:.4f}, {hi:.4f}], width {hi - lo:.4f} "
          f"(closed form {2 * 1.96 * np.sqrt(a[0] ** 2 + (b[0] * A[1, i]) ** 2):.4f})")
