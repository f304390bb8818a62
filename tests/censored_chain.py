"""Data, populations and the reference posterior of tests/test_user_censored.py: the data of tests/noise_model_chain.py
(A -> B -> C, A and B measured, sd^2 = a_k^2 + (b_k f)^2) with limits of quantification (include/smc_hip.h:
smc_set_model_user7; user_models.censor_data, censored_loglik).

    python tests/censored_chain.py [data_seed] [samples] [lower limit of B]

runs random-walk Metropolis chains in NumPy on the closed-form solution under the uniform priors of the full-run test, once with
the values of B below the limit CENSORED (log Phi terms) and once with them DROPPED (NaN), and prints the posterior mean and
standard deviation of theta = (k1, k2, a0, a1, b0) of both: the constants CHAIN_MEAN / CHAIN_SD / DROPPED_K2 of the test (data
seed 0) come from here.  The chain knows nothing of the engine: closed form instead of an integrator, scipy's log_ndtr instead
of the excess formulation."""
import sys

import numpy as np

import noise_model_chain as NC

# the full run: a lower limit on B that censors about a third of its values (washout tails and the first, still empty, times)
FULL_RUN_LIMIT_B = 0.25


def two_sided(seed=0, frac=0.3):
    """The noise tests' data censored on both sides: per output a lower limit at its `frac` quantile and an upper limit at its
    1 - frac quantile, so that 20 - 40 % of the values are censored on each side.  Returns t, the values (NaN past a row's end) and
    the limits, (n_obs,) each: user_models.censor_data(values, lower, upper) makes obs and the flags."""
    t, values = NC.make_data(seed)
    values = np.where(np.isnan(t)[:, :, None], np.nan, values)
    lower = np.nanquantile(values, frac, axis=(0, 1))
    upper = np.nanquantile(values, 1.0 - frac, axis=(0, 1))
    return t, values, lower, upper


def plant(obs, censor):
    """The records a layout can get wrong, planted on censored data (4 x 30 x 2, row 2 ends after 18 times): a record with one
    output censored and the other NaN, one quantified next to a censored one, both flag signs in one record, an experiment whose
    every value is censored (m_e = 0), an output censored everywhere, and flags up to a ragged row's last time."""
    obs, censor = obs.copy(), np.array(censor, dtype=np.int8)
    obs[0, 3] = (0.9, np.nan); censor[0, 3] = (-1, 0)          # censored | not measured
    obs[0, 4] = (0.8, 0.1); censor[0, 4] = (0, 1)              # quantified | censored
    obs[0, 5] = (0.7, 0.2); censor[0, 5] = (1, -1)             # both signs in one record
    obs[0, 6] = (np.nan, np.nan); censor[0, 6] = (0, 0)        # nothing measured
    seen = ~np.isnan(obs[3])
    obs[3] = np.where(seen, 0.3, np.nan)                       # experiment 3: every value censored, from the left
    censor[3] = np.where(seen, -1, 0)
    obs[2, :18, 1] = 0.45                                      # experiment 2 (ragged): output B censored everywhere, from the right
    censor[2, :18, 1] = 1
    censor[2, 18:] = 0
    return obs, censor


def log_post(theta, t, obs, censor):
    from scipy.special import log_ndtr
    if np.any(theta <= 0) or np.any(theta >= NC.PRIOR_HIGH) or theta[0] == theta[1]:
        return -np.inf
    f = NC.closed_form(theta[0], theta[1], t)
    sd = np.sqrt(theta[2:4] ** 2 + (np.array([theta[4], 0.0]) * f) ** 2)
    dens = -0.5 * np.log(2 * np.pi * sd * sd) - (obs - f) ** 2 / (2 * sd * sd)
    z = np.where(censor < 0, obs - f, f - obs) / sd
    return np.nansum(np.where(censor == 0, dens, log_ndtr(z)))      # NaN: not measured / past the row's end


def chain(t, obs, censor, n, cov, start, rs):
    L = np.linalg.cholesky(cov)
    x, lp = start.copy(), log_post(start, t, obs, censor)
    out = np.empty((n, x.size))
    acc = 0
    for i in range(n):
        y = x + L @ rs.standard_normal(x.size)
        ly = log_post(y, t, obs, censor)
        if np.log(rs.uniform()) < ly - lp:
            x, lp = y, ly
            acc += 1
        out[i] = x
    return out, acc / n


def full_run_data(seed=0, limit=FULL_RUN_LIMIT_B):
    """t, obs, censor of the full run, and obs with the censored values dropped (NaN)."""
    t, values = NC.make_data(seed)
    values = np.where(np.isnan(t)[:, :, None], np.nan, values)
    lower = np.array([np.nan, limit])
    with np.errstate(invalid="ignore"):
        below = values < lower
    obs = np.where(below, lower, values)
    censor = -below.astype(np.int8)
    return t, obs, censor, np.where(below, np.nan, values)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
    limit = float(sys.argv[3]) if len(sys.argv) > 3 else FULL_RUN_LIMIT_B
    t, obs, censor, dropped = full_run_data(seed, limit)
    nb = np.sum(~np.isnan(NC.make_data(seed)[1][:, :, 1]))
    print(f"data seed {seed}, limit {limit}: {np.sum(censor != 0)} of {nb} values of B censored")
    np.set_printoptions(precision=5, suppress=True)
    for name, o, c in (("censored", obs, censor), ("dropped", dropped, np.zeros_like(censor))):
        rs = np.random.RandomState(1000 + seed)
        pilot, _ = chain(t, o, c, 30000, np.diag((np.array([0.0064, 0.0017, 0.0011, 0.0015, 0.0128]) * 0.8) ** 2), NC.THETA_TRUE, rs)
        cov = np.cov(pilot[10000:].T) * 2.4 ** 2 / 5
        xs, rate = chain(t, o, c, n + 10000, cov, pilot[-1], rs)
        xs = xs[10000:]
        print(f"{name}: {n} samples, acceptance {rate:.3f}")
        print("mean", repr(xs.mean(axis=0)))
        print("sd  ", repr(xs.std(axis=0)))
        half = n // 2
        print("half-chain means differ by (in sd)", np.abs(xs[:half].mean(axis=0) - xs[half:].mean(axis=0)) / xs.std(axis=0))


if __name__ == "__main__":
    main()
