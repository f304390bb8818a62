"""Data and reference posterior of tests/test_user_noise_model.py: A -> B -> C with A and B measured under the noise model
sd^2 = a_k^2 + (b_k f)^2 (include/smc_hip.h: smc_set_model_user4).

    python tests/noise_model_chain.py [data_seed] [samples]

runs a random-walk Metropolis chain in NumPy on the closed-form solution under the uniform priors of the full-run test and
prints the posterior mean and standard deviation of theta = (k1, k2, a0, a1, b0): the constants CHAIN_MEAN / CHAIN_SD of
the test (data seed 0) come from here.  The chain knows nothing of the engine: closed form instead of an integrator, the
plain density instead of the excess formulation."""
import sys

import numpy as np

A0 = np.array([1.0, 2.0, 0.5, 1.5])
K_TRUE = (0.8, 0.3)
A_TRUE = (0.01, 0.02)
B_TRUE = (0.08, 0.0)
THETA_TRUE = np.array([K_TRUE[0], K_TRUE[1], A_TRUE[0], A_TRUE[1], B_TRUE[0]])
PRIOR_HIGH = np.array([3.0, 3.0, 0.2, 0.2, 0.5])      # uniform on (0, high)
NOISE = {"additive": [("param", 2), ("param", 3)], "proportional": [("param", 4), ("fixed", 0.0)]}


def closed_form(k1, k2, t):
    """Outputs (A, B) at t (n_ex, n_t) (NaN times give NaN): (n_ex, n_t, 2)."""
    a = A0[:, None] * np.exp(-k1 * t)
    b = A0[:, None] * k1 / (k2 - k1) * (np.exp(-k1 * t) - np.exp(-k2 * t))
    return np.stack([a, b], axis=2)


def make_data(seed=0):
    """4 experiments x 30 times, row 2 cut after 18 times, 15 % of the observations NaN; noise drawn with sd_ik from the closed form."""
    rs = np.random.RandomState(seed)
    n_ex, n_t = 4, 30
    t = np.tile(np.linspace(0.0, 10.0, n_t), (n_ex, 1))
    t[2, 18:] = np.nan
    f = closed_form(K_TRUE[0], K_TRUE[1], np.nan_to_num(t))
    sd = np.sqrt(np.array(A_TRUE) ** 2 + (np.array(B_TRUE) * f) ** 2)
    obs = f + sd * rs.standard_normal(f.shape)
    obs[rs.uniform(size=obs.shape) < 0.15] = np.nan
    return t, obs


def log_post(theta, t, obs):
    if np.any(theta <= 0) or np.any(theta >= PRIOR_HIGH) or theta[0] == theta[1]:
        return -np.inf
    f = closed_form(theta[0], theta[1], t)
    sd2 = theta[2:4] ** 2 + (np.array([theta[4], 0.0]) * f) ** 2
    return np.nansum(-0.5 * np.log(2 * np.pi * sd2) - (obs - f) ** 2 / (2 * sd2))       # NaN: not measured / past the row's end


def chain(t, obs, n, cov, start, rs):
    L = np.linalg.cholesky(cov)
    x, lp = start.copy(), log_post(start, t, obs)
    out = np.empty((n, x.size))
    acc = 0
    for i in range(n):
        y = x + L @ rs.standard_normal(x.size)
        ly = log_post(y, t, obs)
        if np.log(rs.uniform()) < ly - lp:
            x, lp = y, ly
            acc += 1
        out[i] = x
    return out, acc / n


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
    t, obs = make_data(seed)
    rs = np.random.RandomState(1000 + seed)
    pilot, _ = chain(t, obs, 30000, np.diag((np.array([0.0064, 0.0017, 0.0011, 0.0015, 0.0128]) * 0.8) ** 2), THETA_TRUE, rs)
    cov = np.cov(pilot[10000:].T) * 2.4 ** 2 / 5
    xs, rate = chain(t, obs, n + 10000, cov, pilot[-1], rs)
    xs = xs[10000:]
    np.set_printoptions(precision=5, suppress=True)
    print(f"data seed {seed}, {n} samples, acceptance {rate:.3f}")
    print("mean", repr(xs.mean(axis=0)))
    print("sd  ", repr(xs.std(axis=0)))
    half = n // 2
    print("half-chain means differ by (in sd)", np.abs(xs[:half].mean(axis=0) - xs[half:].mean(axis=0)) / xs.std(axis=0))
    print("truth off by (in sd)", (xs.mean(axis=0) - THETA_TRUE) / xs.std(axis=0))


if __name__ == "__main__":
    main()
