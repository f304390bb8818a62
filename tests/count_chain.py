"""Models, data and reference posterior of tests/test_user_counts.py: count observations of a user model (include/smc_hip.h:
COUNT OBSERVATIONS).  A -> B -> C of tests/noise_model_chain.py with A measured (Gaussian) and the number of B molecules in a
volume V counted: the output V * B is the mean of a negative-binomial or Poisson count.

    python tests/count_chain.py [data_seed] [samples]

runs two random-walk Metropolis chains in NumPy on the closed-form solution, one under user_models.count_loglik with the counts
negative binomial, one with the same counts declared Gaussian with an estimated sigma, and prints posterior means and standard
deviations: the constants CHAIN_MEAN / CHAIN_SD / GAUSS_K2 of the test come from here.  The chains know nothing of the engine."""
import os
import sys

import numpy as np

import noise_model_chain as NC

V = 300.0                                  # cond[1]: counts up to about 270
COND = np.column_stack([NC.A0, np.full(4, V)])
K_TRUE, A_TRUE, B_TRUE = NC.K_TRUE, 0.01, 0.5
THETA_TRUE = np.array([K_TRUE[0], K_TRUE[1], A_TRUE, B_TRUE])
NAMES = ("k1", "k2", "a0", "b")
PRIOR_HIGH = np.array([3.0, 3.0, 0.2, 1.0])             # uniform on (0, high); b: the coefficient of variation of the extra scatter
GAUSS_PRIOR_HIGH = np.array([3.0, 3.0, 0.2, 500.0])     # ... and the sigma of the counts declared Gaussian
NOISE_NB = {"additive": [("param", 2), ("fixed", 1.0)], "proportional": [("fixed", 0.0), ("param", 3)]}
NOISE_POISSON = {"additive": [("param", 2), ("fixed", 1.0)]}
NOISE_GAUSS = {"additive": [("param", 2), ("param", 3)]}
# three outputs, an odd n_obs and a count in slot 0: (V B negative binomial, V C Poisson, A Gaussian), theta = (k1, k2, a, b)
NOISE_3 = {"additive": [("fixed", 1.0), ("fixed", 1.0), ("param", 2)], "proportional": [("param", 3), ("fixed", 0.0), ("fixed", 0.0)]}

_HEAD = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = -theta[0] * y[0];
    dydt[1] = theta[0] * y[0] - theta[1] * y[1];
}
"""
_OUT2 = r"""
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) {
    out[0] = y[0];
    out[1] = cond[1] * y[1];
}
"""
_OUT3 = r"""
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) {
    out[0] = cond[1] * y[1];
    out[1] = cond[1] * (cond[0] - y[0] - y[1]);
    out[2] = y[0];
}
"""


def family_line(family):
    return "// the families: a use of the name smc_user_obs_family in a comment is passed over\n" \
           "__device__ const int smc_user_obs_family[] = {" + ", ".join(str(f) for f in family) + "};\n"


def source(family=None):
    """The A -> B -> C source with outputs (A, V B), or (V B, V C, A) for three families; None: without the name."""
    outs = _OUT3 if family is not None and len(family) == 3 else _OUT2
    return ("" if family is None else family_line(family)) + _HEAD + outs


# dy/dt = 0, out = theta[0]: the mean is the parameter itself, for planted values (one experiment of 64 times)
def constant_source(family):
    return family_line([family]) + r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) { dydt[0] = 0.0; }
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) { out[0] = theta[0]; }
"""


def closed_form(k1, k2, t, three=False):
    """Outputs at t (n_ex, n_t): (A, V B), or (V B, V C, A)."""
    ab = NC.closed_form(k1, k2, t)
    a, b = ab[:, :, 0], ab[:, :, 1]
    if three:
        return np.stack([V * b, V * (NC.A0[:, None] - a - b), a], axis=2)
    return np.stack([a, V * b], axis=2)


def negbin_draw(rs, mu, b):
    """Counts with mean mu and variance mu + (b mu)^2: a gamma-mixed Poisson (b = 0: Poisson)."""
    mu = np.asarray(mu, dtype=np.float64)
    lam = mu if b == 0 else mu * rs.gamma(1.0 / b ** 2, b ** 2, size=mu.shape)
    return rs.poisson(lam).astype(np.float64)


def make_data(seed=0, b=B_TRUE, three=False):
    """4 experiments x 30 times, row 2 cut after 18 times, 15 % of the values NaN (NC.make_data's layout).  Two outputs: A with sd
    A_TRUE, V B negative binomial with overdispersion b (0: Poisson); three: V B so, V C Poisson, A Gaussian."""
    rs = np.random.RandomState(seed)
    n_ex, n_t = 4, 30
    t = np.tile(np.linspace(0.0, 10.0, n_t), (n_ex, 1))
    t[2, 18:] = np.nan
    f = closed_form(K_TRUE[0], K_TRUE[1], np.nan_to_num(t), three)
    obs = np.empty_like(f)
    if three:
        obs[:, :, 0] = negbin_draw(rs, f[:, :, 0], b)
        obs[:, :, 1] = negbin_draw(rs, f[:, :, 1], 0.0)
        obs[:, :, 2] = f[:, :, 2] + A_TRUE * rs.standard_normal(f.shape[:2])
    else:
        obs[:, :, 0] = f[:, :, 0] + A_TRUE * rs.standard_normal(f.shape[:2])
        obs[:, :, 1] = negbin_draw(rs, f[:, :, 1], b)
    obs[rs.uniform(size=obs.shape) < 0.15] = np.nan
    return t, obs


def plant(t, obs, count=1, gauss=0):
    """Planted records on the two-output data: zeros, counts up to 2000, an all-NaN count column in one experiment (an experiment
    with no count), a Gaussian value beside a missing count and the other way round.  Row 2 is ragged already."""
    obs = obs.copy()
    obs[0, 0:3, count] = 0.0                      # the mean is 0 at t = 0 for V B: mu = 0 with y = 0
    obs[0, 7, count], obs[1, 9, count], obs[1, 10, count] = 2000.0, 1999.0, 1.0
    obs[3, :, count] = np.nan                      # no count in experiment 3
    obs[1, 4, gauss], obs[1, 5, count] = np.nan, np.nan
    obs[2, 20:, :] = 7.0                           # past the row's end: ignored
    return obs


def _user_models():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as g
    return g.load_package().user_models


def log_post(theta, t, obs, um, counts_gaussian):
    high = GAUSS_PRIOR_HIGH if counts_gaussian else PRIOR_HIGH
    if np.any(theta <= 0) or np.any(theta >= high) or theta[0] == theta[1]:
        return -np.inf
    pred = closed_form(theta[0], theta[1], t)[None]
    if counts_gaussian:
        return float(um.noise_loglik(pred, t, obs, theta[None], NOISE_GAUSS)[0])
    return float(um.count_loglik(pred, t, obs, theta[None], (0, 2), NOISE_NB)[0])


def chain(t, obs, n, cov, start, rs, um, counts_gaussian):
    L = np.linalg.cholesky(cov)
    x, lp = start.copy(), log_post(start, t, obs, um, counts_gaussian)
    out = np.empty((n, x.size))
    acc = 0
    for i in range(n):
        y = x + L @ rs.standard_normal(x.size)
        ly = log_post(y, t, obs, um, counts_gaussian)
        if np.log(rs.uniform()) < ly - lp:
            x, lp = y, ly
            acc += 1
        out[i] = x
    return out, acc / n


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    um = _user_models()
    t, obs = make_data(seed)
    np.set_printoptions(precision=5, suppress=True)
    means = {}
    for gaussian in (False, True):
        rs = np.random.RandomState(1000 + seed)
        start = THETA_TRUE.copy()
        if gaussian:
            start[3] = 0.3 * np.nanstd(obs[:, :, 1])
        step = np.array([0.006, 0.006, 0.001, 0.05 if not gaussian else 0.1 * start[3]])
        pilot, _ = chain(t, obs, 20000, np.diag(step ** 2), start, rs, um, gaussian)
        cov = np.cov(pilot[5000:].T) * 2.4 ** 2 / 4
        xs, rate = chain(t, obs, n + 5000, cov, pilot[-1], rs, um, gaussian)
        xs = xs[5000:]
        half = n // 2
        name = "counts declared Gaussian" if gaussian else "negative binomial"
        print(f"{name}: data seed {seed}, V {V}, {n} samples, acceptance {rate:.3f}")
        print("mean", repr(xs.mean(axis=0)))
        print("sd  ", repr(xs.std(axis=0)))
        print("half-chain means differ by (in sd)", np.abs(xs[:half].mean(axis=0) - xs[half:].mean(axis=0)) / xs.std(axis=0))
        means[gaussian] = (xs.mean(axis=0), xs.std(axis=0), np.abs(xs[:half].mean(axis=0) - xs[half:].mean(axis=0)))
    m, sd, spread = means[False]
    print("Gaussian declaration off by (in negative-binomial chain sd)", (means[True][0][:3] - m[:3]) / sd[:3],
          "half-chain spread (in sd)", np.maximum(spread, means[True][2])[:3] / sd[:3])


if __name__ == "__main__":
    main()
