"""The model, populations and data of tests/test_user_pointwise.py: a user model whose outputs ARE its parameters (as
tests/planted_values.py), so that a test plants the means, noise levels and overdispersions it wants and NumPy on the uploaded
array alone says what the pointwise kernels (csrc/pointwise_kernels.hip) must see.  A helper module, not a test.

The model.  One state, y0 = 0, rhs = 0 (RK45 is exact on it) and
    out[k] = theta[gate] < cond[0] ? theta[k] : NaN      (k < n_obs)
theta[gate] is the GATE, a permutation of i + 0.5 (i < n): an experiment with cond = j leaves exactly min(j, n) particles finite in
its cells, so cells with 0, 1, 2, 3 and 40 finite particles sit next to full ones (cond = 1e18), and the data does not depend on n.
A NaN output is no failed solve.

VARIANTS: name -> the layout of theta, the likelihood and what set_model_user gets.
    one          the one-output model (smc_user_obs, 2-D obs), theta = (m0, gate, sigma), sigma estimated
    sigma_est    two outputs under the sigma rule, theta = (m0, m1, gate, sigma)
    sigma_fixed  ... with sigma fixed at 0.3, theta = (m0, m1, gate)
    noise        additive + proportional noise with obs_scale (1, 2.5), theta = (m0, m1, a0, a1, b0, gate); b1 fixed 0.1
    censored     the same with left- and right-censored values
    counts       (Gaussian, Poisson, negative binomial), theta = (m0, mu1, mu2, a0, b2, gate): smc_user_obs_family {0, 1, 2}"""
import numpy as np

VARIANTS = {
    "one": dict(n_obs=1, dim=3, gate=1, one_output=True, noise={"additive": [("param", 2)]}, kw={}),
    "sigma_est": dict(n_obs=2, dim=4, gate=2, noise={"additive": [("param", 3)] * 2}, kw={}),
    "sigma_fixed": dict(n_obs=2, dim=3, gate=2, noise={"additive": [("fixed", 0.3)] * 2}, kw={"est_sigma": False, "sigma_fixed": 0.3}),
    "noise": dict(n_obs=2, dim=6, gate=5, noise={"additive": [("param", 2), ("param", 3)], "proportional": [("param", 4), ("fixed", 0.1)]},
                  obs_scale=(1.0, 2.5), pass_noise=True, kw={}),
    "censored": dict(n_obs=2, dim=6, gate=5, noise={"additive": [("param", 2), ("param", 3)], "proportional": [("param", 4), ("fixed", 0.1)]},
                     obs_scale=(1.0, 2.5), pass_noise=True, censored=True, kw={}),
    "counts": dict(n_obs=3, dim=6, gate=5, family=(0, 1, 2), pass_noise=True, kw={},
                   noise={"additive": [("param", 3), ("fixed", 1.0), ("fixed", 1.0)], "proportional": [("fixed", 0.0), ("fixed", 0.0), ("param", 4)]}),
}

# cells -> (n_ex, n_t, finite particles per experiment as (kind, value), the row cut short and after how many times, or None)
_ALL, _HALF = ("j", 10 ** 18), ("j", 40)
_ELEVEN = [_ALL, _HALF, ("j", 3), ("j", 2), ("j", 1), ("j", 0), _ALL, _HALF, ("j", 3), ("j", 2), ("j", 1)]
DESIGNS = {      # by n_obs
    1: {1: (1, 1, [_ALL], None), 8: (2, 4, [_ALL, _HALF], None)},      # the one-output model takes neither NaN nor a short row
    2: {8: (2, 2, [_ALL, _HALF], (1, 1)), 32: (2, 8, [_ALL, ("j", 3)], (1, 5)), 264: (11, 12, _ELEVEN, (6, 7))},
    3: {36: (6, 2, [_ALL, _HALF, ("j", 3), ("j", 2), ("j", 1), ("j", 0)], (1, 1)), 264: (11, 8, _ELEVEN, (6, 3))},
}


def source(name):
    """HIP text of the variant's model."""
    v = VARIANTS[name]
    sig = "const double *theta, const double *cond"
    head = (f"__device__ void smc_user_y0({sig}, double *y) {{ y[0] = 0.0; }}\n"
            f"__device__ void smc_user_rhs(double t, const double *y, {sig}, double *dydt) {{ dydt[0] = 0.0; }}\n")
    nan = "__longlong_as_double(0x7ff8000000000000LL)"
    if v.get("one_output"):
        return head + f"__device__ double smc_user_obs(double t, const double *y, {sig}) {{ return theta[{v['gate']}] < cond[0] ? theta[0] : {nan}; }}\n"
    fam = "" if "family" not in v else "__device__ const int smc_user_obs_family[] = {" + ", ".join(str(f) for f in v["family"]) + "};\n"
    rows = "\n".join(f"    out[{k}] = open ? theta[{k}] : {nan};" for k in range(v["n_obs"]))
    return (fam + head + f"__device__ void smc_user_obs_vec(double t, const double *y, {sig}, double *out) {{\n"
            f"    const bool open = theta[{v['gate']}] < cond[0];\n{rows}\n}}\n")


def priors(name):
    return {f"p{j}": {"dist": "uniform", "low": -1e9, "high": 1e9} for j in range(VARIANTS[name]["dim"])}


def population(name, n, seed, invalid=False):
    """(n, dim) particles: means about 1 (counts: Poisson means up to 50 with exact zeros among them, negative-binomial means up to
    5000), noise levels in (0.05, 0.3), overdispersions in (0.05, 1), the gate a permutation of i + 0.5.  invalid: up to
    three particles get parameters that make logL -inf: an a_k <= 0, a b_k < 0, b_k = 0 on the negative-binomial output (sigma_fixed
    has no such parameter)."""
    v = VARIANTS[name]
    rs = np.random.RandomState(seed)
    th = np.empty((n, v["dim"]))
    th[:, 0] = 1.0 + 0.5 * rs.standard_normal(n)
    if name == "one":
        th[:, 2] = rs.uniform(0.05, 0.3, n)
        if invalid:
            th[0, 2] = 0.0
    elif name in ("sigma_est", "sigma_fixed"):
        th[:, 1] = -2.0 + 0.5 * rs.standard_normal(n)
        if name == "sigma_est":
            th[:, 3] = rs.uniform(0.05, 0.3, n)
            if invalid:
                th[0 % n, 3], th[1 % n, 3] = 0.0, -0.2
    elif name in ("noise", "censored"):
        th[:, 1] = -2.0 + 0.5 * rs.standard_normal(n)
        th[:, 2], th[:, 3], th[:, 4] = rs.uniform(0.05, 0.3, n), rs.uniform(0.05, 0.3, n), rs.uniform(0.0, 0.3, n)
        if invalid:
            th[0 % n, 2], th[1 % n, 4] = 0.0, -0.1
    else:
        th[:, 1] = np.where(rs.uniform(size=n) < 0.2, 0.0, rs.uniform(0.0, 50.0, n))
        th[:, 2] = 10.0 ** rs.uniform(-1, 3.7, n)
        th[:, 3], th[:, 4] = rs.uniform(0.05, 0.3, n), rs.uniform(0.05, 1.0, n)
        if invalid:
            th[0 % n, 3], th[1 % n, 4], th[2 % n, 4] = 0.0, 0.0, -0.2
    th[:, v["gate"]] = rs.permutation(n) + 0.5
    return th


def make(name, cells, seed=0):
    """The data of the variant on the design with that many cells: {"t" (n_ex, n_t) with one row cut short, "cond" (n_ex, 1) gate
    thresholds (finite(d, n): the particles they leave finite), "obs", "censor" (or None), "family" (or None), "noise",
    "obs_scale" (or None) - what user_models.pointwise_loglik takes - and "kw", the keyword arguments of set_model_user}.  About a
    sixth of the values are NaN; counts are at most 10^4, with zeros and - next to Poisson means of 0 - positive counts."""
    v = VARIANTS[name]
    n_obs = v["n_obs"]
    n_ex, n_t, kinds, short = DESIGNS[n_obs][cells]
    rs = np.random.RandomState(1000 + seed)
    cond = np.array([float(j) for _, j in kinds])[:, None]
    t = np.tile(np.arange(n_t, dtype=np.float64), (n_ex, 1))
    if short is not None:
        t[short[0], short[1]:] = np.nan
    obs = np.empty((n_ex, n_t, n_obs))
    obs[:, :, 0] = 1.0 + 0.6 * rs.standard_normal((n_ex, n_t))
    if n_obs >= 2:
        obs[:, :, 1] = -2.0 + 0.6 * rs.standard_normal((n_ex, n_t))
    family = v.get("family")
    if family is not None:
        obs[:, :, 1] = np.where(rs.uniform(size=(n_ex, n_t)) < 0.25, 0.0, rs.poisson(20.0, (n_ex, n_t)))
        obs[:, :, 2] = np.where(rs.uniform(size=(n_ex, n_t)) < 0.2, 0.0, np.floor(10.0 ** rs.uniform(0, 4, (n_ex, n_t))))
    if not v.get("one_output"):
        obs[rs.uniform(size=obs.shape) < 1.0 / 6.0] = np.nan
        obs[0, 0, 0] = 1.1      # at least one quantified value
    if family is not None:      # in the first (full) experiment: a zero and a positive count on the Poisson output, a zero on the other
        obs[0, 0, 1], obs[0, n_t - 1, 1], obs[0, 0, 2] = 0.0, 7.0, 0.0
    censor = None
    if v.get("censored"):
        censor = np.where(np.isnan(obs) | np.isnan(t)[:, :, None], 0, rs.randint(-1, 2, obs.shape)).astype(np.int8)
        censor[0, 0, 0] = 0
    kw = dict(v["kw"])
    if v.get("pass_noise"):
        kw["noise"] = v["noise"]
    if "obs_scale" in v:
        kw["obs_scale"] = v["obs_scale"]
    if censor is not None:
        kw["censor"] = censor
    return {"t": t, "cond": cond, "obs": obs[:, :, 0] if v.get("one_output") else obs, "censor": censor,
            "family": family, "noise": v["noise"], "obs_scale": v.get("obs_scale"), "kw": kw}


def finite(d, n):
    """(n_ex,) the particles of a population of n that are finite in each experiment's cells"""
    return np.minimum(d["cond"][:, 0], n).astype(np.int64)


def planted(name, th, d):
    """What the model predicts, (n, n_ex, n_t, n_obs): NumPy on the uploaded particles alone."""
    v = VARIANTS[name]
    is_open = th[:, v["gate"], None] < d["cond"][None, :, 0]
    served = ~np.isnan(d["t"])
    return np.where(is_open[:, :, None, None] & served[None, :, :, None], th[:, None, None, :v["n_obs"]], np.nan)
