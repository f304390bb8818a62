"""Prior families (include/smc_hip.h: PRIOR FAMILIES): the `priors` dict of SMCSettings / HipEngine.set_prior as the
arrays of smc_set_prior_ex, and the definitions in NumPy of what the kernels form.

    {"dist": "uniform", "low", "high"}  {"dist": "normal" | "flat", "mu", "sigma"}                    as before (smc_set_prior)
    {"dist": "lognormal", "mu", "sigma"}                 x > 0            k = -L - (L - mu)^2 / (2 sigma^2), L = log x
    {"dist": "gamma", "shape", "scale"}                  x > 0            k = (shape - 1) log x - x / scale      (shape >= 1/16;
                                                                          a beta's a, b too: the draws need it)
    {"dist": "beta", "a", "b", "low" = 0, "high" = 1}    low < x < high   k = (a - 1) log u + (b - 1) log1p(-u), u = (x - low) / (high - low)
                                                         (and 0 < u < 1 as rounded: an x within an ulp of an end is outside)
    {"dist": "truncnormal", "mu", "sigma", "low" = -inf, "high" = +inf}   low <= x <= high   k = -y^2 / 2, y = (x - mu) / sigma
    {"dist": "halfnormal", "sigma"}                      truncnormal(0, sigma, 0, +inf)

k is the log-kernel, the log-density without its normaliser; a density only acts under prior_mode "ratio_mask" / "ratio" - "mask"
applies the support alone."""
from __future__ import annotations

import math

import numpy as np

from . import binding as B

from .binding import SMC_PRIOR_BETA, SMC_PRIOR_GAMMA, SMC_PRIOR_LOGNORMAL, SMC_PRIOR_TRUNCNORMAL

NEW_KINDS = (SMC_PRIOR_LOGNORMAL, SMC_PRIOR_GAMMA, SMC_PRIOR_BETA, SMC_PRIOR_TRUNCNORMAL)
_KEYS = {"uniform": (B.SMC_PRIOR_UNIFORM, "low", "high"), "normal": (B.SMC_PRIOR_NORMAL, "mu", "sigma"),
         "flat": (B.SMC_PRIOR_FLAT, "mu", "sigma"), "lognormal": (SMC_PRIOR_LOGNORMAL, "mu", "sigma"),
         "gamma": (SMC_PRIOR_GAMMA, "shape", "scale"), "beta": (SMC_PRIOR_BETA, "a", "b"),
         "truncnormal": (SMC_PRIOR_TRUNCNORMAL, "mu", "sigma")}


def _arrays(priors: dict):
    kind, a, b, lo, hi = [], [], [], [], []
    for i, (name, p) in enumerate(priors.items()):
        dist = p["dist"]
        if dist == "halfnormal":
            p = {"dist": "truncnormal", "mu": 0.0, "sigma": p["sigma"], "low": 0.0, "high": math.inf}
            dist = "truncnormal"
        if dist not in _KEYS:
            raise ValueError(f"Unknown prior: {dist} (parameter {i}, {name!r})")
        k, ka, kb = _KEYS[dist]
        try:
            a.append(float(p[ka]))
            b.append(float(p[kb]))
        except KeyError as e:
            raise ValueError(f"parameter {i} ({name!r}): a {dist} prior needs the key {e.args[0]!r}") from None
        kind.append(k)
        if k == SMC_PRIOR_BETA:
            lo.append(float(p.get("low", 0.0)))
            hi.append(float(p.get("high", 1.0)))
        elif k == SMC_PRIOR_TRUNCNORMAL:
            lo.append(float(p.get("low", -math.inf)))
            hi.append(float(p.get("high", math.inf)))
        else:
            lo.append(0.0)
            hi.append(0.0)
    return (np.array(kind, dtype=np.int32), np.array(a, dtype=np.float64), np.array(b, dtype=np.float64),
            np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64))


def prior_layout(priors: dict):
    """(kind, a, b, lo, hi): the five arrays of smc_set_prior_ex for the dict, one entry per parameter in order.  ValueError with the
    library's reason (smc_prior_check: the parameter's index and the rule) for a specification that breaks a rule."""
    kind, a, b, lo, hi = _arrays(priors)
    dp = lambda x: x.ctypes.data_as(B.c_dp)      # noqa: E731
    L = B.lib()
    if L.smc_prior_check(kind.ctypes.data_as(B.c_ip), dp(a), dp(b), dp(lo), dp(hi), len(kind)) != 0:
        raise ValueError(L.smc_last_error(None).decode())
    return kind, a, b, lo, hi


def has_new_kind(priors: dict) -> bool:
    return any(p["dist"] in ("lognormal", "gamma", "beta", "truncnormal", "halfnormal") for p in priors.values())


def _columns(priors, theta):
    """theta as (n, d): a 2-D array of n rows, or ONE row given as a 1-D vector of d values.  Anything else is refused - a vector
    of n values of a one-parameter prior is written theta[:, None]."""
    kind, a, b, lo, hi = _arrays(priors)
    theta = np.asarray(theta, dtype=np.float64)
    if theta.ndim == 1 and theta.shape[0] == len(kind):
        theta = theta[None, :]
    if theta.ndim != 2 or theta.shape[1] != len(kind):
        raise ValueError(f"theta has shape {theta.shape}: expected (n, {len(kind)}), or one row of {len(kind)} values")
    return kind, a, b, lo, hi, theta


def _k_column(k, a, b, lo, hi, x):
    """log-kernel of one new-kind parameter: -inf outside the support, NaN for NaN (csrc/prior.h: prior_log_kernel)"""
    out = np.full(x.shape, -np.inf)
    with np.errstate(all="ignore"):
        if k == SMC_PRIOR_TRUNCNORMAL:
            m = (x >= lo) & (x <= hi)
            y = (x[m] - a) / b
            out[m] = -(y * y) / 2.0
        elif k == SMC_PRIOR_BETA:
            u = (x - lo) / (hi - lo)
            m = (x > lo) & (x < hi) & (u > 0.0) & (u < 1.0)
            out[m] = (a - 1.0) * np.log(u[m]) + (b - 1.0) * np.log1p(-u[m])
        else:
            m = (x > 0.0) & (x < np.inf)
            L = np.log(x[m])
            out[m] = -L - (L - a) ** 2 / (2.0 * (b * b)) if k == SMC_PRIOR_LOGNORMAL else (a - 1.0) * L - x[m] / b
    out[np.isnan(x)] = np.nan
    return out


def prior_log_kernel(priors: dict, theta) -> np.ndarray:
    """K(theta): the sum over the new-kind parameters of their log-kernels, per row of theta (n, d) - what the propose kernels form
    beside P, the product of the uniform / normal densities.  -inf where a new-kind parameter is outside its support, NaN for NaN;
    0 for a dict without new kinds."""
    kind, a, b, lo, hi, theta = _columns(priors, theta)
    K = np.zeros(theta.shape[0])
    with np.errstate(invalid="ignore"):
        for c in range(len(kind)):
            if kind[c] in NEW_KINDS:
                K = K + _k_column(kind[c], a[c], b[c], lo[c], hi[c], theta[:, c])
    return K


def prior_support(priors: dict, theta) -> np.ndarray:
    """True where every parameter of the row is in its prior's support (uniform: the closed box; normal, flat: anywhere; the new
    kinds: the table above).  A NaN is nowhere."""
    kind, a, b, lo, hi, theta = _columns(priors, theta)
    ok = ~np.isnan(theta).any(axis=1)
    with np.errstate(all="ignore"):
        for c in range(len(kind)):
            x = theta[:, c]
            if kind[c] == B.SMC_PRIOR_UNIFORM:
                y = (x - a[c]) / (b[c] - a[c])
                ok &= (y >= 0.0) & (y <= 1.0)
            elif kind[c] in NEW_KINDS:
                ok &= _k_column(kind[c], a[c], b[c], lo[c], hi[c], x) > -np.inf
    return ok


def _phi_diff(zl, zh):
    """Phi(zh) - Phi(zl), with erfc on the side where it is accurate"""
    r = math.sqrt(0.5)
    if zl > 0.0:
        return 0.5 * math.erfc(zl * r) - 0.5 * math.erfc(zh * r)
    return 0.5 * math.erfc(-zh * r) - 0.5 * math.erfc(-zl * r)


def prior_logpdf(priors: dict, theta) -> np.ndarray:
    """The normalised log-density of the whole prior per row of theta: the sum of the parameters' log-densities (a flat one adds
    nothing), -inf outside the support."""
    kind, a, b, lo, hi, theta = _columns(priors, theta)
    out = np.zeros(theta.shape[0])
    with np.errstate(all="ignore"):
        for c in range(len(kind)):
            x, k = theta[:, c], kind[c]
            if k == B.SMC_PRIOR_FLAT:
                term = np.where(np.isnan(x), np.nan, 0.0)
            elif k == B.SMC_PRIOR_UNIFORM:
                y = (x - a[c]) / (b[c] - a[c])
                term = np.where((y >= 0.0) & (y <= 1.0), -math.log(b[c] - a[c]), -np.inf)
                term = np.where(np.isnan(x), np.nan, term)
            elif k == B.SMC_PRIOR_NORMAL:
                y = (x - a[c]) / b[c]
                term = -(y * y) / 2.0 - math.log(b[c]) - 0.5 * math.log(2.0 * math.pi)
            else:
                if k == SMC_PRIOR_LOGNORMAL:
                    norm = math.log(b[c]) + 0.5 * math.log(2.0 * math.pi)
                elif k == SMC_PRIOR_GAMMA:
                    norm = math.lgamma(a[c]) + a[c] * math.log(b[c])
                elif k == SMC_PRIOR_BETA:
                    norm = math.lgamma(a[c]) + math.lgamma(b[c]) - math.lgamma(a[c] + b[c]) + math.log(hi[c] - lo[c])
                else:
                    norm = math.log(b[c]) + 0.5 * math.log(2.0 * math.pi) + math.log(_phi_diff((lo[c] - a[c]) / b[c], (hi[c] - a[c]) / b[c]))
                term = _k_column(k, a[c], b[c], lo[c], hi[c], x) - norm
            out = out + term
    return out


def sample_new_kind(p: dict, n: int) -> np.ndarray:
    """One parameter's n draws from the global NumPy stream (driver.sample_prior, rng="numpy"): np.random.lognormal, np.random.gamma,
    low + (high - low) * np.random.beta; for a truncated normal np.random.normal(size=n), then redraws of exactly the
    out-of-range entries until none is left."""
    kind, a, b, lo, hi = (v[0] for v in _arrays({"p": p}))
    if kind == SMC_PRIOR_LOGNORMAL:
        return np.random.lognormal(mean=a, sigma=b, size=n)
    if kind == SMC_PRIOR_GAMMA:
        return np.random.gamma(shape=a, scale=b, size=n)
    if kind == SMC_PRIOR_BETA:
        return lo + (hi - lo) * np.random.beta(a, b, size=n)
    x = np.random.normal(loc=a, scale=b, size=n)
    bad = np.flatnonzero(~((x >= lo) & (x <= hi)))
    while bad.size:
        x[bad] = np.random.normal(loc=a, scale=b, size=bad.size)
        bad = bad[~((x[bad] >= lo) & (x[bad] <= hi))]
    return x
