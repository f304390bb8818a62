"""The grids, planted models and 60-digit truth behind tests/test_likelihood_terms_truth.py and its fixture
tests/golden/likelihood_terms_truth.npz (written by tests/golden/make_likelihood_terms_truth.py).  A helper module, not a test.

Every GPU test of the likelihood terms compares the device with the NumPy definitions of user_models.py, which are written
operation for operation as the kernels: an error of the formula itself is made on both sides.  Here each term is held to its
mathematical value, computed with mpmath at 60 digits FROM THE FLOAT64 INPUTS (so the rounding of the inputs is no part of the
error), under the bar the project holds count_loglik to against SciPy:  |term - truth| <= 1e-11 max(1, |truth|).  A sum (the lk
of a particle) passes within the sum of its terms' bars.

Every input is formed from decimal literals with +, -, *, / and sqrt alone, which IEEE 754 rounds the same everywhere, so the
grids are the same bits on every machine and the fixture holds the truth alone.  mpmath is needed by the generator only.

COUNTS.  y in Y, mu = f max(y, 1) with f in F (both sides of mu = y, of the series of bd0 and of its m < x / 2 switch), the
negative binomial with b in B - the last N_B_RECORD of them "record only": there phi + y no longer holds y, and the tests assert
finite and >= 0 alone.  Truth: Poisson excess mu - y - y log(mu / y) (y = 0: mu; mu = 0 < y: +inf), floor c(y) = loggamma(y + 1) -
y log y + y, negative binomial minus the log-pmf from loggamma with phi = 1 / b^2.
The planted model has ONE EXPERIMENT PER y and lets the particle choose its experiment: theta = (f, b, j), cond = (max(y_e, 1), e,
y_e), out = (e == j) ? f max(y_e, 1) : y_e.  Off its experiment a particle predicts mu = y, where the Poisson excess is exactly
0 and the negative-binomial term is the grid's own f = 1 entry (y = 0: mu = 0, the term is exactly 0): a particle's lk holds one term under test beside eleven of size
<= 20, and a wrong term is not averaged away.

CENSORED and GAUSSIAN.  One output with obs_scale s in SCALES, theta = (f, a, b, j), three experiments: e = 0 left-censored at
obs = +128, e = 1 right-censored at obs = -128, e = 2 quantified at obs = 0.5; out = (e == j) ? f : 0.  Off its experiment a
particle has z = 128 / (a s) > 40, where -log Phi(z) is exactly 0 (censored), and the Gaussian term at f = 0, which is of size 1.
  censored: z in +-(1e-3 .. 1e3 by half decades), 0 (the right flag makes it -0), 38.5, 40, 45, -1e4, -1e8, -1e100, -1e154, each
            reached with b f = 0, b f = 1e-4 a s and b f = 1e4 a s (z = -1e154 with b f = 0 alone: beyond it f^2 overflows), from
            the left and from the right.  Truth -log Phi(z): erfc at 60 digits, below z = -1e3 the asymptotic series.
  Gaussian: |r| / sd in RHO times u = (b f / (a s))^2 in U.  Truth: the normal log-density with sd^2 = (a s)^2 + (b f)^2."""
import functools
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "likelihood_terms_truth.npz")
BAR = 1e-11
DPS = 60

Y = np.array([0.0, 1.0, 2.0, 3.0, 7.0, 30.0, 100.0, 1000.0, 31623.0, 1e6, 1e9, 2.0 ** 53])
F = np.array([0.0, 1e-300, 1e-5, 0.25, 0.5 - 1e-12, 0.5, 0.5 + 1e-12, 0.9, 0.99, 1.0 - 1e-9, 1.0, 1.0 + 1e-9, 1.01, 2.0, 1e3, 1e5])
F_ONE = 10                                   # F[F_ONE] = 1: mu = y
B = np.array([10.0, 3.0, 1.0, 0.3, 0.05, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8])
N_B_RECORD = 2                               # the last two: record only
MU = F[None, :] * np.maximum(Y, 1.0)[:, None]                                   # (y, f)

SCALES = (1.0, 2.5)
L_CENS, OBS_G, A_GC = 128.0, 0.5, 0.7
_HALF = [float(f"{m}e{k}") for k in range(-3, 3) for m in ("1", "3.1622776601683795")] + [1e3]
Z_TARGETS = [s * h for h in _HALF for s in (1.0, -1.0)] + [0.0, 38.5, 40.0, 45.0, -1e4, -1e8, -1e100, -1e154]
RATIOS = (0.0, 1e-4, 1e4)                    # b f / (a s)
RHO = (0.0, 1e-8, 1.0, 30.0, 1e3)
U = (0.0, 1e-20, 1e-3, 1.0, 1e6, 1e20)
LEFT, RIGHT, GAUSS = 0, 1, 2
NOISE_NB = {"additive": [("fixed", 1.0)], "proportional": [("param", 1)]}
NOISE_GC = {"additive": [("param", 1)], "proportional": [("param", 2)]}

_HEAD = ("__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = 0.0; }\n"
         "__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) { dydt[0] = 0.0; }\n"
         "__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) ")


# ---- the planted models ----------------------------------------------------------------------------------------------------------
def count_source(family):
    return (f"__device__ const int smc_user_obs_family[] = {{{int(family)}}};\n" + _HEAD
            + "{ out[0] = (cond[1] == theta[2]) ? theta[0] * cond[0] : cond[2]; }\n")


def count_data():
    """t (12, 2), obs (12, 2, 1) with the count at the second time, cond (12, 3)"""
    e = np.arange(Y.size, dtype=np.float64)
    t = np.tile([0.0, 1.0], (Y.size, 1))
    obs = np.full((Y.size, 2, 1), np.nan)
    obs[:, 1, 0] = Y
    return t, obs, np.column_stack([np.maximum(Y, 1.0), e, Y])


def count_particles(family):
    """theta (n, 3) = (f, b, j) in the order of the fixture's arrays: Poisson (y, f), negative binomial (y, f, b); and j (n,)"""
    if family == 1:
        j, i = np.meshgrid(np.arange(Y.size), np.arange(F.size), indexing="ij")
        b = np.zeros(j.size)
    else:
        j, i, k = np.meshgrid(np.arange(Y.size), np.arange(F.size), np.arange(B.size), indexing="ij")
        b = B[k.ravel()]
    j = j.ravel()
    return np.column_stack([F[i.ravel()], b, j.astype(np.float64)]), j


def count_planted(th):
    """what the count model predicts, (n, 12, 2, 1)"""
    t, obs, cond = count_data()
    live = cond[None, :, 1] == th[:, 2, None]
    mu = np.where(live, th[:, 0, None] * cond[None, :, 0], cond[None, :, 2])
    return np.repeat(mu[:, :, None, None], 2, axis=2)


def gc_source():
    return _HEAD + "{ out[0] = (cond[0] == theta[3]) ? theta[0] : 0.0; }\n"


def gc_data():
    """t (3, 2), obs (3, 2, 1), censor (3, 2, 1), cond (3, 1)"""
    t = np.tile([0.0, 1.0], (3, 1))
    obs = np.full((3, 2, 1), np.nan)
    obs[:, 1, 0] = (L_CENS, -L_CENS, OBS_G)
    censor = np.zeros((3, 2, 1), dtype=np.int8)
    censor[LEFT, 1, 0], censor[RIGHT, 1, 0] = -1, 1
    return t, obs, censor, np.arange(3, dtype=np.float64)[:, None]


@functools.lru_cache(maxsize=None)
def _gc_particles(s):
    rows = []
    for z in Z_TARGETS:
        for ratio in (RATIOS if z != -1e154 else RATIOS[:1]):
            for flag in (LEFT, RIGHT):
                a = A_GC if z != -1e154 else 0.5 / s
                as_ = a * s
                c = ratio * as_
                sd = np.sqrt(as_ * as_ + c * c)
                f = L_CENS - z * sd if flag == LEFT else -L_CENS + z * sd
                assert f != 0.0
                rows.append((f, a, c / abs(f), float(flag)))
    for ir, rho in enumerate(RHO):
        for iu, u in enumerate(U):
            as_ = A_GC * s
            sd = as_ * np.sqrt(1.0 + u)
            f = OBS_G + (rho * sd if (ir + iu) % 2 else -(rho * sd))
            assert f != 0.0
            rows.append((f, A_GC, np.sqrt(u) * as_ / abs(f), float(GAUSS)))
    return np.array(rows)


def gc_particles(s):
    """theta (n, 4) = (f, a, b, j) for obs_scale s, in the order of the fixture's arrays; and j (n,)"""
    th = _gc_particles(float(s)).copy()
    return th, th[:, 3].astype(np.int64)


def gc_planted(th):
    """what the censored / Gaussian model predicts, (n, 3, 2, 1)"""
    live = np.arange(3.0)[None, :] == th[:, 3, None]
    return np.repeat(np.where(live, th[:, 0, None], 0.0)[:, :, None, None], 2, axis=2)


def mask(j, n_ex):
    """(n, n_ex) the (particle, cell) pairs whose term the fixture holds: a particle's own experiment"""
    return np.arange(n_ex)[None, :] == np.asarray(j)[:, None]


def bar(truth):
    truth = np.asarray(truth, dtype=np.float64)
    return BAR * np.maximum(1.0, np.abs(truth))


def rel(got, truth):
    """|got - truth| / max(1, |truth|), 0 where both are the same infinity"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isinf(truth) & (got == truth), 0.0, np.abs(got - truth) / np.maximum(1.0, np.abs(truth)))


def load():
    return dict(np.load(FIXTURE))


# ---- the truth (mpmath) ----------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath.mp


@functools.lru_cache(maxsize=None)
def floor_truth(j):
    mp = _mp()
    y = mp.mpf(float(Y[j]))
    return mp.mpf(0) if y == 0 else mp.loggamma(y + 1) - y * mp.log(y) + y


@functools.lru_cache(maxsize=None)
def poisson_truth(j, i):
    mp = _mp()
    y, mu = mp.mpf(float(Y[j])), mp.mpf(float(MU[j, i]))
    if y == 0:
        return mu
    return mp.inf if mu == 0 else mu - y - y * mp.log(mu / y)


@functools.lru_cache(maxsize=None)
def negbin_truth(j, i, k):
    mp = _mp()
    y, mu, b = mp.mpf(float(Y[j])), mp.mpf(float(MU[j, i])), mp.mpf(float(B[k]))
    phi = 1 / (b * b)
    if mu == 0:
        return mp.mpf(0) if y == 0 else mp.inf
    return -(mp.loggamma(y + phi) - mp.loggamma(phi) - mp.loggamma(y + 1) + phi * mp.log(phi / (phi + mu)) + y * mp.log(mu / (phi + mu)))


def neg_log_phi(z):
    """-log Phi(z) of an mpf"""
    mp = _mp()
    if z < -1000:      # Phi(z) = exp(-z^2 / 2) / (|z| sqrt(2 pi)) (1 - 1 / z^2 + 3 / z^4 - 15 / z^6 + ...): 12 terms, below 1e-70
        term, total = mp.mpf(1), mp.mpf(1)
        for m in range(1, 13):
            term = -term * (2 * m - 1) / (z * z)
            total += term
        return z * z / 2 + mp.log(2 * mp.pi) / 2 + mp.log(-z) - mp.log(total)
    if z > 0:
        return -mp.log1p(-mp.erfc(z / mp.sqrt(2)) / 2)
    return -mp.log(mp.erfc(-z / mp.sqrt(2)) / 2)


def _gc_cell(e, f, a, b, s):
    """the term of experiment e at the prediction f (mpf from float64)"""
    mp = _mp()
    f, a, b, s = (mp.mpf(float(v)) for v in (f, a, b, s))
    sd2 = (a * s) ** 2 + (b * f) ** 2
    if e == LEFT:
        return -neg_log_phi((L_CENS - f) / mp.sqrt(sd2))
    if e == RIGHT:
        return -neg_log_phi((f + L_CENS) / mp.sqrt(sd2))
    r = OBS_G - f
    return -mp.log(2 * mp.pi * sd2) / 2 - r * r / (2 * sd2)


def _sum_and_bar(terms):
    mp = _mp()
    if any(mp.isinf(v) for v in terms):
        return -np.inf, np.inf
    return float(mp.fsum(terms)), float(BAR * mp.fsum(max(mp.mpf(1), abs(v)) for v in terms))


def entry(name, idx):
    """One entry of the fixture's array `name` as float64.  The arrays:
        floor (y,)            c(y)                       pois_x (y, f)   the Poisson excess      nb_x (y, f, b)  minus the log-pmf
        pois_lk, nb_lk        the lk of the particle that plants the entry: its term and the eleven of the other experiments at
                              mu = y (Poisson: every floor, excess 0), summed at 60 digits;  *_bar: the sum of the terms' bars
        gc_l_<n> (particle,)  the term of a censored / Gaussian particle's own experiment for obs_scale SCALES[n]
        gc_lk_<n>, gc_bar_<n> its lk over the three experiments, and the sum of their bars"""
    idx = tuple(int(v) for v in np.atleast_1d(idx))
    if name == "floor":
        return float(floor_truth(*idx))
    if name == "pois_x":
        return float(poisson_truth(*idx))
    if name == "nb_x":
        return float(negbin_truth(*idx))
    if name in ("pois_lk", "pois_bar"):
        j, i = idx
        terms = [-(floor_truth(e) + (poisson_truth(j, i) if e == j else 0)) for e in range(Y.size)]
        return _sum_and_bar(terms)[name == "pois_bar"]
    if name in ("nb_lk", "nb_bar"):
        j, i, k = idx
        terms = [-negbin_truth(e, i, k) if e == j else (-negbin_truth(e, F_ONE, k) if Y[e] > 0 else _mp().mpf(0)) for e in range(Y.size)]
        return _sum_and_bar(terms)[name == "nb_bar"]
    kind, n = name.rsplit("_", 1)
    s = SCALES[int(n)]
    f, a, b, j = _gc_particles(float(s))[idx[0]]
    if kind == "gc_l":
        return float(_gc_cell(int(j), f, a, b, s))
    terms = [_gc_cell(e, f if e == int(j) else 0.0, a, b, s) for e in range(3)]
    return _sum_and_bar(terms)[kind == "gc_bar"]


def shapes():
    n_gc = _gc_particles(1.0).shape[0]
    out = {"floor": (Y.size,), "pois_x": MU.shape, "pois_lk": MU.shape, "pois_bar": MU.shape}
    out.update({k: MU.shape + (B.size,) for k in ("nb_x", "nb_lk", "nb_bar")})
    out.update({f"{k}_{n}": (n_gc,) for n in range(len(SCALES)) for k in ("gc_l", "gc_lk", "gc_bar")})
    return out


def sample(count=200, seed=20261021):
    """a fixed sample of the fixture's entries, (name, index) pairs spread over every array"""
    rs = np.random.RandomState(seed)
    sh = shapes()
    names = sorted(sh)
    return [(nm, tuple(int(rs.randint(0, d)) for d in sh[nm])) for nm in (names[q % len(names)] for q in range(count))]
