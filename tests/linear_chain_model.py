"""The model family, data, exact solutions and bounds of tests/test_user_model_matrix.py: a linear chain of 1 .. 8 states with
1 .. 8 outputs whose solution is known exactly, so that the run-time compiled user kernels (csrc/user_rk45_kernel.h,
user_bdf_kernel.h, user_obs_args.h) are held to the promise |error| <~ atol + rtol |y| at every state and output count and
not only to "the same numbers as SciPy's solver".

    python tests/linear_chain_model.py [case ...]     # prints, per case, the worst ratio, K = 2 x that ratio, the swap counts

The model.  theta[0] = kf, theta[1] = kb; cond = (A0, spread, gain).  y0 = (A0, 0, ...).  Link i (0 .. ns - 2) carries the flux
kf c_i y_i - kb c_i y_(i+1) with c_i = exp2(spread i); the last state drains with kb (ns = 1: y' = -kb y).  gain != 1 makes
link 0 irreversible (no back flux into y_0, none taken out of y_1) and multiplies what it delivers into y_1 by gain: the
matrix is then block triangular, -kf c_0 over a reversible chain with a drain, so its eigenvalues stay real and negative, and
I - c J has the entry -c gain kf c_0 under a diagonal of order 1, so partial pivoting swaps rows 0 and 1 (SciPy does in every
solve).  What that exercises is the exchange itself - the selects that swap the rows of lu_factor and the entries of lu_solve's
right-hand side, which must agree with each other.  It does NOT show that pivoting is needed: row 0 of I - c J is
(1 + c kf c_0, 0, ..., 0), elimination without a swap causes no fill and no growth, and an LU that never pivots, consistently in
factorisation and solve, follows SciPy to 1e-14 - the matrix cannot tell it from the real one.
Outputs: out[k] = sum_j w_kj y_j with w_kj = 1 + (3 k + 5 j) % 7.

The exact solution y(t) = expm(A (t - t0)) y0 is formed twice: by scipy.linalg.expm, and by the eigen-decomposition of the
symmetrised reversible chain (with the decaying y_0 as a forcing term when gain != 1).

The bound.  K[case] = 2 x the worst |y_scipy - y_exact| / (atol + rtol |y_exact|) over the case's own population, data and
tolerances, SciPy's solve_ivp running the same method with the same t_eval, rtol, atol and (where the case has smc_user_jac)
the matrix as its Jacobian: measured on the CPU from the reference alone, before the first device run, and doubled as in
tests/robertson_bdf_bound.py.  SWAPS[case] = (solves with at least one row swap, solves, factorisations with a swap,
factorisations) of SciPy's BDF on the same population: with gain = 1e4 every solve swaps, with gain = 1 none does.

The output times.  An RK45 case must stay limited by accuracy, not by stability, or SciPy is no reference to 1e-9: past
RK45's stability limit, h |lambda|_max = 3.3, every step multiplies the rounding noise of the fastest mode, and two roundings
of the same right-hand side end 1e-8 apart.  The eight-state chain at rtol = 1e-6 gets there on rows of 13 times 0.3 .. 1.2
apart, so R7's times are half as far apart (t_scale = 0.5).  reference(cid)["rounding"] measures it - SciPy's solves of the
flux-by-flux and of the A y right-hand side against each other - and tests/test_user_model_matrix.py holds it under 1e-11
for every RK45 case."""
import functools
import multiprocessing
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

A0 = np.array([1.0, 2.0, 0.5, 1.5, 0.8])
K_TRUE = (0.8, 0.4)
N_T = 13
SPREAD = {"RK45": 0.25, "BDF": 2.0}         # BDF: rates 4^i apart, 4096 at eight states
LOOSE, TIGHT = (1e-3, 1e-6), (1e-6, 1e-9)   # (rtol, atol)

# noise specifications (user_models.noise_layout); parameters 0 and 1 are kf and kb
_P, _F = (lambda j: ("param", j)), (lambda v: ("fixed", v))
NOISE_8A = {"additive": [_P(2), _P(3), _P(4), _P(2), _F(0.05), _P(3), _F(0.08), _P(7)],          # parameter 7: an additive level
            "proportional": [_P(5), _P(6), _F(0.0), _P(5), _P(6), _F(0.1), _P(5), _P(6)]}
# ... a proportional coefficient; the last output alone reads parameters 4 and 7 (a validity check must reach it)
NOISE_8B = {"additive": [_P(2), _P(3), _P(2), _P(2), _P(3), _P(3), _F(0.06), _P(4)],
            "proportional": [_P(5), _P(6), _P(5), _F(0.0), _P(5), _P(6), _F(0.05), _P(7)]}
NOISE_2 = {"additive": [_P(2), _P(7)], "proportional": [_P(5), _P(3)]}
NOISE_4_ADD = {"additive": [_P(2), _P(5), _F(0.05), _P(7)]}
NOISE_3 = {"additive": [_P(2), _F(0.05), _P(3)], "proportional": [_P(4), _F(0.0), _P(4)]}
NOISE_2_ADD = {"additive": [_P(2), _P(3)]}
NOISE_6 = {"additive": [_P(2), _P(3), _P(4), _F(0.04), _P(2), _P(7)], "proportional": [_P(5), _P(6), _F(0.0), _P(5), _P(6), _P(5)]}


def _case(method, ns, n_obs, dim, n, n_ex, tol=LOOSE, gain=1.0, jac=0, noise=None, scalar=False, obs2d=False, scale=None,
          sigma_fixed=None, t_scale=1.0):
    return {"method": method, "ns": ns, "n_obs": n_obs, "dim": dim, "n": n, "n_ex": n_ex, "rtol": tol[0], "atol": tol[1],
            "gain": gain, "jac": jac, "noise": noise, "scalar": scalar, "obs2d": obs2d, "scale": scale, "sigma_fixed": sigma_fixed,
            "t_scale": t_scale}


# the covering set: every n_states and n_obs in 1 .. 8 under each method; n and n_ex on the edges of the scheduler's hand-out (a
# chunk is 64 particles x 2 experiments).  scalar: the source defines smc_user_obs only; obs2d: 2-D obs, the
# smc_set_model_user2 path (no NaN, no ragged row there).  Without noise the likelihood has one sigma, the last parameter (or
# sigma_fixed).  t_scale: the spacing of the output times (the module's text).
CASES = {
    "R2": _case("RK45", 3, 8, 8, 65, 3, noise=NOISE_8A),
    "B3": _case("BDF", 4, 8, 8, 130, 1, tol=TIGHT, noise=NOISE_8A),
    "B7": _case("BDF", 8, 8, 8, 65, 2, tol=TIGHT, gain=1e4, jac=1, noise=NOISE_8B),
    "R1": _case("RK45", 1, 1, 3, 65, 2, scalar=True, obs2d=True),
    "R3": _case("RK45", 4, 5, 6, 63, 5, tol=TIGHT, scale=(1.0, 3.0, 0.5, 2.0, 1.5)),
    "R4": _case("RK45", 5, 4, 8, 130, 1, noise=NOISE_4_ADD),
    "R5": _case("RK45", 6, 7, 3, 1, 2, sigma_fixed=0.05),
    "R6": _case("RK45", 7, 2, 8, 257, 3, gain=1e4, noise=NOISE_2),
    "R7": _case("RK45", 8, 8, 8, 64, 2, tol=TIGHT, noise=NOISE_8B, t_scale=0.5),
    "B1": _case("BDF", 1, 1, 3, 65, 2, scalar=True, obs2d=True),
    "B2": _case("BDF", 2, 3, 5, 63, 3, gain=1e4, jac=1, noise=NOISE_3),
    "B4": _case("BDF", 5, 2, 4, 1, 5, gain=1e4, jac=1, noise=NOISE_2_ADD),
    "B5": _case("BDF", 6, 6, 8, 257, 2, jac=1, noise=NOISE_6),
    "B6": _case("BDF", 7, 1, 3, 64, 3, scalar=True),
}
SUMMARY_CASES = ("R2", "B3", "B7")          # first in CASES: eight outputs, a cell count that is no multiple of 32, n odd / not 64 k

# `python tests/linear_chain_model.py` (SciPy 1.15.3): K = 2 x the worst ratio, fixed before the first device run
K = {
    "R2": 3.777, "B3": 16.036, "B7": 76.219, "R1": 5.636, "R3": 2.338, "R4": 4.664, "R5": 2.286, "R6": 23.987, "R7": 1.857,
    "B1": 5.478, "B2": 8.618, "B4": 5.419, "B5": 7.232, "B6": 7.664,
}
# ... and its swap counts: (solves with a swap, solves, factorisations with a swap, factorisations); single-time rows are no solves.
# Informative only - the test recomputes them and asserts that every solve of a gain = 1e4 case (B7, B2, B4) swaps;
# gain = 1: none swaps (I - c J is diagonally dominant), which is recorded and not asserted.
SWAPS = {
    "B3": (0, 130, 0, 4060), "B7": (130, 130, 3801, 4907), "B1": (0, 130, 0, 1070), "B2": (126, 126, 1088, 1592),
    "B4": (4, 4, 53, 71), "B5": (0, 514, 0, 7746), "B6": (0, 128, 0, 1963),
}


def weights(n_obs, ns):
    k, j = np.arange(n_obs)[:, None], np.arange(ns)[None, :]
    return (1 + (3 * k + 5 * j) % 7).astype(np.float64)


def source(ns, n_obs, jac, scalar=False):
    """HIP text of the model: smc_user_y0, smc_user_rhs, smc_user_obs_vec (scalar: smc_user_obs, n_obs = 1) and, with jac,
    smc_user_jac (row-major J[i * ns + j])."""
    assert 1 <= ns <= 8 and 1 <= n_obs <= 8 and (not scalar or n_obs == 1)
    sig = "const double *theta, const double *cond"
    head = ["    const double kf = theta[0], kb = theta[1], sp = cond[1], g = cond[2];", "    const bool one_way = g != 1.0;"]
    head += [f"    const double c{i} = exp2(sp * {i}.0);" for i in range(ns - 1)]
    out = [f"__device__ void smc_user_y0({sig}, double *y) {{ " + " ".join(f"y[{i}] = {'cond[0]' if i == 0 else '0.0'};" for i in range(ns)) + " }"]
    body = list(head)
    for i in range(ns - 1):
        flux = f"kf * c{i} * y[{i}] - kb * c{i} * y[{i + 1}]"
        body.append(f"    const double q{i} = " + (f"one_way ? kf * c0 * y[0] : {flux};" if i == 0 else f"{flux};"))
    for i in range(ns):
        gain_in = "(one_way ? g * q0 : q0)" if i == 1 else f"q{i - 1}"
        loss = f"q{i}" if i < ns - 1 else f"kb * y[{i}]"
        body.append(f"    dydt[{i}] = " + (f"-({loss});" if i == 0 else f"{gain_in} - {loss};"))
    out.append(f"__device__ void smc_user_rhs(double t, const double *y, {sig}, double *dydt) {{\n" + "\n".join(body) + "\n}")
    w = weights(n_obs, ns).astype(int)
    rows = [" + ".join(f"{w[k, j]}.0 * y[{j}]" for j in range(ns)) for k in range(n_obs)]
    if scalar:
        out.append(f"__device__ double smc_user_obs(double t, const double *y, {sig}) {{ return {rows[0]}; }}")
    else:
        out.append(f"__device__ void smc_user_obs_vec(double t, const double *y, {sig}, double *out) {{\n"
                   + "\n".join(f"    out[{k}] = {r};" for k, r in enumerate(rows)) + "\n}")
    if jac:
        e = {}
        for i in range(ns - 1):              # link i: y_i loses, y_(i+1) gains
            first = i == 0
            e.setdefault((i, i), []).append(f"-kf * c{i}")
            e.setdefault((i, i + 1), []).append("(one_way ? 0.0 : kb * c0)" if first else f"kb * c{i}")
            e.setdefault((i + 1, i), []).append("(one_way ? g * kf * c0 : kf * c0)" if first else f"kf * c{i}")
            e.setdefault((i + 1, i + 1), []).append("-(one_way ? 0.0 : kb * c0)" if first else f"-kb * c{i}")
        e.setdefault((ns - 1, ns - 1), []).append("-kb")
        body = list(head) + [f"    J[{i * ns + j}] = " + (" + ".join(e[(i, j)]).replace("+ -", "- ") if (i, j) in e else "0.0") + ";"
                             for i in range(ns) for j in range(ns)]
        out.append(f"__device__ void smc_user_jac(double t, const double *y, {sig}, double *J) {{\n" + "\n".join(body) + "\n}")
    return "\n".join(out) + "\n"


def case_source(cid):
    c = CASES[cid]
    return source(c["ns"], c["n_obs"], c["jac"], c["scalar"])


def matrix(kf, kb, ns, spread, gain):
    """A of y' = A y."""
    A = np.zeros((ns, ns))
    c = np.exp2(spread * np.arange(max(ns - 1, 1)))
    for i in range(ns - 1):
        one_way = i == 0 and gain != 1.0
        A[i, i] -= kf * c[i]
        A[i + 1, i] += (gain if one_way else 1.0) * kf * c[i]
        if not one_way:
            A[i, i + 1] += kb * c[i]
            A[i + 1, i + 1] -= kb * c[i]
    A[ns - 1, ns - 1] -= kb
    return A


def rhs(t, y, kf, kb, spread, gain):
    """The right-hand side as the HIP text forms it, flux by flux (what SciPy integrates)."""
    ns = len(y)
    d = np.empty(ns)
    if ns == 1:
        d[0] = -(kb * y[0])
        return d
    c = np.exp2(spread * np.arange(ns - 1))
    q = kf * c * y[:-1] - kb * c * y[1:]
    q_in = q.copy()
    if gain != 1.0:
        q[0] = kf * c[0] * y[0]
        q_in[0] = gain * q[0]
    d[0] = -q[0]
    d[1:-1] = q_in[:-1] - q[1:]
    d[-1] = q_in[-1] - kb * y[-1]
    return d


def exact_expm(kf, kb, ns, spread, gain, a0, dt):
    """y(t0 + dt) = expm(A dt) y0 for every dt: (len(dt), ns)."""
    from scipy.linalg import expm
    A = matrix(kf, kb, ns, spread, gain)
    y0 = np.zeros(ns)
    y0[0] = a0
    return np.array([expm(A * x) @ y0 for x in dt])


def _sym_eig(A):
    """A tridiagonal with A_(i,i+1) A_(i+1,i) > 0: A = D S D^-1 with S symmetric; returns (lambda, V, d) with S = V diag(lambda) V^T."""
    n = A.shape[0]
    d = np.ones(n)
    for i in range(n - 1):
        d[i + 1] = d[i] * np.sqrt(A[i + 1, i] / A[i, i + 1])
    S = A * d[None, :] / d[:, None]
    lam, V = np.linalg.eigh(0.5 * (S + S.T))
    return lam, V, d


def exact_eig(kf, kb, ns, spread, gain, a0, dt):
    """The same solution from the eigen-decomposition of the symmetrised reversible chain.  gain != 1: y_0 = A0 exp(-mu t) with
    mu = kf c_0 drives the chain z = y[1:], z' = B z + gain mu y_0 e_1; per mode zeta' = lambda zeta + b exp(-mu t), zeta(0) = 0:
    zeta = b exp(lambda t) expm1(x t) / x with x = -(mu + lambda) (t for x = 0)."""
    dt = np.asarray(dt, dtype=np.float64)
    A = matrix(kf, kb, ns, spread, gain)
    if ns == 1:
        return a0 * np.exp(A[0, 0] * dt)[:, None]
    if gain == 1.0:
        lam, V, d = _sym_eig(A)
        z0 = V.T @ (np.eye(ns)[0] * a0 / d)
        return (np.exp(lam[None, :] * dt[:, None]) * z0[None, :]) @ V.T * d[None, :]
    mu = -A[0, 0]
    y = np.empty((dt.size, ns))
    y[:, 0] = a0 * np.exp(-mu * dt)
    B = A[1:, 1:]
    if ns == 2:
        lam, V, d = np.array([B[0, 0]]), np.ones((1, 1)), np.ones(1)
    else:
        lam, V, d = _sym_eig(B)
    b = V.T @ (np.eye(ns - 1)[0] * (A[1, 0] * a0) / d)
    x, tt = -(mu + lam)[None, :], dt[:, None]
    grow = np.exp(lam[None, :] * tt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        near = grow * np.where(x == 0.0, tt, np.expm1(x * tt) / x)       # |x t| < 1: no cancellation
        far = (np.exp(-mu * tt) - grow) / x                              # else the two exponentials are a factor e apart
    y[:, 1:] = (b[None, :] * np.where(np.abs(x * tt) < 1.0, near, far)) @ V.T * d[None, :]
    return y


# ---- data ----------------------------------------------------------------------------------------------------------

def _seed(cid):
    return 100 + list(CASES).index(cid)


@functools.lru_cache(maxsize=None)
def make_data(cid):
    """(t (n_ex, n_t), obs (n_ex, n_t, n_obs) or (n_ex, n_t) for a 2-D case, cond (n_ex, 3)).  Rows of 13 times that start at 0 or
    at 0.5; row 0 holds two times 1e-6 apart (two outputs of one step); and, where NaN is allowed (not obs2d): row 1 is cut after
    7 times, row 2 holds a single time (nothing to integrate: the outputs of y0), 15 % of the observations are NaN."""
    c = CASES[cid]
    rs = np.random.RandomState(_seed(cid))
    n_ex, ns = c["n_ex"], c["ns"]
    t = np.empty((n_ex, N_T))
    for e in range(n_ex):
        t[e] = (0.5 if e % 2 else 0.0) + np.concatenate([[0.0], c["t_scale"] * np.cumsum(rs.uniform(0.3, 1.2, N_T - 1))])
    t[0, 5] = t[0, 4] + 1e-6
    if not c["obs2d"]:
        if n_ex >= 2:
            t[1, 7:] = np.nan
        if n_ex >= 3:
            t[2, 1:] = np.nan
    cond = np.column_stack([A0[:n_ex], np.full(n_ex, SPREAD[c["method"]]), np.full(n_ex, c["gain"])])
    W = weights(c["n_obs"], ns)
    f = np.full((n_ex, N_T, c["n_obs"]), np.nan)
    for e in range(n_ex):
        m = ~np.isnan(t[e])
        f[e, m] = exact_expm(K_TRUE[0], K_TRUE[1], ns, cond[e, 1], cond[e, 2], cond[e, 0], t[e, m] - t[e, 0]) @ W.T
    scale = np.ones(c["n_obs"]) if c["scale"] is None else np.asarray(c["scale"])
    obs = f + np.sqrt((0.03 * scale) ** 2 + (0.05 * f) ** 2) * rs.standard_normal(f.shape)
    if c["obs2d"]:
        return t, obs[..., 0], cond
    obs[rs.uniform(size=obs.shape) < 0.15] = np.nan
    return t, obs, cond


def roles(cid):
    """Per parameter: "k", "add" (an additive level or sigma), "prop" (a proportional coefficient) or "free" (read by nothing)."""
    c = CASES[cid]
    r = ["k", "k"] + ["free"] * (c["dim"] - 2)
    if c["noise"] is None:
        if c["sigma_fixed"] is None:
            r[-1] = "add"
    else:
        for part, role in (("additive", "add"), ("proportional", "prop")):
            for kind, v in c["noise"].get(part, []):
                if kind == "param":
                    r[v] = role
    return r


@functools.lru_cache(maxsize=None)
def population(cid):
    """(n, dim): kf in [0.2, 2], kb in [0.1, 1], noise levels in [0.02, 0.1], proportional coefficients in [0.02, 0.2]."""
    c = CASES[cid]
    rs = np.random.RandomState(1000 + _seed(cid))
    n = c["n"]
    span = {"add": (0.02, 0.1), "prop": (0.02, 0.2), "free": (0.1, 1.0)}
    cols = [rs.uniform(0.2, 2.0, n), rs.uniform(0.1, 1.0, n)] + [rs.uniform(*span[r], n) for r in roles(cid)[2:]]
    return np.column_stack(cols)


def priors(cid):
    high = {"k": 3.0, "add": 1.0, "prop": 1.0, "free": 2.0}
    return {f"p{j}": {"dist": "uniform", "low": 0, "high": high[r]} for j, r in enumerate(roles(cid))}


def model_kwargs(cid):
    """The keyword arguments of HipEngine.set_model_user after (source, n_states, t, obs)."""
    c = CASES[cid]
    kw = {"cond": make_data(cid)[2], "rtol": c["rtol"], "atol": c["atol"], "method": c["method"]}
    if c["noise"] is not None:
        kw["noise"] = c["noise"]
    if c["scale"] is not None:
        kw["obs_scale"] = c["scale"]
    if c["sigma_fixed"] is not None:
        kw.update(est_sigma=False, sigma_fixed=c["sigma_fixed"])
    return kw


# ---- references ----------------------------------------------------------------------------------------------------

def exact_states(cid, how=exact_expm):
    """(n, n_ex, n_t, ns) exact states of the case's population at its data times, NaN past a row's end."""
    c = CASES[cid]
    t, _, cond = make_data(cid)
    th = population(cid)
    y = np.full((c["n"], c["n_ex"], N_T, c["ns"]), np.nan)
    for e in range(c["n_ex"]):
        m = ~np.isnan(t[e])
        for p in range(c["n"]):
            y[p, e, m] = how(th[p, 0], th[p, 1], c["ns"], cond[e, 1], cond[e, 2], cond[e, 0], t[e, m] - t[e, 0])
    return y


def scipy_solve(method, ns, kf, kb, spread, gain, a0, t_eval, rtol, atol, with_jac, matrix_rhs=False):
    """solve_ivp(method, t_eval) on the model: states (len(t_eval), ns) and, for BDF (driven step by step, as solve_ivp does with
    t_eval), (accepted steps, LU factorisations, Jacobian evaluations, factorisations that swapped a row).  matrix_rhs: the
    right-hand side as A y instead of flux by flux - the same function rounded another way."""
    y0 = np.zeros(ns)
    y0[0] = a0
    if t_eval.size == 1:                      # base.py: nothing to integrate
        return y0[None, :].copy(), (0, 0, 0, 0)
    f = lambda t, y: rhs(t, y, kf, kb, spread, gain)
    if matrix_rhs:
        A_rhs = matrix(kf, kb, ns, spread, gain)
        f = lambda t, y: A_rhs @ y
    if method == "RK45":
        from scipy.integrate import solve_ivp
        sol = solve_ivp(f, [t_eval[0], t_eval[-1]], y0, method="RK45", t_eval=t_eval, rtol=rtol, atol=atol)
        assert sol.status == 0
        return sol.y.T.copy(), (0, 0, 0, 0)
    from scipy.integrate import BDF
    A = matrix(kf, kb, ns, spread, gain)
    s = BDF(f, t_eval[0], y0, t_eval[-1], rtol=rtol, atol=atol, jac=(lambda t, y: A) if with_jac else None)
    swapped = [0]
    plain_lu = s.lu

    def counting_lu(M):
        r = plain_lu(M)
        swapped[0] += int(np.any(r[1] != np.arange(ns)))
        return r
    s.lu = counting_lu
    out, i, steps = [], 0, 0
    while s.status == "running":
        s.step()
        assert s.status != "failed"
        steps += 1
        j = np.searchsorted(t_eval, s.t, side="right")      # ivp.py: the t_eval values up to and including t
        if j > i:
            out.append(s.dense_output()(t_eval[i:j]).T)
            i = j
    return np.concatenate(out), (steps, s.nlu, s.njev, swapped[0])


def _scipy_particle(args):
    cid, p = args
    c = CASES[cid]
    t, _, cond = make_data(cid)
    th = population(cid)[p]
    y = np.full((c["n_ex"], N_T, c["ns"]), np.nan)
    y_alt = y.copy()
    counts = np.zeros((c["n_ex"], 4), dtype=np.int64)
    for e in range(c["n_ex"]):
        m = ~np.isnan(t[e])
        args = (c["method"], c["ns"], th[0], th[1], cond[e, 1], cond[e, 2], cond[e, 0], t[e, m], c["rtol"], c["atol"],
                bool(c["jac"]))
        y[e, m], counts[e] = scipy_solve(*args)
        if c["method"] == "RK45":
            y_alt[e, m] = scipy_solve(*args, matrix_rhs=True)[0]
    return y, counts, y_alt


def _workers():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Everything the tests compare with, computed once per process: {"exact": (n, n_ex, n_t, ns), "scipy": the same from
    solve_ivp, "counts": (n, n_ex, 4) steps / LU / Jacobians / swapping LUs, "ratio": worst |scipy - exact| / (atol + rtol |exact|),
    RK45 only: "rounding": worst |W y - W y'| / max(1, |W y|) between SciPy's solves of the flux-by-flux and the A y
    right-hand side}."""
    c = CASES[cid]
    exact = exact_states(cid)
    jobs = [(cid, p) for p in range(c["n"])]
    if c["n"] >= 8 and _workers() > 1:
        with ProcessPoolExecutor(max_workers=_workers(), mp_context=multiprocessing.get_context("spawn")) as ex:
            rows = list(ex.map(_scipy_particle, jobs, chunksize=4))
    else:
        rows = [_scipy_particle(j) for j in jobs]
    y = np.array([r[0] for r in rows])
    counts = np.array([r[1] for r in rows])
    assert np.array_equal(np.isnan(y), np.isnan(exact))
    ratio = float(np.nanmax(np.abs(y - exact) / (c["atol"] + c["rtol"] * np.abs(exact))))
    out = {"exact": exact, "scipy": y, "counts": counts, "ratio": ratio}
    if c["method"] == "RK45":
        W = weights(c["n_obs"], c["ns"])
        a, b = y @ W.T, np.array([r[2] for r in rows]) @ W.T
        out["rounding"] = float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(a))))
    return out


def swap_counts(cid):
    """(solves with at least one swapping factorisation, solves, swapping factorisations, factorisations); a single-time row is no solve."""
    cn = reference(cid)["counts"]
    solved = cn[..., 0] > 0
    return int(np.sum(cn[..., 3][solved] > 0)), int(solved.sum()), int(cn[..., 3].sum()), int(cn[..., 1].sum())


def main():
    ids = sys.argv[1:] or list(CASES)
    print(f"{'case':4s} {'worst ratio':>12s} {'K':>9s}   swaps (solves, of, LUs, of)   steps / LU / Jacobians   RK45: rounding")
    for cid in ids:
        r = reference(cid)
        tot = r["counts"].sum(axis=(0, 1))
        sw = swap_counts(cid) if CASES[cid]["method"] == "BDF" else None
        print(f"{cid:4s} {r['ratio']:12.4f} {2 * r['ratio']:9.3f}   {sw}   {tuple(int(v) for v in tot[:3])}   {r.get('rounding', '')}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
