"""The models, data, exact solutions, SciPy references and bounds of tests/test_user_inputs.py: linear models driven by
piecewise-linear measured inputs (include/smc_hip.h: smc_set_model_user5, smc_input), whose solution is known exactly, so that
the run-time compiled kernels with the input lookup (csrc/user_input.h) are held to |error| <~ atol + rtol |y| and not only to
"the same numbers as SciPy's solver" - in the manner of tests/linear_chain_model.py.

    python tests/forced_linear_model.py [case ...]     # prints, per case, the worst ratio and K = 2 x that ratio

The models, y' = A(theta) y + B(theta, cond) u(t), out = y:
  F1  RK45, 1 state, 1 input:   y' = -th0 y + th1 u0(t);  theta = (th0, th1, sigma), cond = (y(t0),).  Three experiments: a
      constant profile (one knot), a switch (a ramp 1e-6 wide), a ragged row (three knots, then NaN).
  F2  BDF with smc_user_jac, 2 states, 2 inputs on one knot grid, 2 outputs:  y0' = -k1 y0 + u0,  y1' = k1 y0 - k2 y1 + g u1;
      theta = (k1, k2, g, sigma) with k2 / k1 in the thousands (RK45 would sit on its stability limit: h k2 <= 3.3), cond =
      (y0(t0), y1(t0)).  Output 1 has NaN gaps.
  F3  BDF with the numerical Jacobian, the same equations with g = cond[2] (n_cond = 3), 8 inputs of which the model reads the
      FIRST and the LAST (u0 and u7: a layout that assumes k small or n_cond <= 1 reads the wrong numbers), a noise model with a
      proportional part; theta = (k1, k2, a0, a1, b).

The exact solution: between two breakpoints (knots and output times) u is linear, so z = [y, u, du/dt] obeys z' = M z with M =
[[A, B, 0], [0, 0, I], [0, 0, 0]] and z(t + tau) = expm(M tau) z(t) (scipy.linalg.expm), one segment at a time, u and du/dt set
afresh from the table at every segment's start.  For F1 the closed form of a segment,
(y_j - a/k + b/k^2) e^(-k tau) + (a + b tau)/k - b/k^2 with a = th1 u(t_j), b = th1 du/dt, is the cross-check.

The bound.  K[case] = 2 x the worst |y_scipy - y_exact| / (atol + rtol |y_exact|) over the case's population, SciPy's solve_ivp
running the same method on f with np.interp inside (what a SciPy user writes): measured on the CPU from the reference alone,
before the first device run - the rule of linear_chain_model.K."""
import functools
import multiprocessing
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

N_T = 13
LOOSE, TIGHT = (1e-3, 1e-6), (1e-6, 1e-9)      # (rtol, atol)
_P, _F = (lambda j: ("param", j)), (lambda v: ("fixed", v))
_SIG = "const double *theta, const double *cond"

F1_SOURCE = f"""
__device__ void smc_user_y0({_SIG}, double *y) {{ y[0] = cond[0]; }}
__device__ void smc_user_rhs(double t, const double *y, {_SIG}, double *dydt) {{
    dydt[0] = -theta[0] * y[0] + theta[1] * smc_input(cond, 0, t);
}}
__device__ double smc_user_obs(double t, const double *y, {_SIG}) {{ return y[0]; }}
"""


def _two_state(gain, last, jac):
    s = f"""
__device__ void smc_user_y0({_SIG}, double *y) {{ y[0] = cond[0]; y[1] = cond[1]; }}
__device__ void smc_user_rhs(double t, const double *y, {_SIG}, double *dydt) {{
    dydt[0] = -theta[0] * y[0] + smc_input(cond, 0, t);
    dydt[1] = theta[0] * y[0] - theta[1] * y[1] + {gain} * smc_input(cond, {last}, t);
}}
__device__ void smc_user_obs_vec(double t, const double *y, {_SIG}, double *out) {{ out[0] = y[0]; out[1] = y[1]; }}
"""
    if jac:
        s += f"""__device__ void smc_user_jac(double t, const double *y, {_SIG}, double *J) {{
    J[0] = -theta[0]; J[1] = 0.0;
    J[2] = theta[0];  J[3] = -theta[1];
}}
"""
    return s


F2_SOURCE = _two_state("theta[2]", 1, True)
F3_SOURCE = _two_state("cond[2]", 7, False)

CASES = {
    "F1": {"method": "RK45", "ns": 1, "n_obs": 1, "n_in": 1, "n_cond": 1, "dim": 3, "n": 65, "n_ex": 3, "n_knot": 5, "tol": LOOSE,
           "source": F1_SOURCE, "noise": None, "jac": False},
    "F2": {"method": "BDF", "ns": 2, "n_obs": 2, "n_in": 2, "n_cond": 2, "dim": 4, "n": 63, "n_ex": 2, "n_knot": 9, "tol": LOOSE,
           "source": F2_SOURCE, "noise": None, "jac": True},
    "F3": {"method": "BDF", "ns": 2, "n_obs": 2, "n_in": 8, "n_cond": 3, "dim": 5, "n": 64, "n_ex": 3, "n_knot": 33, "tol": TIGHT,
           "source": F3_SOURCE, "noise": {"additive": [_P(2), _P(3)], "proportional": [_P(4), _F(0.0)]}, "jac": False},
}
THETA_TRUE = {"F1": (0.8, 1.2, 0.05), "F2": (0.9, 2000.0, 1.3, 0.05), "F3": (0.9, 120.0, 0.05, 0.04, 0.08)}

# `python tests/forced_linear_model.py` (SciPy 1.15.3): K = 2 x the worst ratio, fixed before the first device run
K = {"F1": 45.763, "F2": 17.029, "F3": 10.407}


def matrices(cid, th, cond_e):
    """(A (ns, ns), B (ns, n_in)) of y' = A y + B u."""
    c = CASES[cid]
    if cid == "F1":
        return np.array([[-th[0]]]), np.array([[th[1]]])
    A = np.array([[-th[0], 0.0], [th[0], -th[1]]])
    B = np.zeros((2, c["n_in"]))
    B[0, 0] = 1.0
    B[1, c["n_in"] - 1] = th[2] if cid == "F2" else cond_e[2]
    return A, B


def y_start(cid, cond_e):
    return np.array(cond_e[:CASES[cid]["ns"]], dtype=np.float64)


# ---- data ----------------------------------------------------------------------------------------------------------

def _seed(cid):
    return 300 + list(CASES).index(cid)


@functools.lru_cache(maxsize=None)
def make_inputs(cid):
    """{"t": (n_ex, n_knot), "u": (n_ex, n_knot, n_in)}: NaN past a row's knots (u there is junk on purpose: it is ignored)."""
    c = CASES[cid]
    rs = np.random.RandomState(50 + _seed(cid))
    n_ex, nk, n_in = c["n_ex"], c["n_knot"], c["n_in"]
    tk = np.full((n_ex, nk), np.nan)
    u = rs.uniform(-9.0, 9.0, (n_ex, nk, n_in))          # junk past the knots
    if cid == "F1":
        tk[0, :1], u[0, :1, 0] = [0.0], [1.2]                                                       # a constant
        tk[1], u[1, :, 0] = [0.0, 2.0, 2.0 + 1e-6, 5.0, 8.0], [0.5, 1.1, 1.25, 1.4, 1.0]            # a switch: a 1e-6 ramp
        tk[2, :3], u[2, :3, 0] = [1.0, 4.0, 7.0], [0.0, 1.5, 0.3]                                   # ragged; starts after t0
        return {"t": tk, "u": u}
    for e in range(n_ex):
        m = nk if e != 1 else nk - 2                         # row 1 is ragged
        tk[e, :m] = -0.25 + np.cumsum(rs.uniform(0.2, 2.4, m)) * (9.0 / (1.3 * m))      # starts before t0, ends near 9
        u[e, :m] = rs.uniform(0.0, 2.0, (m, n_in))
    return {"t": tk, "u": u}


@functools.lru_cache(maxsize=None)
def make_data(cid):
    """(t (n_ex, n_t), obs (n_ex, n_t, n_obs), cond (n_ex, n_cond)): rows of 13 times that start at 0 or 0.5, two of row 0 1e-6
    apart; F2: 20 % of output 1 is NaN; F3: row 1 is cut after 7 times."""
    c = CASES[cid]
    rs = np.random.RandomState(_seed(cid))
    n_ex = c["n_ex"]
    t = np.empty((n_ex, N_T))
    for e in range(n_ex):
        t[e] = (0.5 if e % 2 else 0.0) + np.concatenate([[0.0], np.cumsum(rs.uniform(0.3, 1.0, N_T - 1))])
    t[0, 5] = t[0, 4] + 1e-6
    if cid == "F3":
        t[1, 7:] = np.nan
    cond = np.column_stack([rs.uniform(0.5, 2.0, n_ex), rs.uniform(0.0, 0.5, n_ex), rs.uniform(0.5, 1.5, n_ex)])[:, :c["n_cond"]]
    f = exact_outputs(cid, np.array([THETA_TRUE[cid]]), t, cond, make_inputs(cid))[0]
    if c["noise"] is None:
        obs = f + THETA_TRUE[cid][-1] * rs.standard_normal(f.shape)
    else:
        a, b = np.array(THETA_TRUE[cid][2:4]), np.array([THETA_TRUE[cid][4], 0.0])
        obs = f + np.sqrt(a ** 2 + (b * f) ** 2) * rs.standard_normal(f.shape)
    if cid == "F2":
        obs[..., 1][rs.uniform(size=obs.shape[:2]) < 0.2] = np.nan
    return t, obs, cond


@functools.lru_cache(maxsize=None)
def population(cid):
    c = CASES[cid]
    rs = np.random.RandomState(1000 + _seed(cid))
    n = c["n"]
    span = {"F1": [(0.3, 1.5), (0.5, 2.0), (0.02, 0.1)],
            "F2": [(0.5, 1.5), (1000.0, 3000.0), (0.5, 2.0), (0.02, 0.1)],
            "F3": [(0.5, 1.5), (50.0, 200.0), (0.02, 0.1), (0.02, 0.1), (0.02, 0.2)]}[cid]
    return np.column_stack([rs.uniform(lo, hi, n) for lo, hi in span])


def priors(cid):
    high = {"F1": (3.0, 4.0, 1.0), "F2": (3.0, 5000.0, 4.0, 1.0), "F3": (3.0, 400.0, 1.0, 1.0, 1.0)}[cid]
    return {f"p{j}": {"dist": "uniform", "low": 0, "high": h} for j, h in enumerate(high)}


def model_kwargs(cid):
    """The keyword arguments of HipEngine.set_model_user after (source, n_states, t, obs)."""
    c = CASES[cid]
    kw = {"cond": make_data(cid)[2], "rtol": c["tol"][0], "atol": c["tol"][1], "method": c["method"], "inputs": make_inputs(cid)}
    if c["noise"] is not None:
        kw["noise"] = c["noise"]
    return kw


# ---- references ----------------------------------------------------------------------------------------------------

def _row(inputs, e):
    """(tk (m,), u (m, n_in)) of experiment e: its finite knots."""
    tk = np.asarray(inputs["t"], dtype=np.float64)[e]
    u = np.asarray(inputs["u"], dtype=np.float64)
    u = u.reshape(u.shape[0], u.shape[1], -1)[e]
    m = int(np.sum(~np.isnan(tk)))
    return tk[:m], u[:m]


def interp_all(tk, u, t):
    """np.interp for every input: (n_in,)."""
    return np.array([np.interp(t, tk, u[:, k]) for k in range(u.shape[1])])


def exact_row(A, B, y0, tk, u, t_out):
    """y at t_out (len, ns) of y' = A y + B u(t), y(t_out[0]) = y0, u linear between the knots tk: expm of the augmented system,
    one segment between breakpoints (knots, output times) at a time."""
    from scipy.linalg import expm
    ns, n_in = B.shape
    M = np.zeros((ns + 2 * n_in, ns + 2 * n_in))
    M[:ns, :ns], M[:ns, ns:ns + n_in] = A, B
    M[ns:ns + n_in, ns + n_in:] = np.eye(n_in)
    out = np.empty((t_out.size, ns))
    y, now = np.array(y0, dtype=np.float64), t_out[0]
    out[0] = y
    for i in range(1, t_out.size):
        stops = np.concatenate([tk[(tk > now) & (tk < t_out[i])], [t_out[i]]])
        for nxt in stops:
            inside = (now >= tk[0]) and (now < tk[-1])
            j = np.searchsorted(tk, now, side="right") - 1
            slope = (u[j + 1] - u[j]) / (tk[j + 1] - tk[j]) if inside else np.zeros(n_in)
            z = np.concatenate([y, interp_all(tk, u, now), slope])
            y = (expm(M * (nxt - now)) @ z)[:ns]
            now = nxt
        out[i] = y
    return out


def f1_closed_row(th, y0, tk, u, t_out):
    """F1's closed form, segment by segment."""
    k = th[0]
    out = np.empty(t_out.size)
    y, now = float(y0), t_out[0]
    out[0] = y
    for i in range(1, t_out.size):
        for nxt in np.concatenate([tk[(tk > now) & (tk < t_out[i])], [t_out[i]]]):
            inside = (now >= tk[0]) and (now < tk[-1])
            j = np.searchsorted(tk, now, side="right") - 1
            a = th[1] * np.interp(now, tk, u[:, 0])
            b = th[1] * ((u[j + 1, 0] - u[j, 0]) / (tk[j + 1] - tk[j])) if inside else 0.0
            tau = nxt - now
            y = (y - a / k + b / k ** 2) * np.exp(-k * tau) + (a + b * tau) / k - b / k ** 2
            now = nxt
        out[i] = y
    return out


def exact_outputs(cid, th, t, cond, inputs):
    """(n, n_ex, n_t, n_obs) exact outputs (= states) for parameters th (n, dim) on a design, NaN past a row's end."""
    c = CASES[cid]
    y = np.full((th.shape[0], t.shape[0], t.shape[1], c["ns"]), np.nan)
    for e in range(t.shape[0]):
        ok = ~np.isnan(t[e])
        tk, u = _row(inputs, e)
        for p in range(th.shape[0]):
            A, B = matrices(cid, th[p], cond[e])
            y[p, e, ok] = exact_row(A, B, y_start(cid, cond[e]), tk, u, t[e, ok])
    return y


def scipy_solve(cid, th, cond_e, tk, u, t_eval, lookup=None):
    """solve_ivp(method, t_eval) with np.interp inside f: states (len, ns) and, for BDF (driven step by step as solve_ivp does with
    t_eval), (accepted steps, LU factorisations, Jacobian evaluations).  lookup(tk, u_k, t): another rounding of the same input."""
    c = CASES[cid]
    A, B = matrices(cid, th, cond_e)
    y0 = y_start(cid, cond_e)
    if t_eval.size == 1:
        return y0[None, :].copy(), (0, 0, 0)
    used = [k for k in range(c["n_in"]) if np.any(B[:, k] != 0.0)]
    look = lookup or np.interp

    def f(t, y):
        d = A @ y
        for k in used:
            d = d + B[:, k] * look(t, tk, u[:, k])
        return d
    rtol, atol = c["tol"]
    if c["method"] == "RK45":
        from scipy.integrate import solve_ivp
        sol = solve_ivp(f, [t_eval[0], t_eval[-1]], y0, method="RK45", t_eval=t_eval, rtol=rtol, atol=atol)
        assert sol.status == 0
        return sol.y.T.copy(), (0, 0, 0)
    from scipy.integrate import BDF
    s = BDF(f, t_eval[0], y0, t_eval[-1], rtol=rtol, atol=atol, jac=(lambda t, y: A) if c["jac"] else None)
    out, i, steps = [], 0, 0
    while s.status == "running":
        s.step()
        assert s.status != "failed"
        steps += 1
        j = np.searchsorted(t_eval, s.t, side="right")
        if j > i:
            out.append(s.dense_output()(t_eval[i:j]).T)
            i = j
    return np.concatenate(out), (steps, s.nlu, s.njev)


def _scipy_particle(args):
    cid, p = args
    c = CASES[cid]
    t, _, cond = make_data(cid)
    th = population(cid)[p]
    y = np.full((c["n_ex"], N_T, c["ns"]), np.nan)
    counts = np.zeros((c["n_ex"], 3), dtype=np.int64)
    for e in range(c["n_ex"]):
        ok = ~np.isnan(t[e])
        tk, u = _row(make_inputs(cid), e)
        y[e, ok], counts[e] = scipy_solve(cid, th, cond[e], tk, u, t[e, ok])
    return y, counts


def _workers():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Computed once per process: {"exact": (n, n_ex, n_t, ns), "scipy": the same from solve_ivp, "counts": (n, n_ex, 3) steps / LU /
    Jacobians, "ratio": worst |scipy - exact| / (atol + rtol |exact|)}."""
    c = CASES[cid]
    t, _, cond = make_data(cid)
    exact = exact_outputs(cid, population(cid), t, cond, make_inputs(cid))
    jobs = [(cid, p) for p in range(c["n"])]
    if _workers() > 1:
        with ProcessPoolExecutor(max_workers=_workers(), mp_context=multiprocessing.get_context("spawn")) as ex:
            rows = list(ex.map(_scipy_particle, jobs, chunksize=4))
    else:
        rows = [_scipy_particle(j) for j in jobs]
    y = np.array([r[0] for r in rows])
    counts = np.array([r[1] for r in rows])
    assert np.array_equal(np.isnan(y), np.isnan(exact))
    rtol, atol = c["tol"]
    return {"exact": exact, "scipy": y, "counts": counts, "ratio": float(np.nanmax(np.abs(y - exact) / (atol + rtol * np.abs(exact))))}


# ---- the lookup alone: planted rows ----------------------------------------------------------------------------------

PLANTED_M = (1, 2, 3, 5, 8, 9, 33, 256)
ULP_UP, ULP_DOWN = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))


@functools.lru_cache(maxsize=None)
def planted_rows(n_in, n_knot=256, ms=PLANTED_M):
    """{"t": (len(ms), n_knot), "u": (len(ms), n_knot, n_in)}: row r has ms[r] knots, a pair of knots 1e-6 apart (from three knots on),
    and values with +0 and -0, equal neighbours, and scales 1e300 apart (1e150 next to 1e-150, both signs)."""
    rs = np.random.RandomState(7 + n_in + n_knot)
    tk = np.full((len(ms), n_knot), np.nan)
    u = rs.uniform(-3.0, 3.0, (len(ms), n_knot, n_in))
    for r, m in enumerate(ms):
        k = 0.75 + np.cumsum(rs.uniform(0.05, 1.0, m))
        if m >= 3:
            k[2:] += (k[1] + 1e-6) - k[2]
        tk[r, :m] = k
        special = [0.0, -0.0, 1e150, 1e-150, -1e150, -1e-150, 2.5, 2.5]
        for i in range(m):
            if (i + r) % 3 == 0:
                u[r, i] = special[(i // 3 + r) % len(special)] * (1.0 if n_in == 1 else np.where(np.arange(n_in) % 2, -1.0, 1.0))
        if m >= 2:
            u[r, m - 1] = u[r, m - 2]                     # equal neighbours at the end
    return {"t": tk, "u": u}


def planted_times(tk_row, most=32):
    """Output times for one row: before the first knot; for up to `most` knots (the first and last ones and a spread of the
    others) one ulp below, on, and one ulp above; after the last knot.  Strictly increasing."""
    m = int(np.sum(~np.isnan(tk_row)))
    tk = tk_row[:m]
    pick = np.arange(m) if m <= most else np.unique(np.concatenate([np.arange(4), np.arange(m - 4, m), np.linspace(4, m - 5, most - 8).astype(int)]))
    tt = [tk[0] - 0.5]
    for j in pick:
        tt += [ULP_DOWN(tk[j]), tk[j], ULP_UP(tk[j])]
    tt.append(tk[-1] + 0.5)
    tt = np.array(tt)
    assert np.all(np.diff(tt) > 0)
    return tt


def lookup_bound(tk, u, t):
    """The derived bound between two roundings of the same lookup: 8 * 2^-53 * max(|u[j]|, |u[j+1]|) at every t."""
    m = tk.size
    j = np.clip(np.searchsorted(tk, t, side="right") - 1, 0, m - 1)
    return 8.0 * 2.0 ** -53 * np.maximum(np.abs(u[j]), np.abs(u[np.minimum(j + 1, m - 1)]))


def bracket(tk, u, t):
    m = tk.size
    j = np.clip(np.searchsorted(tk, t, side="right") - 1, 0, m - 1)
    j1 = np.minimum(j + 1, m - 1)
    return np.minimum(u[j], u[j1]), np.maximum(u[j], u[j1])


LOOKUP_SOURCE = f"""
__device__ void smc_user_y0({_SIG}, double *y) {{ y[0] = 1.0; }}
__device__ void smc_user_rhs(double t, const double *y, {_SIG}, double *dydt) {{ dydt[0] = 0.0; }}
__device__ void smc_user_obs_vec(double t, const double *y, {_SIG}, double *out) {{
    for (int k = 0; k < N_IN; ++k) out[k] = smc_input(cond, k, t);
}}
"""


def lookup_source(n_in):
    return LOOKUP_SOURCE.replace("N_IN", str(n_in))


def main():
    ids = sys.argv[1:] or list(CASES)
    print(f"{'case':4s} {'worst ratio':>12s} {'K':>9s}   steps / LU / Jacobians")
    for cid in ids:
        r = reference(cid)
        print(f"{cid:4s} {r['ratio']:12.4f} {2 * r['ratio']:9.3f}   {tuple(int(v) for v in r['counts'].sum(axis=(0, 1)))}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
