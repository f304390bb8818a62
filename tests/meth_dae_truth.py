"""The method-independent reference solution of the methanation DAE behind tests/test_meth_dae_truth.py, its fixture
(tests/golden/meth_dae_truth.npz, written by tests/golden/make_meth_dae_truth.py) and the bounds K8 and the CPU checker are held to.

    python tests/meth_dae_truth.py        # prints the measurements below, from which the committed K follows

The reference owes nothing to the project's BDF code (oracle/meth_dae_oracle.c, csrc/meth_dae*.h).  It is built on the residual
reaction(X, X', p) alone - the one function of the DAE that is pinned to the reference's own values (tests/golden/methanation_golden.npz)
- with NumPy and scipy.linalg:
  * backward Euler, F(X1, (X1 - X0) / h, p) = 0, on a graded grid: 0, 1e-6, then geometric segments 1e-6 -> 0.5 -> 5 -> 75 that share
    N0 - 1 = 799 steps by their decades; every further grid bisects each step of the one before, LEVELS = 5 grids (799 .. 12784 steps);
  * X(0) = guess[i].  The algebraic variables (u everywhere, the outlet node) enter F through X1 only, so the first step projects
    them; the differential start values are what defines the problem;
  * Newton with a finite-difference matrix of the step equation from one batch call of 357 rows, kept while the step size stays within
    15 % and the iteration needs at most 10 sweeps, iterated until the update is below 1e-9 units (where the rounding of the residual
    stops the contraction between 1e-9 and 1e-8 units the step is accepted: the worst accepted update is 2.7e-9 units, stored);
  * the full Richardson table, column k = (2^k T[j+1] - T[j]) / (2^k - 1), evaluated as T[j+1] + (T[j+1] - T[j]) / (2^k - 1); the
    stored state is the last column's one entry, its error bar the distance to the last entry of the column before.  The double-precision residual does not limit the table (below), so there
    is no extended-precision restatement.
Units: |a - b| / (1e-6 + 1e-6 |b|), the maximum over all 357 states, whatever the tolerance of the run measured.

The 12 runs: experiments 0, 7, 19, 29 x (BASEPARAMS; BASEPARAMS * (3, 1, 0.3, 1, 1, 1, 1, 1); the first interior prior-box vector of
test_dae_batch_vs_oracle, RandomState(3)), each sampled at t = 0.5, 5 and 75 from one run: 36 samples.  No case had to be replaced.

Measured on the CPU (SciPy 1.15.3, NumPy 2.2.6; `python tests/golden/make_meth_dae_truth.py` takes about 35 s on 8 cores, this
module's main a few seconds), before any device run:

  error bar, worst of the 12 runs            t = 0.5: 9.7e-6    t = 5: 2.3e-3    t = 75: 2.8e-4      (required: <= 0.05)
  run 0 at t = 0.5, successive differences   column 0: 29.2 / 14.6 / 7.32 / 3.66   column 1: 0.394 / 0.101 / 0.0255
                                             column 2: 3.1e-3 / 4.0e-4             column 3: 2.4e-5     (ratios 2, 4, 8: an expansion in h)

  worst distance to the fixture, 12 runs                 tol = 1e-6    1e-7      1e-8      most attempts at 1e-8
  dae_solve_policy(k8_policy())  (= K8)     t = 0.5      3.4383        0.4835    0.0566    264
                                            t = 5        9.2529        0.4831    0.1073    431
                                            t = 75       2.2445        0.2751    0.0219    1666   (K8's budget: 3000; required <= 2000)
  dae_solve (the checker's default policy)  t = 0.5      2.0284        0.2578    0.0315
                                            t = 5        3.0025        0.2474    0.0432
                                            t = 75       0.8866        0.1126    0.0196
  dae_solve_ida (tf = the sample time)      t = 0.5      2.0063        0.3191    0.0193
                                            t = 5        6.6707        0.6529    0.0655
                                            t = 75       1.2297        0.1071    0.0176
All three converge to the independent solution as the tolerance falls.  Per run, dae_solve's distance at 1e-8 is 0.004 .. 0.15 of its distance at 1e-6; the one run above 0.1 (experiment 7, second vector, t = 75: 0.0062 against 0.0425) is a 1e-6 run
that happens to lie 20 times closer than its neighbours, which is why the convergence test takes the worst of the runs on both sides.

The bounds (the rule of dosed_model.K): K = 2 x the worst distance of the CPU statement + the fixture's error bar, in the fixed
1e-6 units, so that K falls with the tolerance.  The factor 2 is for what separates the kernel from its CPU statement (analytic matrix
and block LU against finite differences and a banded LU: Newton iterates differ below the Newton test; test_dae_batch_vs_oracle
observes < 1e-3 units at the base parameters).  K is never fitted to a device result.

Planted errors at tol = 1e-6 (least distance of the 12 runs; the policy run and dae_solve agree to the digits shown):
  activation energy (p0[11]) x (1 + 1e-4)    t = 0.5: 133     t = 5: 890     t = 75: 783       against K_POLICY = 6.88 / 18.5 / 4.49
  rate constant     (p0[10]) x (1 + 1e-4)    t = 0.5: 6.9     t = 5: 53      t = 75: 83
  tf x (1 + 1e-3)                            t = 0.5: 46      t = 5: 795     t = 75: 0.02
What the bar cannot see: at t = 0.5 and tol = 1e-6 a 1e-4 error of the rate constant moves the runs of the third vector by 7 .. 10
units, which is K there (6.88) - visible from tol = 1e-7 on (K = 0.97); at t = 75 the reactor has all but settled (0.075 s more
move it by 0.02 .. 2 units), so a wrong final time is invisible there: that is what the transient samples are for.

Measured on the device (MI355X, 2026-10-21, `python -m pytest tests/test_meth_dae_truth.py -m gpu -s`; K8, the two-wave kernel, worst of
the 12 solves over all 357 states, and its share of K):
                                                         tol = 1e-6       1e-7             1e-8
  K8                                        t = 0.5      3.7666 (0.55)    0.4978 (0.52)    0.0747 (0.66)
                                            t = 5        3.9696 (0.21)    0.6470 (0.67)    0.0860 (0.40)
                                            t = 75       0.9655 (0.22)    0.3810 (0.69)    0.0319 (0.72)
  status 0 for all 108 solves; the flows equal the NumPy mapping of the kernel's own outlet state bit for bit, and lie within 0.07 of
  the propagated bound of the mapping of the fixture's outlet state.  K8 and its CPU statement do not take the same steps to the digit:
  their distances differ by up to several units at 1e-6, inside the factor 2.
"""
import multiprocessing
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
FIXTURE = os.path.join(GOLD, "meth_dae_truth.npz")

NX, NS = 51, 357
TIMES = (0.5, 5.0, 75.0)
TOLS = (1e-6, 1e-7, 1e-8)
EXPERIMENTS = (0, 7, 19, 29)
N0, LEVELS = 800, 5                      # steps of the coarsest grid (nominal), nested levels
T_FIRST = 1e-6
NEWTON_UNITS = 1e-9
OUTLET = np.array([50, 101, 152, 203, 254, 305, 356])
INLET_DIFF = np.array([0, 51, 102, 153, 204, 255])          # the inlet node's six differential values: X' = 0
LINEAR_ROWS = np.array([306, 50, 101, 152, 203, 254, 305, 356])   # u[0] - u_in and the seven outlet conditions
BAR_MAX = 0.05

# `python tests/meth_dae_truth.py`: 2 x worst + bar of the table above, fixed before the first device run.  [tf][tol]
K_POLICY = {0.5: {1e-6: 6.8765, 1e-7: 0.9670, 1e-8: 0.1133},
            5.0: {1e-6: 18.5081, 1e-7: 0.9684, 1e-8: 0.2169},
            75.0: {1e-6: 4.4893, 1e-7: 0.5504, 1e-8: 0.0442}}
K = K_POLICY                                                   # what K8 is held to
K_DEFAULT = {0.5: {1e-6: 4.0567}, 5.0: {1e-6: 6.0074}, 75.0: {1e-6: 1.7734}}      # dae_solve
K_IDA = {0.5: {1e-6: 4.0126}, 5.0: {1e-6: 13.3436}, 75.0: {1e-6: 2.4597}}         # dae_solve_ida
MAX_ATTEMPTS_CPU = 2000                                        # of K8's fixed budget of 3000, for the policy run at 1e-8


def units(a, b):
    """|a - b| in the fixed yardstick 1e-6 + 1e-6 |b|, per state."""
    return np.abs(a - b) / (1e-6 + 1e-6 * np.abs(b))


def methanation():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import methanation as M
    return M


def param_vectors(M):
    """BASEPARAMS, the sharpened / slowed pair of test_methanation_dae.py, the first interior prior-box vector of test_dae_batch_vs_oracle."""
    lo, hi, pos = M.prior_box()
    pr = M.BASEPARAMS.copy()
    pr[:4] = (lo[pos] + (hi[pos] - lo[pos]) * np.random.RandomState(3).uniform(0.2, 0.8, 5))[:4]
    return [M.BASEPARAMS.copy(), M.BASEPARAMS * np.array([3.0, 1.0, 0.3, 1.0, 1, 1, 1, 1]), pr]


def cases(M=None):
    """The 12 runs: (experiment index, parameter-vector index, p0 row (18,), start state (357,)), parameter vector major."""
    M = M or methanation()
    cond = M.load_conditions(os.path.join(GOLD, "methanation_information.csv"))
    guess = M.initial_guess(cond)
    return [(i, k, M.p0_tuple(cond, i, pr), guess[i].copy()) for k, pr in enumerate(param_vectors(M)) for i in EXPERIMENTS]


# ---- the integrator: backward Euler on nested graded grids, Richardson extrapolation ------------------------------------------
def coarse_grid(n0=N0):
    """0, T_FIRST, then geometric segments T_FIRST -> 0.5 -> 5 -> 75 with the n0 - 1 remaining steps shared by their decades."""
    knots = (T_FIRST,) + TIMES
    dec = np.array([np.log10(b / a) for a, b in zip(knots[:-1], knots[1:])])
    n = np.maximum(1, np.round((n0 - 1) * dec / dec.sum()).astype(int))
    t = [np.array([0.0])]
    for a, b, m in zip(knots[:-1], knots[1:], n):
        t.append(a * (b / a) ** (np.arange(m) / m))
    t.append(np.array([knots[-1]]))
    return np.concatenate(t)


def bisect(t):
    out = np.empty(2 * len(t) - 1)
    out[0::2] = t
    out[1::2] = 0.5 * (t[:-1] + t[1:])
    return out


def _pool(workers=None):
    """At most 16 fresh processes (spawn: the parent may hold a GPU context)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return ProcessPoolExecutor(max_workers=workers or max(1, min(16, n)), mp_context=multiprocessing.get_context("spawn"))


class NewtonFailure(RuntimeError):
    pass


def backward_euler(M, y0, p, t, sample_at):
    """X(t[k]) by F(t1, X1, (X1 - X0) / h, p) = 0 from X(0) = y0 (the first step projects the algebraic variables: they enter F
    only through X1); a chord Newton with a finite-difference matrix of the step equation from ONE batch call of 357 rows,
    iterated to an update below NEWTON_UNITS.  Returns the states at the grid indices sample_at and the iteration statistics."""
    import scipy.linalg
    P = np.ascontiguousarray(np.tile(p, (NS, 1)))
    x0 = np.array(y0, dtype=np.float64)
    xm, hm = None, None
    lu, h_lu, last_its = None, None, 0
    out, want = [], set(int(s) for s in sample_at)
    stats = {"matrices": 0, "iterations": 0, "stalled": 0, "worst_final_update": 0.0}

    def G(x, h):
        return M.reaction(x, (x - x0) / h, p)

    def matrix(x, h):
        d = 1e-7 * (1.0 + np.abs(x))
        Xb = np.tile(x, (NS, 1))
        Xb[np.diag_indices(NS)] += d
        d = Xb[np.diag_indices(NS)] - x
        R = M.reaction(Xb, (Xb - x0) / h, P)
        stats["matrices"] += 1
        J = ((R - G(x, h)) / d[:, None]).T
        # rows with the diagonal as their only entry (X' = 0 at the inlet node, u[0] = u_in) are solved by themselves, so that the
        # elimination's rounding does not leak into them: the inlet node keeps its start values to the last bit
        single = np.flatnonzero((np.count_nonzero(J, axis=1) == 1) & (np.diag(J) != 0.0))
        return scipy.linalg.lu_factor(J), single, np.diag(J)[single]

    for k in range(1, len(t)):
        h = t[k] - t[k - 1]
        x = x0.copy() if xm is None else x0 + (x0 - xm) * (h / hm)
        if lu is None or abs(h / h_lu - 1.0) > 0.15 or last_its > 10:
            lu, h_lu = matrix(x, h), h
        prev, its = np.inf, 0
        while True:
            g = G(x, h)
            dx = scipy.linalg.lu_solve(lu[0], -g)
            dx[lu[1]] = -g[lu[1]] / lu[2]
            x = x + dx
            its += 1
            upd = np.max(units(x - dx, x))
            if upd < NEWTON_UNITS:
                break
            if upd < 1e-8 and upd > 0.5 * prev:      # the rounding of the residual: the update no longer contracts
                stats["stalled"] += 1
                break
            if its in (20, 40):
                lu, h_lu = matrix(x, h), h
            if its >= 60 or not np.isfinite(upd):
                raise NewtonFailure(f"step {k} of {len(t) - 1} (t = {t[k]:.3e}, h = {h:.3e}): update {upd:.3e} units after {its} iterations")
            prev = upd
        stats["worst_final_update"] = max(stats["worst_final_update"], upd)
        stats["iterations"] += its
        last_its = its
        xm, hm, x0 = x0, h, x
        if k in want:
            out.append(x.copy())
    return np.array(out), stats


def extrapolate(levels):
    """The full table: column k is (2^k T[j+1] - T[j]) / (2^k - 1), written as T[j+1] + (T[j+1] - T[j]) / (2^k - 1) so that equal
    entries stay equal to the last bit.  Returns the columns (lists of arrays)."""
    cols = [list(levels)]
    for k in range(1, len(levels)):
        c = cols[-1]
        cols.append([c[j + 1] + (c[j + 1] - c[j]) / (2.0 ** k - 1.0) for j in range(len(c) - 1)])
    return cols


def solve_truth(y0, p, n0=N0, levels=LEVELS, times=TIMES, M=None):
    """(states (len(times), 357), error bar (len(times), 357) in units, table) - the bar: best entry against the last entry of the
    column before it."""
    M = M or methanation()
    t, sols, table = coarse_grid(n0), [], {"steps": [], "stats": []}
    t = t[t <= times[-1] * (1 + 1e-12)]
    for _ in range(levels):
        at = [int(np.argmin(np.abs(t - s))) for s in times]
        assert all(t[a] == s for a, s in zip(at, times))
        y, st = backward_euler(M, y0, p, t, at)
        sols.append(y)
        table["steps"].append(len(t) - 1)
        table["stats"].append(st)
        t = bisect(t)
    cols = extrapolate(sols)
    best, before = cols[-1][0], cols[-2][-1]
    table["column_diffs"] = [[np.max(units(c[j], c[j + 1]), axis=1) for j in range(len(c) - 1)] for c in cols[:-1]]     # per sample time
    return best, units(before, best), table


def _truth_job(args):
    y0, p, n0, levels = args
    return solve_truth(y0, p, n0, levels)


def generate(n0=N0, levels=LEVELS, workers=None):
    """All 12 runs in a process pool; the dict that make_meth_dae_truth.py stores."""
    import scipy
    M = methanation()
    M.lib()
    cs = cases(M)
    with _pool(workers) as ex:
        res = list(ex.map(_truth_job, [(y0, p, n0, levels) for _, _, p, y0 in cs]))
    return {
        "p0": np.array([c[2] for c in cs]), "y0": np.array([c[3] for c in cs]),
        "experiment": np.array([c[0] for c in cs]), "param_vector": np.array([c[1] for c in cs]),
        "times": np.array(TIMES), "states": np.array([r[0] for r in res]),                      # (12, 3, 357)
        "bar": np.array([r[1].max(axis=1) for r in res]),                                       # (12, 3) units
        "grid_steps": np.array(res[0][2]["steps"]), "newton_units": NEWTON_UNITS,
        "worst_final_update": np.array([max(s["worst_final_update"] for s in r[2]["stats"]) for r in res]),
        "column_diffs_run0_t0": np.array([[float(x[0]) for x in d] + [np.nan] * (levels - 1 - len(d)) for d in res[0][2]["column_diffs"]]),
        "scipy_version": scipy.__version__, "numpy_version": np.__version__,
    }


def load():
    return np.load(FIXTURE)


# ---- the CPU statements of the integrators against the fixture ---------------------------------------------------------------------
def checker_solve(kind, y0, p, tf, tol):
    """(state at tf, attempts) of 'policy' (dae_solve_policy under k8_policy(): the CPU statement of K8), 'default' (dae_solve) or
    'ida' (dae_solve_ida, which delivers at its last communication point tf)."""
    M = methanation()
    if kind == "policy":
        y, rc, st = M.dae_solve_policy(y0, p, M.k8_policy(), tf=tf, rtol=tol, atol=tol)
    elif kind == "default":
        y, rc, st = M.dae_solve(y0, p, tf=tf, rtol=tol, atol=tol)
    else:
        y, rc, st = M.dae_solve_ida(y0, p, tf=tf, rtol=tol, atol=tol)
    assert rc == 0, (kind, tf, tol, rc)
    attempts = st["steps"] + st.get("rejects", st.get("error_test_failures", 0)) + st.get("newton_fail", st.get("newton_failures", 0))
    return y, attempts


def _checker_job(a):
    return checker_solve(*a)


def checker_runs(kind, fx, tols=TOLS, times=TIMES, scale_p=None, scale_tf=1.0, workers=None):
    """dist[c, it, itol] (worst of the 357 states, units) and attempts[c, it, itol] of a checker against the fixture fx; scale_p
    multiplies the 18 entries of every p0 row, scale_tf the final time (the planted errors of the tests)."""
    p0 = fx["p0"] * (1.0 if scale_p is None else scale_p)
    jobs = [(kind, fx["y0"][c], p0[c], tf * scale_tf, tol) for c in range(len(p0)) for tf in times for tol in tols]
    with _pool(workers) as ex:
        res = list(ex.map(_checker_job, jobs, chunksize=3))
    it_of = {t: k for k, t in enumerate(fx["times"])}
    dist, att = np.empty((len(p0), len(times), len(tols))), np.empty((len(p0), len(times), len(tols)), dtype=np.int64)
    for (j, (y, a)), idx in zip(enumerate(res), np.ndindex(*dist.shape)):
        dist[idx] = np.max(units(y, fx["states"][idx[0], it_of[times[idx[1]]]]))
        att[idx] = a
    return dist, att


def planted_p(j, rel=1e-4):
    s = np.ones(18)
    s[j] = 1.0 + rel
    return s


def bound(worst, bar):
    """The rule of dosed_model.K with the reference's own error added: 2 x the worst CPU distance + the fixture's error bar."""
    return 2.0 * worst + bar


def measure(fx=None):
    fx = fx or load()
    bar = fx["bar"].max(axis=0)                     # per time
    out = {"bar": bar}
    for kind in ("policy", "default", "ida"):
        d, a = checker_runs(kind, fx)
        out[kind] = d.max(axis=0)                   # [time, tol]
        out[kind + "_attempts"] = a.max(axis=0)
    return out


def main():
    np.set_printoptions(linewidth=160, precision=4)
    fx = load()
    print(f"fixture: grids {fx['grid_steps']}, SciPy {fx['scipy_version']}, NumPy {fx['numpy_version']}")
    print("error bar (units), worst of the 12 runs, at t =", fx["times"], ":", fx["bar"].max(axis=0))
    print("worst final Newton update (units):", fx["worst_final_update"].max())
    print("run 0 (experiment 0, BASEPARAMS), t = 0.5: differences of successive entries, column by column\n", fx["column_diffs_run0_t0"])
    m = measure(fx)
    for kind in ("policy", "default", "ida"):
        print(f"{kind}: worst distance to the fixture (units; rows t = 0.5, 5, 75; columns tol = 1e-6, 1e-7, 1e-8)\n", m[kind])
        print("  2 x worst + bar:\n", bound(m[kind], m["bar"][:, None]))
        print("  most attempts:\n", m[kind + "_attempts"])
    d, _ = checker_runs("default", fx)
    print("dae_solve, distance at 1e-8 / distance at 1e-6 per run and time:\n", d[:, :, 2] / d[:, :, 0])
    for name, kw in (("p0[11] x (1 + 1e-4)", {"scale_p": planted_p(11)}), ("p0[10] x (1 + 1e-4)", {"scale_p": planted_p(10)}),
                     ("tf x (1 + 1e-3)", {"scale_tf": 1 + 1e-3})):
        for kind in ("policy", "default"):
            d, _ = checker_runs(kind, fx, tols=(1e-6,), **kw)
            print(f"planted {name}, {kind} at 1e-6: least distance of the 12 runs per time", d[:, :, 0].min(axis=0))


if __name__ == "__main__":
    main()
