"""The test population of tests/test_user_model_bdf.py (Robertson's kinetics under method="BDF") and the derivation of the
factor k of its per-output bound delta = k (atol + rtol |y|), run once on the CPU before the GPU test was written:

    python tests/robertson_bdf_bound.py          # prints the worst ratio and k = 2 x that ratio

SciPy's BDF at the test's tolerances is compared with Radau at rtol 1e-10 on every (particle, experiment) solve of the
population; the worst |y_bdf - y_radau| / (atol + rtol |y_radau|) over the observed outputs, doubled, is k.  Two BDF solves
that each stay within half of that bound of the true solution differ by at most delta: that is how far the device solve
may lie from SciPy's.  Also the SciPy side of the test: a BDF solve driven step by step (as solve_ivp does with t_eval),
with its step, LU and Jacobian counts."""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

RTOL, ATOL = 1e-4, 1e-8
K2 = 3e7
K_TRUE, SIGMA_TRUE = (0.04, 1e4), 0.01
A0 = np.array([1.0, 0.5, 2.0, 1.5])
N_T = 30
T = np.tile(np.linspace(0.0, 40.0, N_T), (len(A0), 1))
# main() on the population below printed a worst ratio of 5.269 (SciPy 1.15.3): k = 2 x 5.269, fixed before the first device run
K_BOUND = 10.54


def rhs(t, y, k1, k3):
    return np.array([-k1 * y[0] + k3 * y[1] * y[2], k1 * y[0] - k3 * y[1] * y[2] - K2 * y[1] * y[1], K2 * y[1] * y[1]])


def jac(t, y, k1, k3):
    return np.array([[-k1, k3 * y[2], k3 * y[1]], [k1, -k3 * y[2] - 2.0 * K2 * y[1], -k3 * y[1]], [0.0, 2.0 * K2 * y[1], 0.0]])


def population(n=512, seed=11):
    """Rate constants spread over two decades around the classic ones, sigma over a decade; noisy observations of C."""
    rs = np.random.RandomState(seed)
    th = np.column_stack([K_TRUE[0] * 10.0 ** rs.uniform(-1, 1, n), K_TRUE[1] * 10.0 ** rs.uniform(-1, 1, n),
                          rs.uniform(0.005, 0.05, n)])
    clean = np.array([bdf_solve(K_TRUE[0], K_TRUE[1], A0[e], T[e], True)[0] for e in range(len(A0))])
    obs = clean + SIGMA_TRUE * rs.standard_normal(clean.shape)
    return th, obs


def bdf_solve(k1, k3, a0, t_eval, analytic_jac, rtol=RTOL, atol=ATOL):
    """solve_ivp(method="BDF", t_eval) driven by hand: C at t_eval, accepted steps, LU factorisations, Jacobian evaluations."""
    from scipy.integrate import BDF
    s = BDF(lambda t, y: rhs(t, y, k1, k3), t_eval[0], np.array([a0, 0.0, 0.0]), t_eval[-1], rtol=rtol, atol=atol,
            jac=(lambda t, y: jac(t, y, k1, k3)) if analytic_jac else None)
    out, i, steps = [], 0, 0
    while s.status == "running":
        s.step()
        if s.status == "failed":
            return None, steps, s.nlu, s.njev
        steps += 1
        j = np.searchsorted(t_eval, s.t, side="right")      # ivp.py: the t_eval values up to and including t
        if j > i:
            out.append(s.dense_output()(t_eval[i:j])[2])
            i = j
    return np.concatenate(out), steps, s.nlu, s.njev


def scipy_row(args):
    """All experiments of one particle (k1, k3, analytic_jac): outputs (n_ex, n_t) and the summed counts."""
    k1, k3, analytic = args
    out = [bdf_solve(k1, k3, A0[e], T[e], analytic) for e in range(len(A0))]
    return np.array([o[0] for o in out]), sum(o[1] for o in out), sum(o[2] for o in out), sum(o[3] for o in out)


def loglik(r2, sigma, n_ex=len(A0), n_t=N_T):
    """The reference's Gaussian log-likelihood (Micmem_likelihood.py) from the summed squared residuals."""
    return n_ex * (-0.5 * n_t) * np.log(2 * np.pi * sigma * sigma) - r2 / (2 * sigma * sigma)


def _ratio(args):
    from scipy.integrate import solve_ivp
    k1, k3 = args
    worst = 0.0
    for e in range(len(A0)):
        yb = bdf_solve(k1, k3, A0[e], T[e], True)[0]
        yr = solve_ivp(rhs, [T[e, 0], T[e, -1]], [A0[e], 0.0, 0.0], method="Radau", t_eval=T[e], rtol=1e-10, atol=1e-14,
                       jac=jac, args=(k1, k3)).y[2]
        worst = max(worst, float(np.max(np.abs(yb - yr) / (ATOL + RTOL * np.abs(yr)))))
    return worst


def main():
    th, _ = population()
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        r = list(ex.map(_ratio, [(a, b) for a, b, _ in th], chunksize=8))
    w = max(r)
    print(f"worst |y_bdf - y_radau| / (atol + rtol |y|) over {len(th)} particles x {len(A0)} experiments: {w:.3f}; k = {2 * w:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
