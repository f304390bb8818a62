"""The model, populations and designs of tests/test_predictive_planted.py: a user model whose outputs ARE its parameters, so that
the summary kernels (csrc/predictive_kernels.hip) see exactly the doubles a test uploaded - ties, adjacent doubles, signed zeros,
denormals, far-apart exponents - and NumPy on the uploaded array alone is the reference.  A helper module, not a test.

The model.  One state, y0 = 0, rhs = 0 (RK45 and BDF are exact on it; the first time of a row is served from y0, the later
ones from the dense output of a step), and
    out[k] = theta[gate] < cond[0] ? v_k(theta) : NaN      (k < 8)
with v_k = theta[k] for k < 7 and v_7 = a signed zero or denormal picked by |theta[4]| (a particle has at most SMC_MAX_DIM = 8
parameters, one of them the gate, so the eighth output is a table looked up with the integers of column 4: exact all the same).
theta[gate] is the GATE: the experiment's condition decides which particles are finite in that experiment's cells.  The
prediction kernels write a model's outputs as they are (user_obs_args.h: emit); NaN from the first time not served on is
what they write themselves past a row's end (pred_tail).  A NaN output is no failed solve, so n_failed stays 0 and a gated
particle cuts no row.  The observations are all NaN (nothing measured): the likelihood plays no part.

The population (n, 8) and the outputs it plants.  gate = 7: seven value columns and the gate.  gate = 6 (a model whose last
parameter is a noise level in (0.05, 0.2), for est_sigma and noise models): six value columns, the gate, the level; output 6 is
then -theta[5].
    0  normal x 10**U(-3, 3), mixed sign       the general case; digit 0 of the keys on both sides of the sign bit
    1  one value repeated                      every pass one bin, whole waves in the leader's ballot of hist_add
    2  x and nextafter(x, inf), 1 : 3          ranks that separate only in the last radix pass
    3  x0 + j ulp, random j < 4096             many ranks splitting in the last two passes, with repeats
    4  integers -7 .. 7 (zero is +0)           several bins per wave: leader path and lone-lane path of hist_add together
    5  column 0 sorted (descending: odd seed)  memory order correlated with waves
    6  +-10**U(-150, 150)                      far-apart exponents; mean and sd still finite
    7  +-0, +-5e-324, +-1e-310, +-DBL_MIN      signed zeros and denormals: SPECIALS[|theta[4]|], all eight present
    gate: a permutation of (i + 0.5) / n, so that cond = j / n leaves exactly j particles finite."""
import numpy as np

N_OBS = 8
# output 7 by a = |theta[4]| in 0 .. 7: magnitude a & 3, negative for a >= 4
SPECIALS = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, -0.0, -5e-324, -1e-310, -2.2250738585072014e-308])
X2_BITS = 0x3FF8A3D70A3D707F        # column 2's x, about 1.54: low byte 0x7f, so x and its successor share their top 7 bytes
X3_BITS = 0x4009E353F7CF0000        # column 3's x0, about 3.24: low 16 bits clear, so j < 4096 never carries past them


def source(gate=7, jac=False):
    """HIP text of the model; jac: with smc_user_jac, for method="BDF"."""
    assert gate in (6, 7)
    sig = "const double *theta, const double *cond"
    mag = [int(np.array([v]).view(np.uint64)[0]) for v in SPECIALS[:4]]
    vals = [f"theta[{k}]" for k in range(min(gate, 7))] + ["-theta[5]"] * (7 - gate) + ["((a & 4) ? -mag : mag)"]
    rows = "\n".join(f"    out[{k}] = open ? {v} : nan;" for k, v in enumerate(vals))
    s = (f"__device__ void smc_user_y0({sig}, double *y) {{ y[0] = 0.0; }}\n"
         f"__device__ void smc_user_rhs(double t, const double *y, {sig}, double *dydt) {{ dydt[0] = 0.0; }}\n"
         f"__device__ void smc_user_obs_vec(double t, const double *y, {sig}, double *out) {{\n"
         f"    const double nan = __longlong_as_double(0x7ff8000000000000LL);\n"
         f"    const bool open = theta[{gate}] < cond[0];\n"
         f"    const int a = (int)fabs(theta[4]);\n"
         f"    const double mag = __longlong_as_double((a & 3) == 0 ? {mag[0]}LL : (a & 3) == 1 ? {mag[1]}LL : (a & 3) == 2 ? {mag[2]}LL : {mag[3]}LL);\n"
         f"{rows}\n}}\n")
    if jac:
        s += f"__device__ void smc_user_jac(double t, const double *y, {sig}, double *J) {{ J[0] = 0.0; }}\n"
    return s


def population(n, seed, gate=7):
    """(n, 8) particles: the value families above in columns 0 .. gate - 1, the gate and, for gate = 6, a noise level at column 7."""
    assert gate in (6, 7)
    rs = np.random.RandomState(seed)
    th = np.empty((n, 8))
    th[:, 0] = rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 3, n)
    th[:, 1] = rs.standard_normal() * 10.0 ** rs.uniform(-3, 3)
    x = np.array([X2_BITS], dtype=np.uint64).view(np.float64)[0]
    th[:, 2] = np.where(rs.permutation(n) % 4 == 0, x, np.nextafter(x, np.inf))
    th[:, 3] = (np.uint64(X3_BITS) + rs.randint(0, 4096, n).astype(np.uint64)).view(np.float64)
    th[:, 4] = rs.randint(0, 8, n) * np.where(rs.permutation(n) % 2 == 0, 1.0, -1.0) + 0.0      # -0 + 0 = +0
    th[:, 5] = np.sort(th[:, 0])[::-1] if seed % 2 else np.sort(th[:, 0])
    th[:, 6] = np.where(rs.uniform(size=n) < 0.5, 1.0, -1.0) * 10.0 ** rs.uniform(-150, 150, n)
    level = rs.uniform(0.05, 0.2, n)
    th[:, gate] = (rs.permutation(n) + 0.5) / n
    if gate == 6:
        th[:, 7] = level
    return th


def outputs(th, gate=7):
    """(n, 8): what the model's eight outputs are for these particles when the gate is open."""
    v = np.empty((th.shape[0], N_OBS))
    v[:, :7] = th[:, :7]
    if gate == 6:
        v[:, 6] = -th[:, 5]
    v[:, 7] = SPECIALS[np.abs(th[:, 4]).astype(np.int64)]
    return v


# cells -> (times of a row, finite particles per experiment as (kind, value), the row cut short after its first time or None)
_FULL, _HALF = ("all", 0), ("half", 0)
_DESIGNS = {
    8: ([0.0], [_HALF], None),                                              # one time: served from y0 alone; a ragged tile
    32: ([0.0, 1.0], [_FULL, ("j", 3)], 1),                                 # one full transpose tile of cells
    120: ([0.0, 1.0, 2.0], [_FULL, _HALF, ("j", 2), ("j", 1), ("j", 0)], 2),
    264: ([0.0, 1.0, 2.0], [_FULL, _HALF, ("j", 3), ("j", 2), ("j", 1), ("j", 0), _FULL, _HALF, ("j", 3), ("j", 2), ("j", 1)], 6),
}
DESIGNS = tuple(_DESIGNS)


def design(cells, n):
    """(t, cond, m) of the design with that many cells for n particles: t (n_ex, n_t) with one row cut short by NaN, cond
    (n_ex, 1) gate thresholds j / n and m (n_ex,) the finite particles j they leave: n, about n / 2, 3, 2, 1 and 0 (at most n)."""
    times, kinds, short = _DESIGNS[cells]
    m = np.array([n if k == "all" else (n + 1) // 2 if k == "half" else min(v, n) for k, v in kinds], dtype=np.int64)
    t = np.tile(np.array(times), (len(kinds), 1))
    if short is not None:
        t[short, 1:] = np.nan
    assert t.size * N_OBS == cells
    return t, (m / n)[:, None], m


def planted(th, t, cond, gate=7):
    """What the model predicts, (n, n_ex, n_t, 8): NumPy on the uploaded particles alone."""
    is_open = th[:, gate, None] < np.asarray(cond)[None, :, 0]
    served = ~np.isnan(t)
    return np.where(is_open[:, :, None, None] & served[None, :, :, None], outputs(th, gate)[:, None, None, :], np.nan)
