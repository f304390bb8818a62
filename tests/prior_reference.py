"""csrc/prior_draw.h restated in NumPy on count_draw_reference.Supply: the prior draws of the families of smc_set_prior_ex
(lognormal, gamma, beta, truncated normal) under the key (seed, global particle, tag 0x505249, cell = parameter index), decision
for decision, in double with the C library's functions element by element (count_draw_reference's conventions).  Beside each
draw it returns what a test needs to hold a device against it:

  blocks  the last Philox block the draw opened;
  err     a bound on |device - restated|, counted from the operation sequence (below);
  margin  the smallest distance of a rejection comparison of this draw from its threshold, in units of the comparison's scale
          (|lhs| + |rhs| + 1).  A test asserts margin > MARGIN before it compares anything: then no decision can fall the other
          way on a device whose log / cos / pow differ from the C library's in their last bits.

Error model: EPS = 2^-52; a device-library function (exp, log, pow) within 2 ulp of the exact value - the ROCm device-library
document with the per-function bounds is not among this project's files, so 2 ulp is ASSUMED for all of them; a Box-Muller normal within the
project's 35 EPS (test_predictive_planted._noise_bound); one rounding (EPS / 2, counted as EPS) per arithmetic operation.  Both
sides are double evaluations of the same expression, so the distance between them is at most twice the one-sided bound: `err`
below is 2 x the one-sided count.

  z normal:                  dz = 35 EPS
  lognormal  exp(a + b z):   argument t = a + b z, dt = b dz + 2 EPS |t|; x (dt + 2 EPS)
  gamma      b d v boost:    w = 1 + c z, dw = c dz + 2 EPS (1 + |c z|); v = w^3, dv = 3 w^2 dw + 2 EPS v; boost = pow(u0, 1 / shape)
                             with 1 / shape rounded: relative (|ln u0| / shape + 2) EPS; three products: 3 EPS
                             -> G (dv / v + boost's + 3 EPS), times scale: + EPS
  beta       lo + (hi - lo) G1 / (G1 + G2):   relative r1 + r2 + 3 EPS on the fraction f (r: the gammas' relative bounds),
                             (hi - lo) f (r1 + r2 + 5 EPS) + EPS |x|
  truncnormal a + b z:       b dz + 2 EPS |x|
A helper module, not a test."""
import math

import numpy as np

import count_draw_reference as R
import philox_reference as PR  # noqa: F401  (the supply draws through it)

TAG_PRIOR = 0x505249
LOGNORMAL, GAMMA, BETA, TRUNCNORMAL = 3, 4, 5, 6
EPS = float(np.finfo(float).eps)
DZ = 35 * EPS
MARGIN = 1e-12      # about 4500 EPS of the comparison's scale; the counted error of a comparison stays below 300 EPS of it for
                    # shapes up to 64 (the largest term, d dv = 3 sqrt(d) dz, is 250 EPS at d = 64)
_exp = R._elementwise(math.exp)


class _Margin:
    def __init__(self, shape):
        self.m = np.full(shape, np.inf)

    def note(self, mask, lhs, rhs):
        with np.errstate(all="ignore"):
            rel = np.abs(lhs - rhs) / (np.abs(lhs) + np.abs(rhs) + 1.0)
        sel = mask & np.isfinite(rel)
        self.m[sel] = np.minimum(self.m[sel], rel[sel])


def _gamma(s, shape, m, mg):
    """gamma_mt of count_draw.h for the elements of m (count_draw_reference._gamma with the margins noted and the error counted):
    returns (G, relative error bound, mask of the elements that got a value)."""
    out, rel = np.full(m.shape, np.nan), np.zeros(m.shape)
    with np.errstate(all="ignore"):
        shape = np.where(m, shape, 1.0)
        boost, rboost = np.ones(m.shape), np.zeros(m.shape)
        low = m & (shape < 1.0)
        u0 = s.uniform(low)
        m = m & ~s.dry
        low = low & m
        if low.any():
            boost[low] = R._pow(u0[low], 1.0 / shape[low])
            rboost[low] = (np.abs(R._log(u0[low])) / shape[low] + 2.0) * EPS
        shape = np.where(low, shape + 1.0, shape)
        d = shape - 1.0 / 3.0
        c = 1.0 / np.sqrt(9.0 * d)
        done = np.zeros(m.shape, dtype=bool)
        todo = m.copy()
        while todo.any():
            x = s.normal(todo)
            todo = todo & ~s.dry
            w = 1.0 + c * x
            mg.note(todo, w, np.zeros(m.shape))
            t = todo & ~(w <= 0.0)
            v = w * w * w
            u = s.uniform(t)
            todo = todo & ~s.dry
            t = t & ~s.dry
            x2 = x * x
            squeeze = 1.0 - 0.0331 * (x2 * x2)
            mg.note(t, u, squeeze)
            acc1 = t & (u < squeeze)
            t2 = t & ~acc1 & (u > 0.0)
            lu = R._on(t2, R._log, u)
            bound = R._on(t2, lambda xx, dd, vv: 0.5 * xx + dd * (1.0 - vv + R._log(vv)), x2, d, v)
            mg.note(t2, lu, bound)
            acc = acc1 | (t2 & (lu < bound))
            out[acc] = (d * v * boost)[acc]
            dw = c * DZ + 2 * EPS * (1.0 + np.abs(c * x))
            rel[acc] = ((3.0 * w * w * dw + 2 * EPS * v) / v + rboost + 3 * EPS)[acc]
            done |= acc
            todo = todo & ~acc
    return out, rel, done


def prior_draw(seed, g, cell, kind, a, b, lo=0.0, hi=0.0):
    """prior_draw of prior_draw.h for arrays that broadcast: seed an int, g the global particle numbers, cell the parameter
    indices, kind 3 .. 6, (a, b, lo, hi) as smc_set_prior_ex takes them.  Returns (draws, blocks, err, margin), see the top."""
    g, cell, kind, a, b, lo, hi = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(cell, dtype=np.uint64), np.asarray(kind),
                                                      *[np.asarray(v, dtype=np.float64) for v in (a, b, lo, hi)])
    s = R.Supply(seed, g, TAG_PRIOR, cell)
    out, err = np.full(g.shape, np.nan), np.zeros(g.shape)
    mg = _Margin(g.shape)
    with np.errstate(all="ignore"):
        m = kind == LOGNORMAL
        if m.any():
            z = s.normal(m)
            ok = m & ~s.dry
            t = a + b * z
            out[ok] = R._on(ok, _exp, t)[ok]
            err[ok] = (np.abs(out) * (b * DZ + 2 * EPS * np.abs(t) + 2 * EPS))[ok]
        m = kind == GAMMA
        if m.any():
            G, rel, got = _gamma(s, np.where(m, a, 1.0), m, mg)
            out[got] = (b * G)[got]
            err[got] = (np.abs(b * G) * (rel + EPS))[got]
        m = kind == BETA
        if m.any():
            G1, r1, got1 = _gamma(s, np.where(m, a, 1.0), m, mg)
            G2, r2, got = _gamma(s, np.where(got1, b, 1.0), got1, mg)
            f = G1 / (G1 + G2)
            x = lo + (hi - lo) * f
            out[got] = x[got]
            err[got] = (np.abs((hi - lo) * f) * (r1 + r2 + 5 * EPS) + EPS * np.abs(x))[got]
        todo = kind == TRUNCNORMAL
        while todo.any():
            z = s.normal(todo)
            todo = todo & ~s.dry
            x = a + b * z
            for edge in (lo, hi):                                  # a comparison with an infinite bound is never near
                mg.note(todo & np.isfinite(edge), x, np.where(np.isfinite(edge), edge, 0.0))
            acc = todo & (x >= lo) & (x <= hi)
            out[acc] = x[acc]
            err[acc] = (b * DZ + 2 * EPS * np.abs(x))[acc]
            todo = todo & ~acc
    return out, s.block.copy(), 2.0 * err, mg.m


def draws_for(seed, global_offset, n, layout):
    """The new-kind columns of sample_prior_kernel for particles global_offset .. global_offset + n - 1 under the arrays
    layout = (kind, a, b, lo, hi) of priors.prior_layout: (x, blocks, err, margin), each (n, d) with NaN / 0 / 0 / inf in the
    columns of the old kinds (those come from philox_reference.prior_draw)."""
    kind, a, b, lo, hi = layout
    d = len(kind)
    x, blocks, err, margin = np.full((n, d), np.nan), np.zeros((n, d), dtype=np.int64), np.zeros((n, d)), np.full((n, d), np.inf)
    g = np.uint64(global_offset) + np.arange(n, dtype=np.uint64)
    for c in range(d):
        if kind[c] >= LOGNORMAL:
            x[:, c], blocks[:, c], err[:, c], margin[:, c] = prior_draw(seed, g, c, int(kind[c]), a[c], b[c], lo[c], hi[c])
    return x, blocks, err, margin
