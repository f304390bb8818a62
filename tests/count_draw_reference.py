"""csrc/count_draw.h restated in NumPy on philox_reference.philox_block_np: the replicated count draws of
smc_user_predict_summary(noise = 2) and of the count PIT, vectorised over any array of (particle, cell) with masks for the
rejection loops.  Every decision is the header's: the same doubles formed in the same order, with exp, log, cos, pow and lgamma
of the C library in double on them (element by element - NumPy's own vector versions may differ from libm in the last bit).  A helper module, not a test."""
import math

import numpy as np

import philox_reference as PR

TAG_PREDICT, TAG_PIT = 0x505245, 0x504954
GAUSSIAN, POISSON, NEGBIN = 0, 1, 2
LAST_BLOCK = 254
TWO52 = 4503599627370496.0


def _elementwise(fn):
    uf = np.frompyfunc(fn, 1, 1)

    def call(x):
        x = np.asarray(x, dtype=np.float64)
        return uf(x).astype(np.float64) if x.size else x.copy()
    return call


def _guard(fn, at_zero):
    def g(x):
        return at_zero if x == 0.0 else fn(x)
    return g


def _libm_lgamma():
    """lgamma of the C library (math.lgamma is CPython's own Lanczos sum, which differs from it in the last bits at large x)"""
    import ctypes
    import ctypes.util
    fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").lgamma
    fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
    return fn


_exp, _cos, _lgamma = _elementwise(math.exp), _elementwise(math.cos), _elementwise(_libm_lgamma())
_log = _elementwise(_guard(math.log, -math.inf))      # only of values >= 0
_log1p = _elementwise(math.log1p)


def _on(mask, fn, *args):
    """fn of the masked elements of args, 0 elsewhere"""
    out = np.zeros(mask.shape)
    if mask.any():
        out[mask] = fn(*[a[mask] for a in args])
    return out


class Supply:
    """The uniform supply of count_draw.h for an array of draws: blocks 1 .. 254 of the stream tag << 32 | cell, in order."""

    def __init__(self, seed, g, tag, cell):
        g, cell = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(cell, dtype=np.uint64))
        self.seed, self.g = int(seed), g.copy()
        self.stream = (np.uint64(tag) << np.uint64(32)) | (cell & np.uint64(0xFFFFFFFF))
        self.block = np.zeros(g.shape, dtype=np.int64)
        self.left = np.zeros(g.shape, dtype=np.int64)
        self.dry = np.zeros(g.shape, dtype=bool)
        self.q = [np.zeros(g.shape, dtype=np.uint64) for _ in range(4)]

    def _open(self, m):
        can = m & (self.block < LAST_BLOCK)
        self.dry |= m & ~can
        self.left[m & ~can] = 0
        self.block[can] += 1
        for blk in np.unique(self.block[can]):
            sel = can & (self.block == blk)
            r = PR.philox_block_np(self.seed, self.g[sel], self.stream[sel], int(blk))
            for i in range(4):
                self.q[i][sel] = r[i]
        self.left[can] = 2

    def uniform(self, m):
        """one uniform for every element of the mask m; 0.5 where the supply is dry (look at .dry)"""
        self._open(m & (self.left == 0))
        ok = m & ~self.dry
        u = np.where(self.left == 2, PR.u01_from(self.q[0], self.q[1]), PR.u01_from(self.q[2], self.q[3]))
        self.left[ok] -= 1
        return np.where(ok, u, 0.5)

    def normal(self, m):
        self._open(m)
        ok = m & ~self.dry
        self.left[ok] = 0
        u1, u2 = 1.0 - PR.u01_from(self.q[0], self.q[1]), PR.u01_from(self.q[2], self.q[3])
        z = _on(ok, lambda a, b: np.sqrt(-2.0 * _log(a)) * _cos(6.283185307179586 * b), u1, u2)
        return z


def _ptrs_bound(lam, k):
    """ptrs_bound of the header: the log of the Poisson probability of k, from lam = 2^18 on without the large terms"""
    big = lam >= 262144.0
    out = np.empty(lam.shape)
    d = (lam[big] - k[big]) / k[big]
    out[big] = -(k[big] * (d - _log1p(d))) - 0.5 * _log(6.283185307179586 * k[big]) - 1.0 / (12.0 * k[big])
    out[~big] = -lam[~big] + k[~big] * _log(lam[~big]) - _lgamma(k[~big] + 1.0)
    return out


def _poisson(s, lam, m, out):
    with np.errstate(all="ignore"):
        bad = m & (~(lam >= 0.0) | (lam == np.inf) | (lam >= TWO52))
        out[bad] = np.nan
        zero = m & ~bad & (lam == 0.0)
        out[zero] = 0.0
        act = m & ~bad & ~zero
        # inversion
        small = act & (lam < 10.0)
        u = s.uniform(small)
        out[small & s.dry] = np.nan
        small = small & ~s.dry
        p = _on(small, lambda x: _exp(-x), lam)
        c, k = p.copy(), np.zeros(lam.shape)
        run = small & (u > c) & (k < 128.0)
        while run.any():
            k[run] += 1.0
            p[run] = p[run] * (lam[run] / k[run])
            c[run] = c[run] + p[run]
            run = run & (u > c) & (k < 128.0)
        out[small] = k[small]
        # PTRS
        big = act & (lam >= 10.0)
        slam = np.sqrt(np.where(big, lam, 100.0))
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        while big.any():
            U = s.uniform(big) - 0.5
            V = s.uniform(big)
            out[big & s.dry] = np.nan
            big = big & ~s.dry
            us = 0.5 - np.abs(U)
            t = big & ~((us == 0.0) | (V == 0.0))
            us_ = np.where(t, us, 0.25)
            kk = np.floor((2.0 * a / us_ + b) * U + lam + 0.43)
            acc1 = t & (us >= 0.07) & (V <= vr)
            t2 = t & ~acc1 & ~((kk < 0.0) | ((us < 0.013) & (V > us)))
            lhs = _on(t2, lambda v, ia, aa, uu, bb: _log(v) + _log(ia) - _log(aa / (uu * uu) + bb), V, invalpha, a, us_, b)
            rhs = _on(t2, _ptrs_bound, lam, kk)
            acc = acc1 | (t2 & (lhs <= rhs))
            out[acc] = kk[acc]
            big = big & ~acc


def _pow(x, y):
    return np.array([math.pow(a, b) for a, b in zip(x, y)], dtype=np.float64)


def _gamma(s, shape, m, out):
    """Marsaglia-Tsang for the elements of m; returns the mask of those that got a value (the others are dry: out NaN)"""
    with np.errstate(all="ignore"):
        shape = np.where(m, shape, 1.0)
        boost = np.ones(shape.shape)
        low = m & (shape < 1.0)
        u0 = s.uniform(low)
        out[low & s.dry] = np.nan
        m = m & ~s.dry
        low = low & m
        boost[low] = _pow(u0[low], 1.0 / shape[low]) if low.any() else boost[low]
        shape = np.where(low, shape + 1.0, shape)
        d = shape - 1.0 / 3.0
        c = 1.0 / np.sqrt(9.0 * d)
        done = np.zeros(m.shape, dtype=bool)
        todo = m.copy()
        while todo.any():
            x = s.normal(todo)
            out[todo & s.dry] = np.nan
            todo = todo & ~s.dry
            v = 1.0 + c * x
            t = todo & ~(v <= 0.0)
            v = v * v * v
            u = s.uniform(t)
            out[t & s.dry] = np.nan
            todo = todo & ~s.dry
            t = t & ~s.dry
            x2 = x * x
            acc1 = t & (u < 1.0 - 0.0331 * (x2 * x2))
            t2 = t & ~acc1 & (u > 0.0)
            lu = _on(t2, _log, u)
            bound = _on(t2, lambda xx, dd, vv: 0.5 * xx + dd * (1.0 - vv + _log(vv)), x2, d, v)
            acc = acc1 | (t2 & (lu < bound))
            out[acc] = (d * v * boost)[acc]
            done |= acc
            todo = todo & ~acc
    return done


def count_draw(seed, g, cell, tag, family, mu, b=0.0):
    """count_draw of count_draw.h for arrays that broadcast: seed an int, g the global particle numbers, cell the global cells, tag
    an int, family 1 (Poisson) or 2 (negative binomial), mu the means, b the overdispersions.  Returns (draws, last_block): the
    counts as float64 (NaN by the header's rules) and the last Philox block each draw opened (0: it consumed nothing)."""
    g, cell, family, mu, b = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(cell, dtype=np.uint64), np.asarray(family),
                                                 np.asarray(mu, dtype=np.float64), np.asarray(b, dtype=np.float64))
    s = Supply(seed, g, tag, cell)
    out = np.full(g.shape, np.nan)
    with np.errstate(all="ignore"):
        ok = (mu >= 0.0) & (mu != np.inf)
        nb = family == NEGBIN
        _poisson(s, np.where(ok & ~nb, mu, 0.0), ok & ~nb, out)
        nbok = ok & nb & (b > 0.0) & (b != np.inf)
        b2 = np.where(nbok, b * b, 1.0)
        G = np.full(g.shape, np.nan)
        got = _gamma(s, 1.0 / b2, nbok, G)
        lam = np.where(got, mu * (b2 * G), 0.0)
        _poisson(s, lam, got, out)
    return out, s.block.copy()


def draws_for(seed, global_offset, n, cells, tag, family, mu, b=0.0):
    """The draws of particles global_offset .. global_offset + n - 1 on the GLOBAL cells `cells`: (n, len(cells)); family per
    cell or scalar, mu and b (n, len(cells)) or broadcastable to it."""
    g = (np.uint64(global_offset) + np.arange(n, dtype=np.uint64))[:, None]
    return count_draw(seed, g, np.asarray(cells, dtype=np.uint64)[None, :], tag, family, mu, b)[0]
