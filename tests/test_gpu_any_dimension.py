"""What sits between two likelihood sweeps, at every parameter count d = 1 .. 8 (SMC_MAX_DIM): the layout kernels
(aos_to_soa_kernel, soa_to_aos_kernel), the moment kernels (moment_sum_kernel, moment_centered_kernel and the two-pass start
of the fused factor), the three gather kernels of the resampler (resample_gather_kernel, resample_gather_all_kernel,
resample_stale_rows_kernel) and the [component][count] blocks of d + 1 rows that travel between ranks (smc_resample_phase3,
peer_pull_copies, peer_exchange).  All of it is generic in d and was pinned exactly at d = 3 only.  No model is needed: the
engines here hold none.

Planted population: x[i, c] = (i + 1) + (c + 1) / 16 - exact in a double and distinct, so a row or a component that arrives
from the wrong place is identifiable from its value.  Grid: d in {1, 2, 4, 7, 8} (3 as the control), n in {1, 63, 64, 65, 257,
1025} - one lane, a wave and its neighbours, a 256-block plus one, a scan tile plus one.

Bounds of the moment tests (derived, not tuned; u = eps / 2 is the unit roundoff):
  column sums        |got - fsum| <= n eps sum|x_i|: the bound (n - 1) u sum|x| of ANY summation order, with a factor 2 of slack;
  centred sums       about the mean the test passes in, against exact rational arithmetic over the same doubles rounded once
                     (integer numerators over one power-of-two denominator, fractions.Fraction for the final rounding):
                     (n + 4) eps sum|(x_a - m_a)(x_b - m_b)| - two subtractions, one product, any summation order;
  cov of the factor  the same reference about the mean the device forms (its own column sums / n, one correctly rounded
                     division), times w_cov / n, under the same bound scaled by w_cov / n (1 / n rounded, two products: inside
                     the + 4 and the factor 2 between eps and u).
Measured on an MI355X, worst ratio to the bound per d over the six sizes (sums / centred / cov):
    d = 1   0.0020 / 0.0090 / 0.0089        d = 4   0.0080 / 0.0161 / 0.0167
    d = 2   0.0083 / 0.0109 / 0.0125        d = 7   0.0141 / 0.0128 / 0.0135
    d = 3   0.0123 / 0.0101 / 0.0135        d = 8   0.0154 / 0.0158 / 0.0174
(the block trees are some sixty times more accurate than the worst case of an arbitrary order; a wrong or missing term is of
order 1 / (n eps) bounds.)

Resampling.  Weight patterns spread (sigma = 30 at gm = 0.05), one_hot, last_only, underflow_tail (the definitions of
test_resample_degenerate_weights, gm = 1) with u = 0.318 - not within an ulp of 0 or 1, where the summation order of the scan
may name another particle than the sequential loop (stage_kernels.hip; oracle.resample_python at u = 1 - 2^-53 writes n - 1
rows for several of these patterns, which is a property of one summation order).  Rows nobody writes are FORCED: the weight
sum handed to the engine is doubled, so the weights sum to 1/2 and about n / 2 offspring result; the CPU part asserts that the
oracle's written count lies in [0.4 n, 0.6 n] for every (n, pattern) used (n = 1 is left out of that part: one row cannot be
half written).  Three ranks on one GPU: n = 3 x 257 with nearly all weight on rank 0, so its offspring travel; with the doubled
sum rank 1 is partly stale, rank 2 receives nothing and is stale throughout, rank 0 still sends.

Mutations, each on a copy of the library (every one stays inside the buffers), and the tests that fail:
    resample_gather_kernel copies min(d, 5) components              test_gathered_rows_are_their_ancestors and
                                                                    test_rows_nobody_writes_... at d = 7, 8 (every n), the three-rank
                                                                    test at d = 8 (both variants); d <= 4 passes
    resample_gather_all_kernel copies min(d, 5) components          the same two one-rank tests at d = 7, 8 (the enqueued half)
    smc_resample_phase3 packs lk into row d - 1 of the send block   test_three_ranks_exchange_blocks_of_d_plus_one_rows, d = 1 and 8,
                                                                    both variants (and the sharded runs of test_user_sharded.py)
    resample_stale_rows_kernel writes zeros whatever first_step     test_rows_nobody_writes_... at every (d, n), the three-rank test
    the else-branch of resample_gather_all_kernel likewise          test_rows_nobody_writes_... at every (d, n)
    smc_moment_centered_local reads its sums with d = 3 packing     test_moments_stay_within_the_summation_bounds and
                                                                    test_a_constant_column_... at d = 4, 7, 8; d <= 3 passes
    moment_sum_kernel sums min(d, 5) columns                        the same two tests at d = 7, 8
    moment_centered_kernel pairs column b >= 5 as column 4          the same two tests at d = 7, 8
    both layout kernels swap components 5 and 6 (consistently)      the round trip passes, as it must; the bounds test fails at d = 7, 8
                                                                    (the column sums arrive in the wrong place), the constant column at 7
"""
import fractions
import functools
import math
import threading

import numpy as np
import pytest

D_GRID = (1, 2, 4, 7, 8)
D_CTRL = (1, 2, 3, 4, 7, 8)          # with the control d = 3, where a test is new even for it
N_GRID = (1, 63, 64, 65, 257, 1025)
N_STALE = N_GRID[1:]                  # n = 1 left out: one row cannot be half written
PATTERNS = ("spread", "one_hot", "last_only", "underflow_tail")
SCHEMES = ("residual_systematic", "systematic", "multinomial")
U = 0.318
EPS = np.finfo(float).eps
SCAN_TILE = 1024                      # kScanTile of stage_kernels.hip: 256 threads x 4 particles


def planted(n, d):
    return (np.arange(n, dtype=np.float64)[:, None] + 1.0) + (np.arange(d, dtype=np.float64)[None, :] + 1.0) / 16.0


def pattern_lk(pattern, n):
    """(lk, gm): the weight patterns of test_resample_degenerate_weights and the spread one of test_resample_vs_oracle."""
    lk = np.zeros(n)
    if pattern == "spread":
        return np.random.RandomState(n).standard_normal(n) * 30.0, 0.05
    if pattern == "one_hot":
        lk[:] = -1e6
        lk[n // 3] = 0.0
    elif pattern == "last_only":
        lk[:] = -1e6
        lk[n - 1] = 0.0
    elif pattern == "underflow_tail":
        lk = -np.arange(n, dtype=float) * 30.0
    else:
        raise ValueError(pattern)
    return lk, 1.0


def weight_case(pattern, n, halve):
    """lk and the es dict of driver.resample; halve: the engine is told twice the weight sum, so the weights sum to 1/2."""
    lk, gm = pattern_lk(pattern, n)
    mx = float(lk.max())
    w = np.exp((lk - mx) * gm)
    sum_w = float(np.sum(w)) * (2.0 if halve else 1.0)
    return lk, w / sum_w, {"max_lk": mx, "gm": gm, "sum_weight": sum_w}


_ORACLE = {}


def oracle_case(O, pattern, n, d, halve, first_step):
    """O.resample on the planted population (computed once per case and shared; the arrays are not to be changed): offspring,
    written count and the WHOLE p_filt / lk1 - rows nobody writes hold zeros in the first step and the PRED rows later."""
    key = (pattern, n, d, halve, first_step)
    if key not in _ORACLE:
        lk, w, _ = weight_case(pattern, n, halve)
        _ORACLE[key] = _run_oracle(O, w, lk, planted(n, d), first_step)
    return _ORACLE[key]


def _run_oracle(O, w, lk, p_pred, first_step):
    p_filt = np.zeros_like(p_pred) if first_step else p_pred.copy()
    lk1 = np.zeros_like(lk) if first_step else lk.copy()
    p_is, n_written, _ = O.resample(w, U, p_pred, lk, p_filt, lk1)
    return p_is, int(n_written), p_filt, lk1


# ---- CPU: the conditions the GPU part relies on ------------------------------------------------------------------------

def test_the_grid_covers_every_path_of_the_kernels():
    assert set(D_GRID) >= {1, 2, 7, 8} and max(D_GRID) == 8 and 3 in D_CTRL and 3 not in D_GRID
    assert any(d > 5 for d in D_GRID)                                  # above the methanation model's d = 5
    assert {1, 63, 64, 65} <= set(N_GRID)                              # one lane, a wave and its neighbours
    assert any(n == 256 + 1 for n in N_GRID) and any(n == SCAN_TILE + 1 for n in N_GRID)
    x = planted(1025, 8)
    assert np.unique(x).size == x.size                                 # every value names its row and component
    assert np.array_equal(x * 16.0, np.round(x * 16.0))                # ... and is exact in a double


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", N_STALE)
def test_half_the_weight_leaves_about_half_the_rows_unwritten(O, n, pattern):
    """Part (d) forces stale rows; this is the proof that it does, for every (n, pattern) of the GPU part (the oracle's counts
    do not depend on d: d = 1 and d = 8 are both run).  n = 1 is left out."""
    for d in (1, 8):
        p_is, n_written, p_filt, _ = oracle_case(O, pattern, n, d, True, True)
        assert 0.4 * n <= n_written <= 0.6 * n, (n, pattern, n_written)
        assert p_is.sum() == n_written and np.all(p_filt[n_written:] == 0.0) and np.all(p_filt[:n_written] != 0.0)
    p_is, n_written, _, _ = oracle_case(O, pattern, n, 8, False, True)
    assert n_written == n == p_is.sum()                                # ... and the full weight writes every row


def test_three_rank_case_sends_from_rank_zero_and_starves_rank_two(O):
    for d in (1, 8):
        for halve in (False, True):
            p_is, n_written, _, _ = _three_rank_oracle(O, d, halve, True)
            assert p_is[:NL3].sum() > 0.9 * n_written                  # rank 0's offspring fill the other ranks' rows
            if halve:
                assert NL3 + 64 < n_written < 2 * NL3 - 64             # rank 1 partly stale, rank 2 throughout
            else:
                assert n_written == 3 * NL3


# ---- (a) layout round trip ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", N_GRID)
@pytest.mark.parametrize("d", D_CTRL)
def test_layout_round_trip_is_bit_exact(pkg, d, n):
    """upload_particles / download_particles (aos_to_soa_kernel, soa_to_aos_kernel) and upload_lk / download_lk on both sets:
    bit for bit, the other set untouched, and a partial upload leaves the rows above it alone."""
    x = planted(n, d)
    y = -planted(n, d)[::-1].copy() - 4096.0
    lx, ly = -(np.arange(n) + 1.0) - 1.0 / 32.0, (np.arange(n) + 1.0) * 3.0 + 1.0 / 64.0
    with pkg.HipEngine(n, d, device=0) as eng:
        P, F = pkg.SMC_SET_PRED, pkg.SMC_SET_FILT
        eng.upload_particles(P, x)
        eng.upload_lk(P, lx)
        assert np.array_equal(eng.download_particles(P), x) and np.array_equal(eng.download_lk(P), lx)
        assert np.all(eng.download_particles(F) == 0.0) and np.all(eng.download_lk(F) == 0.0)      # a fresh engine's other set
        eng.upload_particles(F, y)
        eng.upload_lk(F, ly)
        assert np.array_equal(eng.download_particles(F), y) and np.array_equal(eng.download_lk(F), ly)
        assert np.array_equal(eng.download_particles(P), x) and np.array_equal(eng.download_lk(P), lx)
        eng.upload_particles(P, y)                                      # the other direction
        eng.upload_lk(P, ly)
        assert np.array_equal(eng.download_particles(P), y) and np.array_equal(eng.download_particles(F), y)
        m = n // 2
        if m:                                                           # the first m rows only
            eng.upload_particles(F, x[:m])
            eng.upload_lk(F, lx[:m])
            assert np.array_equal(eng.download_particles(F), np.concatenate([x[:m], y[m:]]))
            assert np.array_equal(eng.download_lk(F), np.concatenate([lx[:m], ly[m:]]))
            assert np.array_equal(eng.download_particles(F, m), x[:m]) and np.array_equal(eng.download_particles(P), y)


# ---- (b) moments -------------------------------------------------------------------------------------------------------

def cloud(d, n):
    """A badly scaled, correlated cloud far from zero: column scales 10^-3 .. 10^2, |mean| / sd from 1 to 10^6."""
    rs = np.random.RandomState(100 * d + n % 97)
    scale = 10.0 ** np.linspace(-3.0, 2.0, d) if d > 1 else np.array([1e-3])
    far = 10.0 ** np.linspace(6.0, 0.0, d)
    mix = rs.standard_normal((d, d)) + 2.0 * np.eye(d)
    z = rs.standard_normal((n, d)) @ mix
    sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    return (z / np.sqrt(np.sum(mix * mix, axis=0)) + sign * far) * scale


def _as_ints(*arrays):
    """The doubles of the arrays as Python ints over ONE denominator 2^K: exact rational arithmetic from there on."""
    ratios = [[float(v).as_integer_ratio() for v in np.asarray(a, dtype=np.float64).ravel()] for a in arrays]
    K = max(den.bit_length() - 1 for r in ratios for _, den in r)
    return [[num << (K - (den.bit_length() - 1)) for num, den in r] for r in ratios], K


def exact_centred(x, mean):
    """sum_i (x_ia - m_a)(x_ib - m_b) in exact arithmetic, rounded once, and sum_i |(x_ia - m_a)(x_ib - m_b)|: (d, d) each."""
    n, d = x.shape
    (X, M), K = _as_ints(x, mean)
    dev = [[X[i * d + c] - M[c] for c in range(d)] for i in range(n)]
    ref, mag = np.zeros((d, d)), np.zeros((d, d))
    for a in range(d):
        for b in range(a, d):
            tot = sum(r[a] * r[b] for r in dev)
            tot_abs = sum(abs(r[a] * r[b]) for r in dev)
            ref[a, b] = ref[b, a] = float(fractions.Fraction(tot, 1 << (2 * K)))
            mag[a, b] = mag[b, a] = float(fractions.Fraction(tot_abs, 1 << (2 * K)))
    return ref, mag


def _ratio(err, bound):
    """worst err / bound; a zero bound admits a zero error only"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(err[bound == 0.0] == 0.0)
    return float(np.max(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), 0.0)))


@pytest.mark.gpu
@pytest.mark.parametrize("d", D_CTRL)
def test_moments_stay_within_the_summation_bounds(pkg, d):
    """moment_sums_local, moment_centered_local and proposal_factor_device against fsum and exact rational arithmetic, under
    the bounds of the module's text; prints the worst ratio to each bound over the six sizes."""
    worst = {"sums": 0.0, "centred": 0.0, "cov": 0.0}
    w = np.full((d, d), 0.5)
    for n in N_GRID:
        x = cloud(d, n)
        sd = x.std(axis=0)
        if n >= 63:
            assert np.abs(x.mean(axis=0) / sd).max() > 1e5 and (d == 1 or sd.max() / sd.min() > 1e4)     # the cloud is what it says
        with pkg.HipEngine(n, d, device=0) as eng:
            eng.upload_particles(pkg.SMC_SET_FILT, x)
            eng.upload_particles(pkg.SMC_SET_PRED, -x[::-1].copy())     # the moments are FILT's, whatever PRED holds
            sums = eng.moment_sums_local()
            ref_s = np.array([math.fsum(x[:, c]) for c in range(d)])
            r_s = _ratio(np.abs(sums - ref_s), n * EPS * np.abs(x).sum(axis=0))
            mean = ref_s / n
            cent = eng.moment_centered_local(mean)
            ref_c, mag = exact_centred(x, mean)
            r_c = _ratio(np.abs(cent - ref_c), (n + 4) * EPS * mag)
            assert np.array_equal(cent, cent.T)
            cov, xf = eng.proposal_factor_device(w)
            assert np.array_equal(eng.moment_sums_local(), sums)        # the same kernel, the same order: the device's mean
            ref_d, mag_d = exact_centred(x, sums / float(n))
            r_v = _ratio(np.abs(cov - ref_d * w / n), (n + 4) * EPS * mag_d * w / n)
        print(f"d = {d}, n = {n}: ratio to the bound: sums {r_s:.3g}, centred {r_c:.3g}, cov {r_v:.3g}")
        assert r_s <= 1.0 and r_c <= 1.0 and r_v <= 1.0, (d, n, r_s, r_c, r_v)
        # the factor reproduces cov_m (test_device_mvn_factor_any_dimension's bar) and is NumPy's SVD factor up to row signs
        assert np.abs(xf.T @ xf - cov).max() <= 1e-12 * np.abs(cov).max()
        if n == 1:
            assert np.all(cent == 0.0) and np.all(cov == 0.0) and np.all(xf == 0.0)
        for k, v in (("sums", r_s), ("centred", r_c), ("cov", r_v)):
            worst[k] = max(worst[k], v)
    print(f"d = {d}: worst ratio to the bound over n = {N_GRID}: sums {worst['sums']:.3g}, centred {worst['centred']:.3g}, "
          f"cov {worst['cov']:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", D_CTRL)
def test_a_constant_column_has_exactly_zero_variance(pkg, d):
    """A column of identical values (3.0: every partial sum is an integer, the device's mean is exact) gives exactly 0 in its
    row and column of the centred sums and of cov_m, whatever the other columns hold - at d = 8 the last of 36 pairs."""
    for n in (1, 257, 1025):
        for col in sorted({0, d - 1}):
            x = cloud(d, n)
            x[:, col] = 3.0
            with pkg.HipEngine(n, d, device=0) as eng:
                eng.upload_particles(pkg.SMC_SET_FILT, x)
                mean = np.array([math.fsum(x[:, c]) for c in range(d)]) / n
                assert mean[col] == 3.0 and eng.moment_sums_local()[col] == 3.0 * n
                cent = eng.moment_centered_local(mean)
                cov, _ = eng.proposal_factor_device(np.full((d, d), 0.5))
            assert np.all(cent[col] == 0.0) and np.all(cent[:, col] == 0.0), (d, n, col)
            assert np.all(cov[col] == 0.0) and np.all(cov[:, col] == 0.0), (d, n, col)
            if n > 1 and d > 1:
                other = [c for c in range(d) if c != col]
                assert np.all(np.diag(cent)[other] > 0.0) and np.all(np.diag(cov)[other] > 0.0)


# ---- (c), (d) gather after resampling, rows nobody writes --------------------------------------------------------------

def _resample_once(pkg, eng, n, scheme, es, lk, p_pred, first_step, defer):
    """One resampling on an engine whose FILT set holds the reversed population: (n_offspring, offspring, FILT rows, FILT lk)."""
    eng.set_resampling(scheme)
    eng.upload_particles(pkg.SMC_SET_PRED, p_pred)
    eng.upload_lk(pkg.SMC_SET_PRED, lk)
    eng.upload_particles(pkg.SMC_SET_FILT, -p_pred[::-1].copy())        # recognisable where nobody writes
    eng.upload_lk(pkg.SMC_SET_FILT, -lk[::-1].copy() + 0.5)
    out = pkg.resample(eng, pkg.SingleComm(), es, U, pkg.SMCSettings(n_particle=n, resampling=scheme), first_step=first_step,
                       defer=defer)
    if defer:
        assert callable(out)
        out = out()
    return out["n_offspring"], eng.download_offspring(), eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT)


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_GRID)
@pytest.mark.parametrize("d", D_GRID)
def test_gathered_rows_are_their_ancestors(pkg, O, d, n):
    """Every scheme, synchronous (resample_gather_kernel) and enqueued (resample_gather_all_kernel), four weight patterns: the
    FILT rows and lk below the offspring total are p_pred[anc] and lk[anc] bit for bit, anc = repeat(arange(n), offspring);
    residual_systematic: offspring, count and rows equal the sequential oracle."""
    p_pred = planted(n, d)
    with pkg.HipEngine(n, d, device=0) as eng:
        for pattern in PATTERNS:
            lk, _, es = weight_case(pattern, n, False)
            for scheme in SCHEMES:
                for defer in (False, True):
                    what = (d, n, pattern, scheme, defer)
                    tot, p_is, f, l = _resample_once(pkg, eng, n, scheme, es, lk, p_pred, True, defer)
                    assert p_is.sum() == tot and 0 < tot <= n, what
                    anc = np.repeat(np.arange(n), p_is)
                    assert np.array_equal(f[:tot], p_pred[anc]) and np.array_equal(l[:tot], lk[anc]), what
                    if scheme == "residual_systematic":
                        r_is, r_tot, r_f, r_l = oracle_case(O, pattern, n, d, False, True)
                        assert np.array_equal(p_is, r_is) and tot == r_tot == n, what
                        assert np.array_equal(f, r_f) and np.array_equal(l, r_l), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", N_STALE)
@pytest.mark.parametrize("d", D_GRID)
def test_rows_nobody_writes_hold_zeros_first_and_the_pred_rows_later(pkg, O, d, n):
    """Weights that sum to 1/2 (the CPU part shows: 0.4 n .. 0.6 n rows written).  Rows at and above the offspring total are
    exactly 0 with first_step, exactly the PRED rows at the same index without - resample_stale_rows_kernel (synchronous) and
    the else-branch of resample_gather_all_kernel (enqueued), every scheme; residual_systematic equals the oracle entirely."""
    p_pred = planted(n, d)
    with pkg.HipEngine(n, d, device=0) as eng:
        for pattern in PATTERNS:
            lk, _, es = weight_case(pattern, n, True)
            for scheme in SCHEMES:
                for first in (True, False):
                    for defer in (False, True):
                        what = (d, n, pattern, scheme, first, defer)
                        tot, p_is, f, l = _resample_once(pkg, eng, n, scheme, es, lk, p_pred, first, defer)
                        assert p_is.sum() == tot and 0 < tot < n, what
                        if scheme != "multinomial":        # its count is a draw (binomial about n / 2), the others' is arithmetic
                            assert 0.4 * n <= tot <= 0.6 * n, what
                        anc = np.repeat(np.arange(n), p_is)
                        assert np.array_equal(f[:tot], p_pred[anc]) and np.array_equal(l[:tot], lk[anc]), what
                        if first:
                            assert np.all(f[tot:] == 0.0) and np.all(l[tot:] == 0.0), what
                        else:
                            assert np.array_equal(f[tot:], p_pred[tot:]) and np.array_equal(l[tot:], lk[tot:]), what
                        if scheme == "residual_systematic":
                            r_is, r_tot, r_f, r_l = oracle_case(O, pattern, n, d, True, first)
                            assert np.array_equal(p_is, r_is) and tot == r_tot, what
                            assert np.array_equal(f, r_f) and np.array_equal(l, r_l), what


# ---- (e) three ranks on one GPU ----------------------------------------------------------------------------------------

NL3, W3 = 257, 3


@functools.lru_cache(maxsize=None)
def _three_rank_inputs(d):
    n = NL3 * W3
    lk = np.random.RandomState(12).standard_normal(n) * 3.0
    lk[:NL3] += 25.0                   # rank 0 holds nearly all the weight (test_multi_rank_resample_exchange_exact)
    mx, gm = float(lk.max()), 0.3
    return lk, planted(n, d), {"max_lk": mx, "gm": gm, "sum_weight": float(np.sum(np.exp((lk - mx) * gm)))}


def _three_rank_oracle(O, d, halve, first_step):
    lk, p_pred, es = _three_rank_inputs(d)
    key = ("three_ranks", NL3 * W3, d, halve, first_step)
    if key not in _ORACLE:
        w = np.exp((lk - es["max_lk"]) * es["gm"]) / (es["sum_weight"] * (2.0 if halve else 1.0))
        _ORACLE[key] = _run_oracle(O, w, lk, p_pred, first_step)
    return _ORACLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("peer", [False, True], ids=["host_pull", "in_engine"])
@pytest.mark.parametrize("d", [1, 8])
def test_three_ranks_exchange_blocks_of_d_plus_one_rows(pkg, O, d, peer):
    """Three ranks of 257 particles on one GPU, nearly all weight on rank 0: offspring, FILT rows and lk concatenated over the
    ranks equal the sequential oracle exactly - with the full weight sum (every rank receives), and with the doubled one (385
    rows or so: rank 1 partly stale, rank 2 receives nothing and is stale throughout, rank 0 still sends), first_step on and
    off, each TWICE in a row on the same engines (send staging and pull events reused).  host_pull: debug_set_local_peers +
    the Python communicator (smc_resample_phase3 + smc_resample_phase3_pull); in_engine: debug_peer_collectives + PeerComm
    (smc_resample_global, peer_exchange)."""
    from _thread_comm import PeerComm, ThreadWorld
    n = NL3 * W3
    lk, p_pred, es0 = _three_rank_inputs(d)
    tw = ThreadWorld(W3)
    engines = [pkg.HipEngine(NL3, d, device=0, n_global=n) for _ in range(W3)]
    for r, e in enumerate(engines):
        e.debug_set_local_peers(engines, r, tw.barrier.wait)
    if peer:
        for e in engines:
            e.debug_peer_collectives(True)
    combos = [(halve, first) for halve in (False, True) for first in (True, False) for _ in range(2)]
    res, errs = [[None] * len(combos) for _ in range(W3)], []
    s = pkg.SMCSettings(n_particle=n)

    def work(r):
        try:
            e, sl = engines[r], slice(r * NL3, (r + 1) * NL3)
            comm = PeerComm(tw, r) if peer else tw.comm(r)
            e.upload_particles(pkg.SMC_SET_PRED, p_pred[sl])
            e.upload_lk(pkg.SMC_SET_PRED, lk[sl])
            for k, (halve, first) in enumerate(combos):
                e.upload_particles(pkg.SMC_SET_FILT, -p_pred[sl][::-1].copy())      # recognisable where nobody writes
                e.upload_lk(pkg.SMC_SET_FILT, -lk[sl][::-1].copy() + 0.5)
                es = dict(es0, sum_weight=es0["sum_weight"] * (2.0 if halve else 1.0))
                out = pkg.resample(e, comm, es, U, s, first_step=first)
                res[r][k] = (out["n_offspring"], e.download_offspring(), e.download_particles(pkg.SMC_SET_FILT),
                             e.download_lk(pkg.SMC_SET_FILT))
                comm.barrier()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            tw.barrier.abort()
    ths = [threading.Thread(target=work, args=(r,)) for r in range(W3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for e in engines:
        e.close()
    if errs:
        raise errs[0]
    for k, (halve, first) in enumerate(combos):
        r_is, r_tot, r_f, r_l = _three_rank_oracle(O, d, halve, first)
        what = (d, peer, halve, first, k)
        assert all(res[r][k][0] == r_tot for r in range(W3)), what
        assert np.array_equal(np.concatenate([res[r][k][1] for r in range(W3)]), r_is), what
        assert np.array_equal(np.concatenate([res[r][k][2] for r in range(W3)]), r_f), what
        assert np.array_equal(np.concatenate([res[r][k][3] for r in range(W3)]), r_l), what
        if halve:                      # rank 2 is stale throughout: zeros, or its own PRED rows
            want = np.zeros((NL3, d)) if first else p_pred[2 * NL3:]
            assert np.array_equal(res[2][k][2], want), what
