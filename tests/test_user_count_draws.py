"""Replicated count draws and the PIT of counts on the device (include/smc_hip.h: smc_user_predict_summary with noise = 2,
smc_user_pointwise_summary_opt; csrc/count_draw.h) against the NumPy restatement of the sampler
(tests/count_draw_reference.py) on the device's own predictions.

The integer results are held to the restatement with zero tolerance: with contraction off a last-bit difference between the
device's and the C library's log / exp / lgamma flips a decision only when a comparison falls within that bit, below 1e-9 per
draw at ordinary means; every test here holds fewer than 10^6 draws.  Should a flip ever be met the failing assertion names the
cells (and the PIT test the particles) - then the test's seed is changed and the incident is written into DESIGN.md 4.17; no
tolerance is added.

All models are constant (dy/dt = 0, the outputs are parameters), so the mean of every draw is planted."""
import ctypes
import re

import numpy as np
import pytest

import count_chain as CC
import count_draw_reference as R

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
N_T = 64
T = np.linspace(0.0, 1.0, N_T)[None, :]
PRIOR2 = {"mu": {"dist": "uniform", "low": 0, "high": 1e7}, "b": {"dist": "uniform", "low": 0, "high": 5}}
PROBS = (0.0, 0.01, 0.025, 0.05, 0.1, 0.2, 0.25, 0.4, 0.5, 0.6, 0.75, 0.8, 0.9, 0.95, 0.975, 1.0)
NB_NOISE = {"additive": [("fixed", 1.0)], "proportional": [("param", 1)]}
EDGE_MU = (0.0, 5e-324, 1e-300, float(np.nextafter(10.0, 0.0)), 10.0, float(np.nextafter(10.0, 20.0)), 1e9, 4e15, 2.0 ** 52, np.inf, np.nan, -1.0)
EDGE_B = (0.0, -1.0, np.nan, 1e-4, 10.0)
# two outputs, (theta[0] Gaussian, theta[1] a count), theta = (g, mu, a, b)
MIXED_NOISE = {"additive": [("param", 2), ("fixed", 1.0)], "proportional": [("fixed", 0.0), ("param", 3)]}
PRIOR4 = {"g": {"dist": "uniform", "low": -10, "high": 10}, "mu": {"dist": "uniform", "low": 0, "high": 1e7},
          "a": {"dist": "uniform", "low": 0, "high": 5}, "b": {"dist": "uniform", "low": 0, "high": 5}}


def mixed_source(family):
    return CC.family_line(family) + r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) { dydt[0] = 0.0; }
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) { out[0] = theta[0]; out[1] = theta[1]; }
"""


def _population(n, seed):
    """(mu, b) rows: ordinary ones first (n = 1, 2), then the edge grid - every edge mean beside a valid b (4e15 beside 1e-4, so
    that lam stays about there), every edge b beside an ordinary mean -, then a log-uniform fill.  At most one finite draw of
    the order 4e15 and one of 1e9 per cell: the cell sums stay below 2^53."""
    rs = np.random.RandomState(seed)
    rows = [(4.0, 0.5), (1e4, 2.0)] + [(m, 1e-4 if m == 4e15 else 0.5) for m in EDGE_MU] + [(37.5, b) for b in EDGE_B]
    fill = max(0, n - len(rows))
    mu = np.exp(rs.uniform(np.log(1e-3), np.log(1e7), fill))
    b = np.exp(rs.uniform(np.log(1e-3), np.log(10.0), fill))
    th = np.concatenate([np.array(rows), np.column_stack([mu, b])])[:n]
    return np.ascontiguousarray(th)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cells_of(bad):
    return [tuple(int(x) for x in c) for c in np.argwhere(bad)[:5]]


def _check_draw_summary(out, draws, n, what):
    """out of predictive_summary against the restatement's draws (n, n_ex, n_t, n_obs): the integer results exactly, sd within
    test_user_predictive._check_summary's bound."""
    import warnings
    m = np.isfinite(draws).sum(axis=0)
    assert np.array_equal(out["n_finite"], m), (what, "n_finite differs in cells", _cells_of(out["n_finite"] != m))
    some = m > 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lower = np.nanquantile(draws, PROBS, axis=0, method="lower")
        upper = np.nanquantile(draws, PROBS, axis=0, method="higher")
        total = np.nansum(draws, axis=0)
        sd = np.nanstd(draws, axis=0)
        big = np.maximum(np.nanmax(np.abs(draws), axis=0), 1e-300)
    assert np.all(total < 2.0 ** 53)                                   # integer sums: exact in any order
    for name, ref in (("lower", lower), ("upper", upper)):
        bad = out[name][:, some] != ref[:, some]
        assert not bad.any(), (what, name, "differs in cells", [tuple(np.argwhere(some)[j]) for j in np.argwhere(bad)[:5, 1]])
        assert np.isnan(out[name][:, ~some]).all()
    mean = np.where(some, total / np.maximum(m, 1), np.nan)
    assert np.array_equal(out["mean"][some], mean[some]), (what, "mean differs in cells", _cells_of(some & (out["mean"] != mean)))
    e_sd = np.max(np.abs(out["sd"][some] - sd[some]) / big[some]) if some.any() else 0.0
    print(f"{what}: {int(np.isfinite(draws).sum())} finite draws of {draws.size}, largest {np.nanmax(draws) if some.any() else float('nan'):.4g}, sd off by {e_sd:.3g} (bound {4 * n * EPS:.3g})")
    assert e_sd <= 4 * n * EPS


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2049])
def test_planted_draws_are_the_restatements(pkg, n, family):
    th = _population(n, seed=100 * family + n)
    seed, goff = 11 + n, 1000 * n
    obs = np.full((1, N_T, 1), 3.0)
    with pkg.HipEngine(n, 2, device=0) as eng:
        eng.set_prior(PRIOR2)
        eng.set_model_user(CC.constant_source(family), 1, T, obs, est_sigma=False, noise=None if family == 1 else NB_NOISE)
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        _, pred, _ = eng.predict_user(th)
        out = eng.predictive_summary(pkg.SMC_SET_PRED, probs=PROBS, noise="family", seed=seed, global_offset=goff)
        again = eng.predictive_summary(pkg.SMC_SET_PRED, probs=PROBS, noise="family", seed=seed, global_offset=goff)
        other = eng.predictive_summary(pkg.SMC_SET_PRED, probs=PROBS, noise="family", seed=seed + 1, global_offset=goff)
    assert pred.shape == (n, 1, N_T, 1)
    draws = R.draws_for(seed, goff, n, np.arange(N_T), R.TAG_PREDICT, family, pred[:, 0, :, 0], th[:, 1:2]).reshape(pred.shape)
    _check_draw_summary(out, draws, n, f"family {family}, n = {n}")
    for k in ("mean", "sd", "lower", "upper", "n_finite"):
        assert _bits(out[k], again[k]), k                              # a repeated call: the same bits
    assert not _bits(out["mean"], other["mean"])


def _mixed_data(n_ex=1):
    obs = np.zeros((n_ex, N_T, 2))
    obs[:, :, 0] = 0.3
    obs[:, :, 1] = np.tile(np.array([0.0, 37.0, 1.0, 1e6, 12.0, 38.0, 5.0, 200.0]), N_T // 8)[None, :]
    return obs


def _mixed_population(n, seed, invalid=True):
    rs = np.random.RandomState(seed)
    th = np.column_stack([0.3 + 0.2 * rs.standard_normal(n), np.exp(rs.uniform(np.log(5.0), np.log(200.0), n)), rs.uniform(0.05, 0.5, n),
                          np.exp(rs.uniform(np.log(0.01), np.log(2.0), n))])
    if invalid and n >= 64:
        th[3, 3], th[17, 3], th[40, 3], th[41, 2] = 0.0, -0.5, np.nan, -1.0       # invalid b, and an invalid a beside a valid b
        th[5, 1], th[6, 1], th[7, 1] = np.nan, -2.0, 0.0                          # no prediction, a negative mean, a mean of 0
        th[8, 1], th[9, 1] = 9.99, 10.0
    return np.ascontiguousarray(th)


def test_mixed_model_gaussian_bands_are_noise_trues_and_noise_true_stays_refused(pkg):
    n = 2049
    th = _mixed_population(n, 3, invalid=False)
    obs = _mixed_data()
    got = {}
    with pkg.HipEngine(n, 4, device=0) as eng:
        eng.set_prior(PRIOR4)
        for name, fam in (("gauss", (0, 0)), ("count", (0, 2))):
            eng.set_model_user(mixed_source(fam), 1, T, obs, noise=MIXED_NOISE)
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            kw = {"probs": PROBS, "seed": 5, "global_offset": 77}
            got[name] = {noise: eng.predictive_summary(pkg.SMC_SET_PRED, noise=noise, **kw) for noise in ((False, True, "family") if name == "gauss" else (False, "family"))}
            if name == "count":
                with pytest.raises(pkg.SmcError, match="replicated count draws need a Poisson / gamma sampler on the Philox stream") as e:
                    eng.predictive_summary(pkg.SMC_SET_PRED, noise=True, **kw)
                assert "noise = 2" in str(e.value)
                with pytest.raises(ValueError, match='noise must be False, True or "family"'):
                    eng.predictive_summary(pkg.SMC_SET_PRED, noise="poisson", **kw)
                _, pred, _ = eng.predict_user(th)
    keys = ("mean", "sd", "lower", "upper", "n_finite")
    # a model without counts: "family" is True, bit for bit
    assert all(_bits(got["gauss"]["family"][k], got["gauss"][True][k]) for k in keys)
    # the count model: the Gaussian output's bands are those of the all-zero family list under noise=True ...
    assert all(_bits(got["count"]["family"][k][..., 0], got["gauss"][True][k][..., 0]) for k in keys)
    assert all(_bits(got["count"][False][k], got["gauss"][False][k]) for k in keys)
    # ... and the count output holds counts: the restatement's
    cells = 2 * np.arange(N_T) + 1
    draws = R.draws_for(5, 77, n, cells, R.TAG_PREDICT, 2, pred[:, 0, :, 1], th[:, 3:4])
    c = got["count"]["family"]
    assert np.array_equal(c["n_finite"][0, :, 1], np.isfinite(draws).sum(axis=0))
    assert np.array_equal(c["lower"][:, 0, :, 1], np.nanquantile(draws, PROBS, axis=0, method="lower"))
    assert np.array_equal(c["upper"][:, 0, :, 1], np.nanquantile(draws, PROBS, axis=0, method="higher"))
    assert np.array_equal(c["mean"][0, :, 1], draws.sum(axis=0) / n)
    assert np.all(c["sd"][0, :, 1] > got["count"][False]["sd"][0, :, 1])      # the band of the data is wider than the band of the mean


def _abc(pkg, eng, family):
    t, obs = CC.make_data(0, b=0.0 if family == 1 else CC.B_TRUE)
    eng.set_prior({nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(CC.NAMES, CC.PRIOR_HIGH)})
    eng.set_model_user(CC.source((0, family)), 2, t, obs, cond=CC.COND, noise=CC.NOISE_POISSON if family == 1 else CC.NOISE_NB)
    return t, obs


def _abc_population(n, seed):
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray(CC.THETA_TRUE * np.exp(0.1 * rs.standard_normal((n, 4))))


@pytest.mark.parametrize("family", [1, 2])
def test_staging_groups_cannot_change_a_draw(pkg, family):
    """A -> B -> C with counts, 4 experiments: room for one experiment at a time returns the bits of one group, for the bands of
    replicated observations and for the PIT counts."""
    n = 3000
    th = _abc_population(n, 8)
    with pkg.HipEngine(n, 4, device=0) as eng:
        _abc(pkg, eng, family)
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        kw = {"probs": (0.05, 0.5, 0.95), "noise": "family", "seed": 9, "global_offset": 12345}
        one = eng.predictive_summary(pkg.SMC_SET_PRED, **kw)
        with pytest.raises(pkg.SmcError, match=r"one experiment of the design needs \d+ B of staging") as e:
            eng.predictive_summary(pkg.SMC_SET_PRED, max_staging_bytes=1, **kw)
        need = int(re.search(r"needs (\d+) B", str(e.value)).group(1))
        grouped = eng.predictive_summary(pkg.SMC_SET_PRED, max_staging_bytes=need, **kw)
        for k in ("mean", "sd", "lower", "upper", "n_finite"):
            assert _bits(one[k], grouped[k]), k
        assert np.all(one["n_finite"][:, 0, :] == n)
        counts = one["mean"][..., 1][np.isfinite(one["mean"][..., 1])]
        assert counts.size > 80 and np.all(one["lower"][..., 1][np.isfinite(one["lower"][..., 1])] % 1 == 0)
        pw = eng.pointwise_summary(pkg.SMC_SET_PRED, count_pit=True, seed=9, global_offset=12345)
        with pytest.raises(pkg.SmcError, match=r"one experiment of the design needs \d+ B of staging") as e:
            eng.pointwise_summary(pkg.SMC_SET_PRED, max_staging_bytes=1, count_pit=True, seed=9, global_offset=12345)
        need = int(re.search(r"needs (\d+) B", str(e.value)).group(1))
        pw1 = eng.pointwise_summary(pkg.SMC_SET_PRED, max_staging_bytes=need, count_pit=True, seed=9, global_offset=12345)
        for k in ("n", "max", "sum_exp", "mean", "m2", "pit", "pit_below", "pit_equal", "pit_n", "pit_lower", "pit_upper"):
            assert _bits(pw[k], pw1[k]), k
        assert pw["pit_n"][..., 1].max() == n and pw["pit_n"][..., 0].max() == 0


def _pit_reference(pred, obs, th, seed, goff, observed=None):
    """(below, equal, n) of the mixed model's count output from the restatement: pred (n, 1, n_t, 2), theta = (g, mu, a, b)."""
    n = pred.shape[0]
    f, y = pred[:, 0, :, 1], obs[0, :, 1]
    valid = (th[:, 2] > 0.0) & (th[:, 3] > 0.0)                         # a_k > 0 everywhere, b_k > 0 on the negative-binomial output
    use = np.isfinite(f) & valid[:, None] & np.isfinite(y)[None, :]
    draws = R.draws_for(seed, goff, n, 2 * np.arange(N_T) + 1, R.TAG_PIT, 2, f, th[:, 3:4])
    with np.errstate(invalid="ignore"):
        return (use & (draws < y[None, :])), (use & (draws == y[None, :])), use


@pytest.mark.parametrize("n", [1, 64, 65, 2049])
def test_count_pit_counts_are_the_restatements(pkg, n):
    th = _mixed_population(n, 20 + n)
    obs = _mixed_data()
    obs[0, 5, 1] = np.nan                                               # a count that was not measured
    obs[0, 10, 0] = np.nan
    censor = np.zeros(obs.shape, dtype=np.int8)
    censor[0, 2::7, 0] = -1
    censor[0, 4::9, 0] = 1
    seed, goff = 31 + n, 500 + n
    i64p, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    with pkg.HipEngine(n, 4, device=0) as eng:
        eng.set_prior(PRIOR4)
        eng.set_model_user(mixed_source((0, 2)), 1, T, obs, noise=MIXED_NOISE, censor=censor)
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        _, pred, _ = eng.predict_user(th)
        old = eng.pointwise_summary()
        got = eng.pointwise_summary(count_pit=True, seed=seed, global_offset=goff)
        # the new entry point with the option off, and with no options: the old entry point's bits
        raw = {}
        for label, opts in (("off", pkg.binding.PointwiseOpts(count_pit=0, seed=seed, global_offset=goff)), ("null", None)):
            nn = np.empty(obs.shape, dtype=np.int64)
            a = [np.empty(obs.shape) for _ in range(5)]
            rc = eng.L.smc_user_pointwise_summary_opt(eng.ctx, pkg.SMC_SET_FILT, 0, None if opts is None else ctypes.byref(opts), nn.ctypes.data_as(i64p),
                                                      *[x.ctypes.data_as(dp) for x in a], None, None, None)
            assert rc == 0, eng.L.smc_last_error(eng.ctx)
            raw[label] = [nn.astype(np.float64)] + a
        bad = pkg.binding.PointwiseOpts(count_pit=1, seed=seed, global_offset=goff)
        assert eng.L.smc_user_pointwise_summary_opt(eng.ctx, pkg.SMC_SET_FILT, 0, ctypes.byref(bad), nn.ctypes.data_as(i64p),
                                                    *[x.ctypes.data_as(dp) for x in a], None, None, None) != 0
        assert "count_pit with a NULL pit_below" in eng.L.smc_last_error(eng.ctx).decode()
    for label in raw:
        for k, x in zip(("n", "max", "sum_exp", "mean", "m2", "pit"), raw[label]):
            assert _bits(x, old[k]), (label, k)
    for k in ("n", "max", "sum_exp", "mean", "m2", "lpd", "var"):
        assert _bits(got[k], old[k]), k
    assert _bits(got["pit"][..., 0], old["pit"][..., 0]) and np.all(np.isnan(old["pit"][..., 1]))
    below, equal, use = _pit_reference(pred, obs, th, seed, goff)
    for name, ref in (("pit_below", below), ("pit_equal", equal), ("pit_n", use)):
        diff = got[name][0, :, 1] != ref.sum(axis=0)
        where = [(int(c), [int(p) for p in np.flatnonzero(use[:, c])[:8]]) for c in np.flatnonzero(diff)[:4]]
        assert not diff.any(), (name, "differs in (time, candidate particles)", where)
        assert got[name].dtype == np.int64 and np.all(got[name][..., 0] == 0)
    assert got["pit_n"][0, 5, 1] == 0 and np.isnan(got["pit"][0, 5, 1])
    nv = int(((th[:, 2] > 0) & (th[:, 3] > 0) & np.isfinite(th[:, 1])).sum())
    assert np.all(np.delete(got["pit_n"][0, :, 1], 5) == nv)
    um = pkg.user_models
    assert np.array_equal(got["pit"][..., 1], um.count_pit(got["pit_below"], got["pit_equal"], got["pit_n"], seed)[..., 1], equal_nan=True)
    assert np.array_equal(got["pit_lower"][..., 0], old["pit"][..., 0], equal_nan=True)
    if n >= 64:      # the observations at 0 and far in the tails: nothing below 0, (nearly) everything below 10^6
        y = obs[0, :, 1]
        assert np.all(got["pit_below"][0, y == 0.0, 1] == 0) and np.all(got["pit_below"][0, y == 1e6, 1] >= nv - 1)
        mid = got["pit_lower"][0, y == 37.0, 1]
        assert np.all((mid > 0.05) & (mid < 0.95))
        print(f"n = {n}: {nv} particles count, {int(use.sum())} draws, PIT of y = 37 about {mid.mean():.3f}")


def test_shards_add_up_to_the_whole(pkg):
    """Two engines hold the halves of one population under global offsets 0 and n / 2: against one engine with all of it the PIT
    counts add up exactly, and so do the sums mean x n_finite of the replicated bands."""
    n = 4096
    th = _mixed_population(n, 77)
    obs = _mixed_data()
    seed, goff = 21, 10 ** 6

    def run(part, offset):
        with pkg.HipEngine(part.shape[0], 4, device=0, n_global=n) as eng:
            eng.set_prior(PRIOR4)
            eng.set_model_user(mixed_source((0, 2)), 1, T, obs, noise=MIXED_NOISE)
            eng.upload_particles(pkg.SMC_SET_PRED, np.ascontiguousarray(part))
            return (eng.pointwise_summary(pkg.SMC_SET_PRED, count_pit=True, seed=seed, global_offset=goff + offset),
                    eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.0, 0.5, 1.0), noise="family", seed=seed, global_offset=goff + offset))
    whole, band = run(th, 0)
    halves = [run(th[:n // 2], 0), run(th[n // 2:], n // 2)]
    for k in ("pit_below", "pit_equal", "pit_n"):
        assert np.array_equal(whole[k], halves[0][0][k] + halves[1][0][k]), k
    assert whole["pit_n"][0, :, 1].min() > n - 20
    merged = pkg.user_models.pointwise_merge([h[0] for h in halves])
    assert all(np.array_equal(merged[k], whole[k]) for k in ("n", "pit_below", "pit_equal", "pit_n"))
    total = np.rint(band["mean"][..., 1] * band["n_finite"][..., 1])
    parts = sum(np.rint(h[1]["mean"][..., 1] * h[1]["n_finite"][..., 1]) for h in halves)
    assert np.array_equal(total, parts) and np.all(total < 2.0 ** 50)
    assert np.array_equal(band["n_finite"], halves[0][1]["n_finite"] + halves[1][1]["n_finite"])
    assert np.array_equal(band["lower"][0], np.minimum(halves[0][1]["lower"][0], halves[1][1]["lower"][0]))
    assert np.array_equal(band["upper"][2], np.maximum(halves[0][1]["upper"][2], halves[1][1]["upper"][2]))


def test_closed_form_of_identical_poisson_particles(pkg):
    """65 536 identical particles, Poisson with mean 7.3: pit_lower within 5 x 0.5 / sqrt n of poisson.cdf(y - 1) (a binomial
    share: sd <= 0.5 / sqrt n), and the 5 % / 95 % order statistics of the replicated band are poisson.ppf or its neighbour."""
    from scipy.stats import poisson
    n, mu = 65536, 7.3
    th = np.ascontiguousarray(np.column_stack([np.full(n, mu), np.full(n, 0.5)]))
    y = np.tile(np.array([0.0, 3.0, 7.0, 8.0, 12.0, 20.0, 5.0, 10.0]), N_T // 8)
    with pkg.HipEngine(n, 2, device=0) as eng:
        eng.set_prior(PRIOR2)
        eng.set_model_user(CC.constant_source(1), 1, T, y[None, :, None], est_sigma=False)
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        pw = eng.pointwise_summary(count_pit=True, seed=2, global_offset=0)
        band = eng.predictive_summary(probs=(0.05, 0.95), noise="family", seed=2, global_offset=0)
    assert np.all(pw["pit_n"] == n)
    d_lo = pw["pit_lower"][0, :, 0] - poisson.cdf(y - 1, mu)
    d_up = pw["pit_upper"][0, :, 0] - poisson.cdf(y, mu)
    print(f"pit_lower off by {np.abs(d_lo).max():.3g}, pit_upper by {np.abs(d_up).max():.3g} (bound {2.5 / np.sqrt(n):.3g})")
    assert np.abs(d_lo).max() <= 5 * 0.5 / np.sqrt(n) and np.abs(d_up).max() <= 5 * 0.5 / np.sqrt(n)
    for j, p in enumerate((0.05, 0.95)):
        q = poisson.ppf(p, mu)
        for name in ("lower", "upper"):
            assert np.all(np.abs(band[name][j, 0, :, 0] - q) <= 1), (p, name)
    assert abs(band["mean"].mean() - mu) <= 5 * np.sqrt(mu / (n * N_T)) and np.all(np.abs(band["sd"] - np.sqrt(mu)) < 0.05)
    assert 0.3 < pw["pit"].mean() < 0.7
