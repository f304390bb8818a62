"""Censored observations of a user model (include/smc_hip.h: smc_set_model_user7; csrc/user_censor.h and the SMC_USER_CENSOR
blocks of csrc/user_obs_args.h; user_models.censor_layout, censored_loglik, censor_data; HipEngine.set_model_user(censor=)).
Data, planted records and the reference chain live in tests/censored_chain.py.

CPU part: censored_loglik against a plain triple loop over scipy's log_ndtr and norm.logpdf on planted records; the excess
formula on a grid over [-1e154, 40]; every refusal of the flags' rules in NumPy and through smc_user_censor_check, in the same
words; the censored sources compile for gfx950 in the four variants; dump_source7 without the switch writes dump_source6's
files.

GPU part: the likelihood of a sweep is predict_user's bit for bit and censored_loglik of the engine's own predictions (RK45
and BDF, far tails, invalid particles); Phi(z) + Phi(-z) = 1 through three models; all-zero flags change no bit; noise=None is
the equivalent specification; a Metropolis sweep bit for bit with and without early rejection; with events and with inputs; a
full run against a Metropolis chain on the closed form, and nearer to it than the run with the censored values dropped; the LDS
refusal with an odd n_obs.

Measured on an MI355X: |lk - censored_loglik(pred)| / max(1, |lk|) at most 9.5e-16 (RK45 and BDF, both noise variants, lk
down to -1.5e12 from the tiny additive levels), 3.2e-15 with events and inputs; complementarity 3.8e-14 with Phi(z) from 7e-18
to 1; noise=None against the explicit specification 0; a sweep of 4096 proposals in 190 420 attempts with early rejection,
191 086 without; the full run's means within 0.09 chain sd, sd ratios 0.99 ... 1.04, k2 0.29738 (chain 0.29755) against 0.29686
with the censored values dropped (that chain: 0.29687)."""
import ctypes
import filecmp
import os

import numpy as np
import pytest

import censored_chain as CC
import dosed_model as DM
import forced_linear_model as FM
import noise_model_chain as NC

RK45, BDF = 0, 1
NAMES = ("k1", "k2", "a0", "a1", "b0")
PRIORS = {nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(NAMES, NC.PRIOR_HIGH)}
ADD_ONLY = {"additive": NC.NOISE["additive"]}
# the reference posterior for data seed 0 and the lower limit 0.25 on B: `python tests/censored_chain.py 0 250000` (acceptance
# 0.271; the means of the two half chains differ by at most 0.03 sd).  The chain with the censored values DROPPED (NaN) has the
# k2 mean 0.29687, 0.35 chain sd below the censored one: limits 0.15 and 0.4 separate the two by less (0.12 and 0.17 sd).
CHAIN_MEAN = np.array([0.7923, 0.29755, 0.01139, 0.02126, 0.07781])
CHAIN_SD = np.array([0.00647, 0.00196, 0.00107, 0.00201, 0.01283])
DROPPED_K2 = 0.29687


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _bar(lk, ref):
    return np.max(np.abs(lk - ref) / np.maximum(1.0, np.abs(ref)))


def _planted(pkg, seed=0):
    """The noise tests' data censored on both sides at the 30 % and 70 % quantiles, the records of CC.plant on top."""
    t, values, lower, upper = CC.two_sided(seed)
    obs, censor = pkg.user_models.censor_data(values, lower, upper)
    obs, censor = CC.plant(obs, censor)
    return t, obs, censor


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_censor_data_writes_the_limit_and_the_flag(pkg):
    v = np.array([[[0.1, 5.0], [0.5, np.nan], [0.9, 0.2], [np.nan, 3.0]]])
    obs, c = pkg.user_models.censor_data(v, lower=[0.3, np.nan], upper=[0.8, 2.5])
    assert np.array_equal(obs, np.array([[[0.3, 2.5], [0.5, np.nan], [0.8, 0.2], [np.nan, 2.5]]]), equal_nan=True)
    assert c.dtype == np.int8 and c.tolist() == [[[-1, 1], [0, 0], [1, 0], [0, 1]]]
    obs2, c2 = pkg.user_models.censor_data(v)
    assert np.array_equal(obs2, v, equal_nan=True) and not c2.any()
    t, values, lower, upper = CC.two_sided(0)
    _, c = pkg.user_models.censor_data(values, lower, upper)
    seen = ~np.isnan(values)
    for side in (-1, 1):
        assert 0.2 <= np.sum(c == side) / seen.sum() <= 0.4


def test_censored_loglik_agrees_with_a_plain_triple_loop(pkg):
    from scipy.special import log_ndtr
    from scipy.stats import norm
    um = pkg.user_models
    t, obs, censor = _planted(pkg, 11)
    lay = um.censor_layout(t, obs, censor)
    assert lay["quantified"][3].sum() == 0 and lay["censored"][3].sum() > 20          # an experiment with m_e = 0
    assert lay["quantified"][2, 1] == 0 and lay["censored"][2, 1] == 18              # an output censored everywhere
    assert (censor == -1).sum() > 30 and (censor == 1).sum() > 30
    rs = np.random.RandomState(11)
    n = 7
    theta = np.column_stack([rs.uniform(0.1, 2, n), rs.uniform(0.05, 1, n), rs.uniform(0.005, 0.05, n), rs.uniform(0.005, 0.05, n),
                             rs.uniform(0.0, 0.3, n)])
    pred = np.stack([NC.closed_form(k1, k2, t) for k1, k2 in theta[:, :2]])
    scale = np.array([1.0, 3.0])
    for noise in (NC.NOISE, ADD_ONLY):
        lk = um.censored_loglik(pred, t, obs, censor, theta, noise, obs_scale=scale)
        ref = np.zeros(n)
        terms = 0
        for p, th in enumerate(theta):
            a, b = (th[2], th[3]), (th[4] if "proportional" in noise else 0.0, 0.0)
            for e in range(t.shape[0]):
                for i in range(t.shape[1]):
                    if np.isnan(t[e, i]):
                        continue
                    for k in range(2):
                        if np.isnan(obs[e, i, k]):
                            continue
                        terms += p == 0
                        f = pred[p, e, i, k]
                        sd = np.sqrt((a[k] * scale[k]) ** 2 + (b[k] * f) ** 2)
                        if censor[e, i, k] == 0:
                            ref[p] += norm.logpdf(obs[e, i, k], loc=f, scale=sd)
                        elif censor[e, i, k] < 0:
                            ref[p] += log_ndtr((obs[e, i, k] - f) / sd)
                        else:
                            ref[p] += log_ndtr((f - obs[e, i, k]) / sd)
        assert 150 < terms < 4 * 30 * 2 - 24
        err = _bar(lk, ref)
        print(f"worst |censored_loglik - loop| / max(1, |lk|) = {err:.3g} over {terms} terms")
        assert np.all(np.isfinite(ref)) and err <= 1e-12
    zero = np.zeros_like(censor)
    assert np.array_equal(um.censored_loglik(pred, t, obs, zero, theta, NC.NOISE, obs_scale=scale),
                          um.noise_loglik(pred, t, obs, theta, NC.NOISE, obs_scale=scale))
    bad = theta.copy()
    bad[0, 2], bad[1, 3], bad[2, 4] = 0.0, -0.01, -1e-9
    lk = um.censored_loglik(pred, t, obs, censor, bad, NC.NOISE)
    assert np.isneginf(lk[:3]).all() and np.isfinite(lk[3:]).all()


def _grid():
    tiny = np.array([5e-324, 2.2250738585072014e-308, 1e-300])
    z = np.concatenate([-np.logspace(-290, 154, 889), -tiny, [-0.0, 0.0], tiny, np.logspace(-290, 0, 59), np.linspace(-40.0, 40.0, 1601),
                        [-1e154, 40.0]])
    return np.unique(z)         # sorted; -0.0 and 0.0 compare equal and one of them stays


def test_the_excess_is_non_negative_finite_and_monotone(pkg):
    from scipy.special import log_ndtr
    z = _grid()
    assert z[0] == -1e154 and z[-1] == 40.0 and np.any(z == 0.0) and np.any(np.abs(z) == 5e-324)
    x = pkg.user_models.censor_excess(z)
    assert np.all(x >= 0.0) and np.all(np.isfinite(x)) and np.all(np.diff(x) <= 0.0)
    assert np.array_equal(pkg.user_models.censor_excess(np.array([-0.0, 0.0])), np.full(2, x[z == 0.0][0])) and abs(x[z == 0.0][0] - np.log(2.0)) < 1e-15
    assert np.all(pkg.user_models.censor_excess(np.array([40.0, 41.0, 1e3, np.inf])) == 0.0)
    assert np.isnan(pkg.user_models.censor_excess(np.array([np.nan]))[0])
    m = (z >= -38.0) & (z <= 8.3)
    err = np.max(np.abs(x[m] + log_ndtr(z[m])) / np.abs(log_ndtr(z[m])))
    print(f"worst relative distance to -log_ndtr over [-38, 8.3]: {err:.3g}")
    assert err <= 1.5e-14


def _refusals():
    """(t, obs, censor, the reason without its prefix)"""
    t, obs = NC.make_data(0)
    obs[1, 4, 1] = np.nan
    good = np.zeros(obs.shape, dtype=np.int8)
    good[0, 2, 0], good[3, 7, 1] = -1, 1
    out = []
    out.append((t, obs, good[:, :, :1].copy(), "censor must have the shape of obs (4, 30, 2), got (4, 30, 1)"))
    out.append((t, obs, good[:, :29].copy(), "censor must have the shape of obs (4, 30, 2), got (4, 29, 2)"))
    c = good.copy(); c[1, 3, 1] = 2
    out.append((t, obs, c, "censor holds the flag 2 at row 1, time 3, output 1 (0: measured, -1: at or below obs, +1: at or above obs)"))
    c = good.copy(); c[0, 0, 0] = -2
    out.append((t, obs, c, "censor holds the flag -2 at row 0, time 0, output 0"))
    c = good.copy(); c[1, 4, 1] = -1
    out.append((t, obs, c, "censor flags a value that was not measured (obs is NaN) at row 1, time 4, output 1"))
    c = good.copy(); c[2, 18, 0] = 1
    out.append((t, obs, c, "censor flags a value past the end of its row at row 2, time 18, output 0"))
    return out, good


def _c_check(L, t, obs, c):
    t, obs, c = np.ascontiguousarray(t), np.ascontiguousarray(obs), np.ascontiguousarray(c, dtype=np.int8)
    return L.smc_user_censor_check(_dp(t), _dp(obs), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), *obs.shape, *c.shape)


@pytest.mark.parametrize("k", range(6))
def test_refused_flags_are_refused_in_the_same_words_by_numpy_and_the_library(pkg, k):
    t, obs, c, why = _refusals()[0][k]
    with pytest.raises(ValueError) as e:
        pkg.user_models.censor_layout(t, obs, c)
    assert str(e.value).startswith("censor_layout: " + why), str(e.value)
    L = pkg.lib()
    assert _c_check(L, t, obs, c) != 0
    msg = L.smc_last_error(None).decode()
    assert msg.startswith("smc_user_censor_check: " + why), msg


def test_accepted_flags_and_their_counts(pkg):
    cases, good = _refusals()
    t, obs = cases[0][0], cases[0][1]
    lay = pkg.user_models.censor_layout(t, obs, good)
    assert _c_check(pkg.lib(), t, obs, good) == 0
    seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
    assert np.array_equal(lay["quantified"] + lay["censored"], seen.sum(axis=1))
    assert lay["censored"].tolist() == [[1, 0], [0, 0], [0, 0], [0, 1]]
    assert lay["quantified"].sum() == pkg.user_models.obs_layout(t, obs)["m_e"].sum() - 2


def test_censored_sources_compile_in_the_four_variants(pkg):
    um, L = pkg.user_models, pkg.lib()
    for method in (RK45, BDF):
        for noise in (1, 2):
            log = ctypes.create_string_buffer(16384)
            rc = L.smc_user_model_check7(um.CONSECUTIVE_REACTIONS_AB.encode(), 2, 5, method, 2, noise, 1, 0, 0, 0, 0, 1, log, 16384)
            assert rc == 0, (method, noise, log.value.decode(errors="replace"))
    log = ctypes.create_string_buffer(16384)      # an odd n_obs (the record grows), and together with events
    assert L.smc_user_model_check7(um.CONSECUTIVE_REACTIONS_ABC.encode(), 2, 5, RK45, 3, 2, 1, 0, 0, 0, 0, 1, log, 16384) == 0, log.value
    assert L.smc_user_model_check7(um.ONE_COMPARTMENT_DOSED.encode(), 1, 2, RK45, 1, 1, 1, 0, 0, 5, 1, 1, log, 16384) == 0, log.value
    # censoring without a noise model does not exist
    assert L.smc_user_model_check7(um.CONSECUTIVE_REACTIONS_AB.encode(), 2, 5, RK45, 2, 0, 1, 0, 0, 0, 0, 1, log, 16384) == 2


def test_dump_source7_without_the_switch_writes_dump_source6s_files(pkg, tmp_path):
    um, L = pkg.user_models, pkg.lib()
    for j, (src, ns, dim, method, n_obs, noise, n_ev, n_val) in enumerate([
            (um.CONSECUTIVE_REACTIONS_AB, 2, 5, RK45, 2, 1, 0, 0), (um.CONSECUTIVE_REACTIONS_AB, 2, 5, BDF, 2, 2, 0, 0),
            (um.CONSECUTIVE_REACTIONS_AB, 2, 5, RK45, 2, 0, 0, 0), (um.ONE_COMPARTMENT_DOSED, 1, 2, RK45, 1, 1, 5, 1)]):
        d6, d7, dc = tmp_path / f"six{j}", tmp_path / f"seven{j}", tmp_path / f"cens{j}"
        for d in (d6, d7, dc):
            d.mkdir()
        assert L.smc_user_model_dump_source6(src.encode(), ns, dim, method, n_obs, noise, 1, 0, 0, n_ev, n_val, str(d6).encode()) == 0
        assert L.smc_user_model_dump_source7(src.encode(), ns, dim, method, n_obs, noise, 1, 0, 0, n_ev, n_val, 0, str(d7).encode()) == 0
        names = sorted(os.listdir(d6))
        assert sorted(os.listdir(d7)) == names
        match, mismatch, errors = filecmp.cmpfiles(d6, d7, names, shallow=False)
        assert sorted(match) == names and not mismatch and not errors
        if noise:
            assert L.smc_user_model_dump_source7(src.encode(), ns, dim, method, n_obs, noise, 1, 0, 0, n_ev, n_val, 1, str(dc).encode()) == 0
            assert sorted(os.listdir(dc)) == sorted(names + ["user_censor.h"])
            head = (dc / "smc_user_model.hip").read_text()[:600]
            assert "#define SMC_USER_CENSOR 1\n" in head and "SMC_USER_CENSOR" not in (d7 / "smc_user_model.hip").read_text()
            assert "SMC_USER_CENSOR" not in (d7 / "user_obs_args.h").read_text() and "SMC_USER_CENSOR" in (dc / "user_obs_args.h").read_text()


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _population(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([NC.K_TRUE[0] * (1 + 0.1 * rs.standard_normal(n)), NC.K_TRUE[1] * (1 + 0.1 * rs.standard_normal(n)),
                            rs.uniform(0.005, 0.03, n), rs.uniform(0.01, 0.05, n), rs.uniform(0.02, 0.2, n)])


def _tailed_population(n, seed):
    """_population with the invalid particles of the noise test in front (a <= 0, b < 0, NaN) and a few with a tiny additive level,
    where |z| reaches the far tails (|z| up to about 1e5: x = z^2 / 2 on one side, 0 on the other)."""
    th = _population(n, seed)
    th[0, 2], th[1, 3], th[2, 4], th[3, 2] = 0.0, -0.01, -1e-6, np.nan
    th[4:8, 2] = (1e-5, 3e-4, 1e-6, 2e-3)
    th[6:10, 3] = (1e-5, 1e-6, 4e-4, 1e-3)
    th[4:10, 4] = (0.0, 1e-7, 1e-4, 0.0, 1e-3, 0.0)
    return th


def _sweep(pkg, eng, th):
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    return eng.download_lk(pkg.SMC_SET_PRED), info


def test_censored_loglik_is_finite_for_every_valid_particle_of_the_gpu_population(pkg):
    t, obs, censor = _planted(pkg)
    th = _tailed_population(512, 1)
    pred = np.stack([NC.closed_form(k1, k2, t) for k1, k2 in th[:, :2]])
    for noise in (NC.NOISE, ADD_ONLY):
        lk = pkg.user_models.censored_loglik(pred, t, obs, censor, th, noise, obs_scale=(1.0, 3.0))
        assert np.isneginf(lk[:2]).all() and np.isfinite(lk[4:]).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.abs(obs[None] - pred) / np.sqrt(th[:, None, None, 2:4] ** 2)
    assert np.nanmax(np.where(censor[None] != 0, z, 0.0)[4:]) > 1e4       # the far tails are reached


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [ADD_ONLY, NC.NOISE], ids=["additive", "combined"])
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_likelihood_is_censored_loglik_of_the_engines_own_predictions(pkg, method, noise):
    t, obs, censor = _planted(pkg)
    n = 512
    th = _tailed_population(n, 1)
    scale = (1.0, 3.0)
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], method=method, obs_scale=scale,
                           noise=noise, censor=censor)
        lk, info = _sweep(pkg, eng, th)
        lk_p, pred, pinfo = eng.predict_user(th)
    assert info["n_failed"] == 0 and pinfo["n_failed"] == 0 and info["rk_attempts"] == pinfo["rk_attempts"]
    assert np.array_equal(lk, lk_p)
    bad = 3 if "proportional" in noise else 2             # b < 0 is a rule of the proportional part only
    assert np.isneginf(lk[:2]).all() and (bad == 2 or np.isneginf(lk[2])) and not np.isfinite(lk[3]) and np.isfinite(lk[4:]).all()
    ref = pkg.user_models.censored_loglik(pred, t, obs, censor, th, noise, obs_scale=scale)
    assert np.isfinite(ref[4:]).all()
    err = _bar(lk[4:], ref[4:])
    print(f"{method}: worst |lk - censored_loglik(pred)| / max(1, |lk|) = {err:.3g}; lk from {lk[4:].min():.4g} to {lk[4:].max():.4g}")
    assert err <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [ADD_ONLY, NC.NOISE], ids=["additive", "combined"])
def test_left_and_right_censoring_at_one_limit_are_complementary(pkg, noise):
    """One value censored at L from the left, the same from the right, and dropped (base): Phi(z) + Phi(-z) = 1."""
    t, obs = NC.make_data(0)
    n = 512
    th = _population(n, 4)
    e, i, k = 1, 9, 1
    assert np.isfinite(obs[e, i, k])
    lk = {}
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        for side in (-1, 1, 0):
            o, c = obs.copy(), np.zeros(obs.shape, dtype=np.int8)
            c[e, i, k] = side
            if side == 0:
                o[e, i, k] = np.nan
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, o, cond=NC.A0[:, None], noise=noise, censor=c)
            lk[side], info = _sweep(pkg, eng, th)
            assert info["n_failed"] == 0
    base = lk[0]
    total = np.exp(lk[-1] - base) + np.exp(lk[1] - base)
    worst = np.max(np.abs(total - 1.0) / np.maximum(1.0, np.abs(base)))
    left = np.exp(lk[-1] - base)
    print(f"worst |Phi(z) + Phi(-z) - 1| / max(1, |base|) = {worst:.3g}; Phi(z) from {left.min():.3g} to {left.max():.3g}")
    assert 0.0 < left.min() < 0.3 and 0.7 < left.max() <= 1.0            # both sides of the limit occur
    assert np.all(np.abs(total - 1.0) <= 4e-9 * np.maximum(1.0, np.abs(base)))


@pytest.mark.gpu
def test_all_zero_flags_change_no_bit_and_noise_none_is_the_equivalent_specification(pkg):
    t, obs = NC.make_data(0)
    n = 512
    src = pkg.user_models.CONSECUTIVE_REACTIONS_AB
    th = _population(n, 2)
    th[:, 4] = th[:, 2]                                          # sigma, the last parameter
    zero = np.zeros(obs.shape, dtype=np.int8)
    kw = dict(cond=NC.A0[:, None])
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        for more in ({}, {"noise": NC.NOISE, "obs_scale": (1.0, 3.0)}):
            eng.set_model_user(src, 2, t, obs, **kw, **more)
            lk_a, info_a = _sweep(pkg, eng, th)
            pa = eng.predict_user(th)
            eng.set_model_user(src, 2, t, obs, censor=zero, **kw, **more)
            lk_b, info_b = _sweep(pkg, eng, th)
            pb = eng.predict_user(th)
            assert np.array_equal(lk_a, lk_b) and info_a == info_b and np.all(np.isfinite(lk_a))
            assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1], equal_nan=True) and pa[2] == pb[2]
        _, _, lower, upper = CC.two_sided(0)
        o, c = pkg.user_models.censor_data(np.where(np.isnan(t)[:, :, None], np.nan, obs), lower, upper)
        eng.set_model_user(src, 2, t, o, censor=c, **kw)                                     # est_sigma: every output at dim - 1
        lk_n, info_n = _sweep(pkg, eng, th)
        eng.set_model_user(src, 2, t, o, censor=c, noise={"additive": [("param", 4), ("param", 4)]}, **kw)
        lk_e, info_e = _sweep(pkg, eng, th)
        _, pred, _ = eng.predict_user(th)
        eng.set_model_user(src, 2, t, o, censor=c, est_sigma=False, sigma_fixed=0.02, **kw)
        lk_f, _ = _sweep(pkg, eng, th)
        eng.set_model_user(src, 2, t, o, censor=c, noise={"additive": [("fixed", 0.02), ("fixed", 0.02)]}, **kw)
        lk_g, _ = _sweep(pkg, eng, th)
    print(f"noise=None against the explicit specification: {_bar(lk_n, lk_e):.3g} (est_sigma), {_bar(lk_f, lk_g):.3g} (sigma_fixed)")
    assert info_n == info_e and _bar(lk_n, lk_e) <= 1e-9 and _bar(lk_f, lk_g) <= 1e-9
    ref = pkg.user_models.censored_loglik(pred, t, o, c, th, {"additive": [("param", 4), ("param", 4)]})
    assert _bar(lk_n, ref) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [ADD_ONLY, NC.NOISE], ids=["additive", "combined"])
def test_early_rejection_is_exact_and_saves_attempts_on_censored_data(pkg, noise):
    """The noise test's sweep on censored data; start rejection stays at its default throughout."""
    t, values, lower, upper = CC.two_sided(3)
    obs, censor = pkg.user_models.censor_data(values, lower, upper)
    n = 4096
    th = _population(n, 7)
    out = []
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], noise=noise, censor=censor)
        lk, info = _sweep(pkg, eng, th)
        assert info["n_failed"] == 0 and np.all(np.isfinite(lk))
        for on in (False, True):
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_lk(pkg.SMC_SET_FILT, lk)
            eng.set_early_reject(on)
            mh = eng.mh_step_device_rng(0.5, 1.0, np.diag([0.004, 0.004, 2e-5, 2e-5, 1e-3]), 7, 3)
            out.append((mh, eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags()))
    (m0, p0, l0, a0), (m1, p1, l1, a1) = out
    print(f"accepted {m0['accepted_now']} of {n}; attempts {m0['rk_attempts']} without, {m1['rk_attempts']} with early rejection")
    assert m0["n_failed"] == 0 and m1["n_failed"] == 0 and 0 < m0["accepted_now"] < n
    assert m0["accepted_now"] == m1["accepted_now"] and np.array_equal(a0, a1) and np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert m1["rk_attempts"] < m0["rk_attempts"]


def _check_against_definition(pkg, eng, th, t, obs, censor, noise, what):
    lk, info = _sweep(pkg, eng, th)
    lk_p, pred, pinfo = eng.predict_user(th)
    assert info["n_failed"] == 0 and pinfo["n_failed"] == 0
    assert np.array_equal(lk, lk_p)
    ref = pkg.user_models.censored_loglik(pred, t, obs, censor, th, noise)
    assert np.all(np.isfinite(ref))
    err = _bar(lk, ref)
    print(f"{what}: worst |lk - censored_loglik(pred)| / max(1, |lk|) = {err:.3g}")
    assert err <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["E1", "E4"])
def test_flags_survive_the_event_restart(pkg, cid):
    """The dosed one-compartment model (E1; E4: with a measured input as well) with a lower limit that censors the troughs."""
    c = DM.CASES[cid]
    t, values, _ = DM.make_data(cid)
    limit = np.nanquantile(values, 0.35)
    obs, censor = pkg.user_models.censor_data(values, lower=limit)
    assert 0.25 <= (censor != 0).sum() / np.isfinite(values).sum() <= 0.45
    th = DM.population(cid)
    sigma = {"additive": [("param", c["dim"] - 1)]}
    with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
        eng.set_prior(DM.priors(cid))
        eng.set_model_user(c["source"], c["ns"], t, obs, censor=censor, **DM.model_kwargs(cid))
        _check_against_definition(pkg, eng, th, t, obs, censor, sigma, cid)
        lk_c = eng.download_lk(pkg.SMC_SET_PRED)
        eng.set_model_user(c["source"], c["ns"], t, np.where(censor != 0, np.nan, obs), **DM.model_kwargs(cid))
        lk_d, _ = _sweep(pkg, eng, th)
    # the censored values are in the likelihood: each adds log Phi <= 0 (exactly 0 where the model lies far below the limit)
    assert np.all(lk_c <= lk_d + 1e-9 * np.maximum(1.0, np.abs(lk_d))) and np.mean(lk_c < lk_d - 1e-6) > 0.5


@pytest.mark.gpu
def test_flags_go_with_measured_inputs_and_wider_cond_rows(pkg):
    """F3 of tests/forced_linear_model.py: BDF, eight inputs of 33 knots behind the cond numbers, its own noise model, a ragged row."""
    cid = "F3"
    c = FM.CASES[cid]
    t, values, _ = FM.make_data(cid)
    values = np.where(np.isnan(t)[:, :, None], np.nan, values)
    obs, censor = pkg.user_models.censor_data(values, lower=np.nanquantile(values, 0.3, axis=(0, 1)), upper=np.nanquantile(values, 0.75, axis=(0, 1)))
    assert (censor == -1).any() and (censor == 1).any()
    with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
        eng.set_prior(FM.priors(cid))
        eng.set_model_user(c["source"], c["ns"], t, obs, censor=censor, **FM.model_kwargs(cid))
        _check_against_definition(pkg, eng, FM.population(cid), t, obs, censor, c["noise"], cid)


@pytest.mark.gpu
def test_designs_carry_no_flags_and_run_as_before(pkg):
    """predict_user_at and predictive_summary on a design of their own: the bits of the model without censoring (a design's
    records have the flag word, with no flag set), and the data's own design gives predict_user's predictions."""
    t, obs, censor = _planted(pkg)
    n = 512
    th = _population(n, 5)
    t2 = np.tile(np.linspace(0.0, 12.0, 17), (3, 1))
    t2[1, 11:] = np.nan
    cond2 = np.array([[1.0], [0.7], [2.0]])
    got = {}
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        for name, c in (("plain", None), ("censored", censor)):
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], noise=NC.NOISE, censor=c)
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            pred, info = eng.predict_user_at(th, t=t2, cond=cond2)
            band = eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.05, 0.5), t=t2, cond=cond2, noise=True, seed=11)
            got[name] = (pred, info, band, eng.predict_user_at(th)[0], eng.predict_user(th)[1])
    a, b = got["plain"], got["censored"]
    assert np.array_equal(a[0], b[0], equal_nan=True) and a[1] == b[1] and a[1]["n_failed"] == 0 and np.isfinite(b[0][:, 0]).all()
    for key in ("mean", "sd", "lower", "upper", "n_finite"):
        assert np.array_equal(a[2][key], b[2][key], equal_nan=True), key
    assert np.array_equal(b[3], b[4], equal_nan=True) and np.array_equal(a[3], b[3], equal_nan=True)


@pytest.mark.gpu
def test_full_run_follows_the_chain_and_dropping_the_censored_values_does_not(pkg):
    t, obs, censor, dropped = CC.full_run_data(0)
    share = (censor[:, :, 1] != 0).sum() / (~np.isnan(dropped[:, :, 1]) | (censor[:, :, 1] != 0)).sum()
    assert 0.3 <= share <= 0.5 and not censor[:, :, 0].any()
    n = 8192
    s = pkg.SMCSettings(n_particle=n, priors=PRIORS)
    runs = {}
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        for name, o, c in (("censored", obs, censor), ("dropped", dropped, None)):
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, o, cond=NC.A0[:, None], rtol=1e-6, atol=1e-9, noise=NC.NOISE,
                               censor=c)
            runs[name] = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3)
            assert runs[name]["gamma"] == 1.0
    m, sd = runs["censored"]["p_pred"].mean(axis=0), runs["censored"]["p_pred"].std(axis=0)
    md = runs["dropped"]["p_pred"].mean(axis=0)
    print("mean", m, "sd", sd, "\n(mean - chain) / sd_chain", (m - CHAIN_MEAN) / CHAIN_SD, "sd / sd_chain", sd / CHAIN_SD)
    print(f"k2: censored run {m[1]:.5f}, dropped run {md[1]:.5f}; chains {CHAIN_MEAN[1]:.5f} and {DROPPED_K2:.5f} (sd {CHAIN_SD[1]:.5f})")
    assert np.all(np.abs(m - CHAIN_MEAN) <= 0.5 * CHAIN_SD)
    assert np.all((sd / CHAIN_SD >= 0.75) & (sd / CHAIN_SD <= 1.33))
    assert abs(md[1] - CHAIN_MEAN[1]) > abs(m[1] - CHAIN_MEAN[1])


@pytest.mark.gpu
def test_an_image_that_fits_without_the_flags_and_not_with_them_is_refused_with_the_bytes(pkg):
    """4 experiments x 700 times x 3 outputs under a noise model: records of 4 words, 2560 (pools) + 16 + 4 x 701 x 4 + 72 words =
    110912 B; with the flags a record of an odd n_obs grows to 6 words: 2560 + 16 + 4 x 701 x 6 + 72 words = 155776 B."""
    n_ex, n_t = 4, 700
    t = np.tile(np.linspace(0.0, 10.0, n_t), (n_ex, 1))
    obs = np.zeros((n_ex, n_t, 3))
    cond = np.ones((n_ex, 1))
    noise = {"additive": [("param", 2), ("param", 3), ("param", 3)]}
    src = pkg.user_models.CONSECUTIVE_REACTIONS_ABC
    censor = np.zeros(obs.shape, dtype=np.int8)
    with pkg.HipEngine(64, 5, device=0) as eng:
        eng.set_model_user(src, 2, t, obs, cond=cond, noise=noise)
        eng.set_model_user(src, 2, t, obs, cond=cond, noise=noise, censor=censor)         # no flag set: the same image
        censor[1, 5, 2] = -1
        with pytest.raises(pkg.SmcError, match=r"smc_set_model_user7: .* 155776 B needed, 153600 B available"):
            eng.set_model_user(src, 2, t, obs, cond=cond, noise=noise, censor=censor)
        with pytest.raises(ValueError, match="censor holds the flag -3"):
            eng.set_model_user(src, 2, t, obs, cond=cond, noise=noise, censor=censor * 3)
        small = slice(0, 100)                                                              # the same flags on an image that fits
        eng.set_model_user(src, 2, t[:, small], obs[:, small], cond=cond, noise=noise, censor=censor[:, small])
