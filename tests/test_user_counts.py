"""Count observations of a user model (include/smc_hip.h: COUNT OBSERVATIONS; csrc/user_count.h and the SMC_USER_COUNT blocks of
csrc/user_obs_args.h; user_models.obs_family, count_layout, count_floor, count_excess, count_loglik).  Models, data and the
reference chains live in tests/count_chain.py.

CPU part: count_loglik against a plain loop over scipy.stats' logpmf / logpdf on planted records; the excess on a grid of
counts, means and overdispersions; every refusal in NumPy and through smc_user_count_check / smc_user_obs_family, in the same
words; the count sources compile for gfx950 in their variants; a dump without the name writes dump_source7's files, one with
the name adds user_count.h.

GPU part: the likelihood of a sweep is predict_user's bit for bit and count_loglik of the engine's own predictions (RK45 and
BDF, three models, invalid particles); planted means, counts and overdispersions through a constant model; all-zero families
and the source without the name give the same bits; a Metropolis sweep bit for bit with and without early rejection; with
scheduled events, a measured input, and a censored Gaussian output; designs; a full run against a Metropolis chain on the
closed form, nearer to it than the run that declares the counts Gaussian.

The image of a model with counts is the image without them (C_e lies in words a noise model does not read), so there is no LDS
refusal of its own to test.

Measured on the CPU (SciPy 1.15): |count_loglik - loop| / max(1, |lk|) at most 8.7e-15 (negative binomial), 6.5e-16 (Poisson),
1.6e-15 (three outputs).
Measured on an MI355X: |lk - count_loglik(pred)| / max(1, |lk|) at most 1.5e-15 (A and V B negative binomial), 7.8e-16 (Poisson),
9.2e-16 (three outputs) under RK45 and BDF alike; planted values 4.9e-16 (Poisson, lk down to -3.6e9) and 4.2e-16 (negative
binomial) - 2.4e-12, 4.4e-12 and 1.9e-12 with the lgamma form of the negative binomial that the saddle-point form replaced
(tests/test_likelihood_terms_truth.py holds the terms to their 60-digit values); with events 1.3e-13, the weekly incidence within 3.8e-9 (RK45) and 1.3e-7 (BDF) of solve_ivp; with inputs 6.9e-13;
beside a censored output 1.2e-14; a sweep of 4096 proposals in 190 405 (Poisson) and 190 851 (negative binomial) attempts with
early rejection, 191 086 without; the full run's means within 0.25 chain sd, sd ratios 1.01 ... 1.05, k2 0.30682 (chain 0.30626)
against 0.32506 with the counts declared Gaussian (that chain: 0.3255)."""
import ctypes
import filecmp
import os

import numpy as np
import pytest

import count_chain as CC
import forced_linear_model as FM
import noise_model_chain as NC

RK45, BDF = 0, 1
PRIORS = {nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(CC.NAMES, CC.PRIOR_HIGH)}
# the reference posteriors for data seed 0, V = 300, b = 0.5: `python tests/count_chain.py 0 150000` (acceptance 0.293 and 0.302; the
# means of the two half chains differ by at most 0.03 sd).  The chain with the same counts declared Gaussian with an estimated
# sigma (mean 78.8) has the k2 mean 0.3255, 1.46 chain sd above the negative-binomial one, and twice its sd: 30 times the
# half-chain spread of 0.048 sd.  At b = 0.3 the two differ by 0.06 sd only (seed 0), at V = 3000 by -0.4 sd.
CHAIN_MEAN = np.array([0.79651, 0.30626, 0.0111, 0.51183])
CHAIN_SD = np.array([0.00362, 0.01315, 0.00084, 0.03915])
GAUSS_K2 = 0.3255

MODELS = {      # name: (family, noise, dim, three outputs)
    "negbin": ((0, 2), CC.NOISE_NB, 4, False),
    "poisson": ((0, 1), CC.NOISE_POISSON, 3, False),
    "three": ((2, 1, 0), CC.NOISE_3, 4, True),
}


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _bar(lk, ref):
    return np.max(np.abs(lk - ref) / np.maximum(1.0, np.abs(ref)))


def _data(name, seed=0):
    family, noise, dim, three = MODELS[name]
    return CC.make_data(seed, b=0.0 if name == "poisson" else CC.B_TRUE, three=three)


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_obs_family_reads_the_list_as_the_library_does(pkg):
    um, L = pkg.user_models, pkg.lib()
    buf = (ctypes.c_int * 8)()
    for fam in ((0, 2), (0, 1), (2, 1, 0), (0, 0), (0, 3), (1,)):
        src = CC.source(fam) if len(fam) > 1 else CC.constant_source(fam[0])
        assert um.obs_family(src) == list(fam)
        assert L.smc_user_obs_family(src.encode(), buf, 8) == len(fam) and list(buf)[:len(fam)] == list(fam)
    assert um.obs_family(CC.source()) is None and L.smc_user_obs_family(CC.source().encode(), buf, 8) == 0
    spread = CC.source().replace("__device__ void smc_user_y0", "__device__ const int smc_user_obs_family [ 2 ] = {\n  0 ,\n 2 };\n__device__ void smc_user_y0", 1)
    assert um.obs_family(spread) == [0, 2] and L.smc_user_obs_family(spread.encode(), buf, 8) == 2
    how = ("smc_user_obs_family: the families are written as a list of the integers 0 (Gaussian), 1 (Poisson) or 2 (negative binomial) "
           "behind the first smc_user_obs_family[ of the source")
    for bad in ("// smc_user_obs_family only in a comment\n" + CC.source(), CC.source().replace("y[1] = 0.0; }", "y[1] = 0.0; }\n__device__ const int smc_user_obs_family[] = {0, two};", 1),
                CC.source() + "__device__ const int smc_user_obs_family[2];\n", CC.source() + "__device__ const int smc_user_obs_family[] = {};\n"):
        with pytest.raises(ValueError) as e:
            um.obs_family(bad)
        assert str(e.value) == "obs_family: " + how
        assert L.smc_user_obs_family(bad.encode(), buf, 8) == -1 and L.smc_last_error(None).decode() == how


def test_count_loglik_agrees_with_a_plain_loop_over_scipy(pkg):
    from scipy.stats import nbinom, norm, poisson
    um = pkg.user_models
    rs = np.random.RandomState(5)
    n = 7
    worst = 0.0
    for name, (family, noise, dim, three) in MODELS.items():
        t, obs = _data(name, 11)
        if not three:
            obs = CC.plant(t, obs)
            lay = um.count_layout(t, obs, family, noise, dim=dim)
            assert lay["counts"][3, 1] == 0 and lay["counts"][0, 1] > 10 and np.nanmax(obs[:, :, 1]) == 2000.0 and (obs[0, :3, 1] == 0).all()
            assert (lay["floor"][3] == 0.0) and ((lay["floor"][:3] > 0).all() == (name == "poisson"))
        theta = np.column_stack([rs.uniform(0.5, 1.2, n), rs.uniform(0.1, 0.6, n), rs.uniform(0.005, 0.05, n), rs.uniform(0.02, 1.0, n)])[:, :dim]
        pred = np.stack([CC.closed_form(k1, k2, t, three) for k1, k2 in theta[:, :2]])
        lk = um.count_loglik(pred, t, obs, theta, family, noise)
        ref = np.zeros(n)
        terms = 0
        for p, th in enumerate(theta):
            for e in range(t.shape[0]):
                for i in range(t.shape[1]):
                    if np.isnan(t[e, i]):
                        continue
                    for k, fam in enumerate(family):
                        y, f = obs[e, i, k], pred[p, e, i, k]
                        if np.isnan(y):
                            continue
                        terms += p == 0
                        if fam == 0:
                            ref[p] += norm.logpdf(y, loc=f, scale=th[2])
                        elif fam == 1:
                            ref[p] += poisson.logpmf(y, f)
                        else:
                            phi = 1.0 / th[3] ** 2
                            ref[p] += nbinom.logpmf(y, phi, phi / (phi + f))
        err = _bar(lk, ref)
        worst = max(worst, err)
        print(f"{name}: worst |count_loglik - loop| / max(1, |lk|) = {err:.3g} over {terms} terms, lk from {lk.min():.4g} to {lk.max():.4g}")
        assert terms > 120 and np.all(np.isfinite(ref)) and err <= 1e-11
        # invalid parameters
        bad = theta.copy()
        bad[0, 2] = 0.0
        if dim == 4:
            bad[1, 3], bad[2, 3] = -0.1, 0.0
        lkb = um.count_loglik(pred, t, obs, bad, family, noise)
        assert np.isneginf(lkb[0]) and np.isfinite(lkb[3:]).all()
        assert dim == 3 or (np.isneginf(lkb[1]) and np.isneginf(lkb[2]))
    # every family 0: noise_loglik's / censored_loglik's array exactly
    t, obs = NC.make_data(0)
    theta = np.column_stack([rs.uniform(0.5, 1.2, n), rs.uniform(0.1, 0.6, n), rs.uniform(0.005, 0.05, (n, 3))])
    pred = np.stack([NC.closed_form(k1, k2, t) for k1, k2 in theta[:, :2]])
    assert np.array_equal(um.count_loglik(pred, t, obs, theta, (0, 0), NC.NOISE), um.noise_loglik(pred, t, obs, theta, NC.NOISE))
    c = np.zeros(obs.shape, dtype=np.int8)
    c[0, 3, 1], c[1, 2, 0] = -1, 1
    assert np.array_equal(um.count_loglik(pred, t, obs, theta, (0, 0), NC.NOISE, censor=c), um.censored_loglik(pred, t, obs, c, theta, NC.NOISE))


def test_the_excess_is_non_negative_monotone_and_infinite_where_stated(pkg):
    um = pkg.user_models
    y = np.unique(np.concatenate([[0.0, 1.0, 2.0, 3.0], np.round(np.logspace(0.5, 15.9, 40)), [2.0 ** 53]]))
    mu = np.unique(np.concatenate([[5e-324, 2.2250738585072014e-308], np.logspace(-300, 300, 241), np.logspace(-2, 7, 181)]))
    assert y[0] == 0 and y[-1] == 2.0 ** 53 and mu[0] == 5e-324 and mu[-1] == 1e300
    Y, M = y[:, None], mu[None, :]
    for family, bs in ((1, (0.0,)), (2, (1e-4, 1e-2, 0.3, 1.0, 10.0))):
        for b in bs:
            x = um.count_excess(Y, M, b, family)
            assert x.shape == (y.size, mu.size) and not np.isnan(x).any() and np.all(x >= 0.0)
            # monotone in |mu - y| on each side of the count (the negative binomial's mode in mu is y as well).  No slack: in the
            # saddle-point form nothing large cancels (the lgamma differences it replaced needed one part in 1e12 of the largest
            # term), and neighbouring means of the grid differ by 12 % or more, which moves x by far more than its rounding
            for j, yj in enumerate(y):
                left, right = x[j, mu <= yj], x[j, mu >= yj]
                assert np.all(np.diff(left) <= 0.0) and np.all(np.diff(right) >= 0.0), (family, b, yj)
    at_y = um.count_excess(y[1:], y[1:], 0.0, 1)
    assert np.all(at_y == 0.0) and um.count_excess(0.0, 0.0, 0.0, 1) == 0.0 and um.count_excess(0.0, 0.0, 0.3, 2) == 0.0
    for family, b in ((1, 0.0), (2, 0.3)):
        assert np.all(np.isposinf(um.count_excess(np.array([0.0, 1.0, 7.0]), -1e-300, b, family)))
        assert np.all(np.isposinf(um.count_excess(np.array([0.0, 1.0, 7.0]), np.inf, b, family)))
        assert np.all(np.isposinf(um.count_excess(np.array([1.0, 7.0, 2.0 ** 53]), 0.0, b, family)))
        assert np.all(np.isnan(um.count_excess(np.array([0.0, 1.0, 7.0]), np.nan, b, family)))
        assert np.all(np.isfinite(um.count_excess(np.array([1.0, 7.0]), np.array([1e-300, 1e300])[:, None], b, family)))
    assert np.all(um.count_excess(np.array([0.0, 3.0]), 2.0, np.array([0.0, -1.0, np.nan])[:, None], 2) == 0.0)      # logL = -inf is count_loglik's
    # the floor: the definition where it is exact, and against the series' own next term
    from scipy.special import gammaln, xlogy
    yy = np.arange(0.0, 200.0)
    direct = gammaln(yy + 1.0) - xlogy(yy, yy) + yy
    # the definition's own terms reach 1053 at y = 199 (ulp 2.3e-13) and it rounds four times: 1e-12
    assert np.max(np.abs(um.count_floor(yy) - direct)) <= 1e-12 and um.count_floor(0.0) == 0.0
    big = np.array([1e3, 1e6, 1e9, 2.0 ** 53])
    assert np.max(np.abs(um.count_floor(big) - (0.5 * np.log(2 * np.pi * big) + 1 / (12 * big)))) <= 1e-9


def _spec_arrays(um, noise, n_obs, dim):
    if noise is None:
        return None, None, None, None
    return um.noise_layout(noise, n_obs, dim)


def _refusals():
    """(source family or None, t, obs, keyword arguments of count_layout, the reason without its prefix)"""
    t, obs = CC.make_data(0)
    nb = dict(noise=CC.NOISE_NB, dim=4)
    out = []
    o = obs.copy(); o[1, 3, 1] = 2.5
    out.append(((0, 2), t, o, nb, "obs holds a value that is not an integer on a count output at row 1, time 3, output 1"))
    o = obs.copy(); o[0, 2, 1] = -1.0
    out.append(((0, 2), t, o, nb, "obs holds a negative value on a count output at row 0, time 2, output 1"))
    o = obs.copy(); o[3, 29, 1] = 2.0 ** 53 + 2.0
    out.append(((0, 2), t, o, nb, "obs holds a value above 2^53 on a count output at row 3, time 29, output 1"))
    o = obs.copy(); o[1, 6, 1] = 4.0
    c = np.zeros(obs.shape, dtype=np.int8); c[1, 6, 1] = -1
    out.append(((0, 2), t, o, dict(nb, censor=c), "censor flags a value of a count output at row 1, time 6, output 1 (censored counts are not supported)"))
    out.append(((0, 2), t, obs, dict(nb, obs_scale=(1.0, 2.0)), "output 1: the obs_scale of a count output must be 1"))
    out.append(((0, 2), t, obs, dict(noise={"additive": [("param", 2), ("fixed", 2.0)], "proportional": CC.NOISE_NB["proportional"]}, dim=4),
                "output 1: the additive entry of a count output must be fixed at 1 (it is not used)"))
    out.append(((0, 2), t, obs, dict(noise={"additive": [("param", 2), ("param", 3)], "proportional": CC.NOISE_NB["proportional"]}, dim=4),
                "output 1: the additive entry of a count output must be fixed at 1 (it is not used)"))
    out.append(((0, 1), t, obs, nb, "output 1: a Poisson output takes no proportional entry (absent, or fixed at 0)"))
    out.append(((0, 2), t, obs, dict(noise=CC.NOISE_POISSON, dim=4), "output 1: a negative-binomial output needs a proportional entry (its b_k: a parameter, or fixed > 0)"))
    out.append(((0, 2), t, obs, dict(noise={"additive": CC.NOISE_NB["additive"], "proportional": [("fixed", 0.0), ("fixed", 0.0)]}, dim=4),
                "output 1: a negative-binomial output needs a proportional entry (its b_k: a parameter, or fixed > 0)"))
    out.append(((1, 1), t, np.where(np.isnan(obs), np.nan, np.round(np.abs(obs))), dict(noise=None, est_sigma=True, dim=3),
                "est_sigma without a noise model and no Gaussian output: the last parameter would be a noise level that nothing uses"))
    out.append(((0, 2, 1), t, obs, nb, "smc_user_obs_family: 3 entries for n_obs = 2 outputs (one entry per output)"))
    out.append(((0, 3), t, obs, nb, "smc_user_obs_family: entry 3 of output 1 is none of 0 (Gaussian), 1 (Poisson), 2 (negative binomial)"))
    out.append(((2,), t, obs[:, :, 1], dict(noise=None, dim=3), "smc_user_obs_family: the name in a one-output source (n_obs = 0) - count outputs need the "
                "multi-output source (smc_user_obs_vec, n_obs >= 1)"))
    return out


def _c_check(pkg, family, t, obs, noise=None, obs_scale=None, censor=None, est_sigma=False, dim=None):
    um, L = pkg.user_models, pkg.lib()
    t, obs = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(obs, dtype=np.float64)
    n_obs = obs.shape[2] if obs.ndim == 3 else 0
    fam = np.ascontiguousarray(family, dtype=np.int32)
    ai, af, pi, pf = _spec_arrays(um, noise, max(n_obs, 1), dim)
    keep = [None if a is None else np.ascontiguousarray(a) for a in (ai, af, pi, pf)]
    sc = None if obs_scale is None else np.ascontiguousarray(obs_scale, dtype=np.float64)
    cz = None if censor is None else np.ascontiguousarray(censor, dtype=np.int8)
    return L.smc_user_count_check(_ip(fam), fam.size, _dp(t), _dp(obs), None if cz is None else cz.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
                                  _dp(sc), t.shape[0], t.shape[1], n_obs, int(est_sigma), _ip(keep[0]), _dp(keep[1]), _ip(keep[2]), _dp(keep[3]))


@pytest.mark.parametrize("k", range(14))
def test_refusals_come_in_the_same_words_from_numpy_and_the_library(pkg, k):
    family, t, obs, kw, why = _refusals()[k]
    with pytest.raises(ValueError) as e:
        pkg.user_models.count_layout(t, obs, family, **kw)
    assert str(e.value) == "count_layout: " + why, str(e.value)
    assert _c_check(pkg, family, t, obs, **kw) != 0
    msg = pkg.lib().smc_last_error(None).decode()
    assert msg == "smc_user_count_check: " + why, msg


def test_accepted_models_pass_both_checks(pkg):
    um = pkg.user_models
    for name, (family, noise, dim, three) in MODELS.items():
        t, obs = _data(name)
        lay = um.count_layout(t, obs, family, noise, dim=dim)
        assert _c_check(pkg, family, t, obs, noise=noise, dim=dim) == 0
        seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
        assert np.array_equal(lay["counts"], (seen & (np.array(family) != 0)).sum(axis=1))
    t, obs = _data("poisson")
    assert _c_check(pkg, (0, 1), t, obs, noise=None, est_sigma=True, dim=3) == 0          # the sigma rule with a Gaussian output
    assert _c_check(pkg, (0, 0), t, obs * 0.5, noise=None, est_sigma=True, dim=3) == 0    # no count: nothing to check
    c = np.zeros(obs.shape, dtype=np.int8)
    c[0, 3, 0] = -1                                                                        # a flag on the Gaussian output is fine
    assert np.isfinite(obs[0, 3, 0]) and _c_check(pkg, (0, 1), t, obs, noise=CC.NOISE_POISSON, censor=c, dim=3) == 0
    um.count_layout(t, obs, (0, 1), CC.NOISE_POISSON, censor=c, dim=3)


def _check_spec(pkg, src, **fields):
    log = ctypes.create_string_buffer(16384)
    spec = pkg.binding.UserSourceSpec(source=src.encode(), **fields)
    return pkg.lib().smc_user_model_check_spec(ctypes.byref(spec), log, 16384), log.value.decode(errors="replace")


def test_count_sources_compile_for_gfx950_in_their_variants(pkg):
    um = pkg.user_models
    for method in (RK45, BDF):
        for fam, noise, n_obs in (((0, 2), 2, 2), ((0, 1), 1, 2), ((0, 1), 2, 2), ((2, 1, 0), 2, 3)):
            rc, log = _check_spec(pkg, CC.source(fam), n_states=2, dim=4, method=method, n_obs=n_obs, noise=noise, n_cond=2)
            assert rc == 0, (method, fam, noise, log)
        # censoring on the Gaussian output beside the count
        rc, log = _check_spec(pkg, CC.source((0, 2)), n_states=2, dim=4, method=method, n_obs=2, noise=2, n_cond=2, censor=1)
        assert rc == 0, log
        # scheduled events; a measured input; state-triggered events
        rc, log = _check_spec(pkg, um.SIR_WEEKLY_CASES, n_states=3, dim=3, method=method, n_obs=1, noise=2, n_cond=2, n_ev=7, n_val=0)
        assert rc == 0, log
        rc, log = _check_spec(pkg, CC.family_line((2, 0)) + FM.F3_SOURCE, n_states=2, dim=5, method=method, n_obs=2, noise=2, n_cond=3, n_in=8, n_knot=33)
        assert rc == 0, log
        rc, log = _check_spec(pkg, CC.family_line((1,)) + um.THRESHOLD_REDOSED, n_states=1, dim=3, method=method, n_obs=1, noise=1, n_cond=2)
        assert rc == 0, log
    # what does not compile says which rule was broken
    for fam, noise, n_obs, why in (((0, 3), 2, 2, "entry 3 of output 1 is none of 0 (Gaussian), 1 (Poisson), 2 (negative binomial)"),
                                   ((0, 2, 1), 2, 2, "3 entries for n_obs = 2 outputs"), ((0, 2), 0, 0, "the name in a one-output source (n_obs = 0)"),
                                   ((0, 2), 1, 2, "a negative-binomial output needs the proportional part (noise = 2)"),
                                   ((0, 1), 0, 2, "a model with a count output is compiled with a noise model")):
        rc, log = _check_spec(pkg, CC.source(fam), n_states=2, dim=4, method=RK45, n_obs=n_obs, noise=noise, n_cond=2)
        assert rc == 1 and "smc_user_obs_family: " in log and why in log, (fam, log)
    # an all-zero list is a model without counts, under the sigma rule too
    rc, log = _check_spec(pkg, CC.source((0, 0)), n_states=2, dim=4, method=RK45, n_obs=2, noise=0, n_cond=2)
    assert rc == 0, log


def _dump(pkg, src, d, **fields):
    spec = pkg.binding.UserSourceSpec(source=src.encode(), **fields)
    return pkg.lib().smc_user_model_dump_source_spec(ctypes.byref(spec), str(d).encode())


def test_a_dump_without_the_name_is_dump_source7s_and_one_with_it_adds_user_count_h(pkg, tmp_path):
    L = pkg.lib()
    for j, (method, noise, censor) in enumerate([(RK45, 2, 0), (BDF, 1, 0), (RK45, 2, 1), (RK45, 0, 0)]):
        d7, ds, dz, dc = (tmp_path / f"{nm}{j}" for nm in ("seven", "spec", "zero", "count"))
        for d in (d7, ds, dz, dc):
            d.mkdir()
        fields = dict(n_states=2, dim=4, method=method, n_obs=2, noise=noise, n_cond=2, censor=censor)
        assert L.smc_user_model_dump_source7(CC.source().encode(), 2, 4, method, 2, noise, 2, 0, 0, 0, 0, censor, str(d7).encode()) == 0
        assert _dump(pkg, CC.source(), ds, **fields) == 0
        names = sorted(os.listdir(d7))
        assert sorted(os.listdir(ds)) == names and "user_count.h" not in names
        match, mismatch, errors = filecmp.cmpfiles(d7, ds, names, shallow=False)
        assert sorted(match) == names and not mismatch and not errors
        for f in names:
            assert "SMC_USER_COUNT" not in (ds / f).read_text(), f
        # an all-zero list: the same headers, and no switch in the source
        assert _dump(pkg, CC.source((0, 0)), dz, **fields) == 0
        assert sorted(os.listdir(dz)) == names and "#define SMC_USER_COUNT" not in (dz / "smc_user_model.hip").read_text()
        match, mismatch, errors = filecmp.cmpfiles(d7, dz, [f for f in names if f != "smc_user_model.hip"], shallow=False)
        assert not mismatch and not errors
        if noise:
            fam = (0, 2) if noise == 2 else (0, 1)
            assert _dump(pkg, CC.source(fam), dc, **fields) == 0
            assert sorted(os.listdir(dc)) == sorted(names + ["user_count.h"])
            head = (dc / "smc_user_model.hip").read_text()[:900]
            assert "#define SMC_USER_COUNT 1\n#define SMC_USER_FAMILY {0, %d}\n" % fam[1] in head
            assert "SMC_USER_COUNT" in (dc / "user_obs_args.h").read_text()
            assert ("SMC_USER_CENSOR" in (dc / "user_obs_args.h").read_text()) == bool(censor)


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _population(name, n, seed, invalid=True):
    family, noise, dim, three = MODELS[name]
    rs = np.random.RandomState(seed)
    th = np.column_stack([NC.K_TRUE[0] * (1 + 0.1 * rs.standard_normal(n)), NC.K_TRUE[1] * (1 + 0.1 * rs.standard_normal(n)),
                          rs.uniform(0.005, 0.03, n), rs.uniform(0.05, 0.9, n)])[:, :dim]
    if invalid and dim == 4:      # b < 0, negative binomial b = 0, NaN, a <= 0 - and small and large overdispersions behind them
        th[0, 3], th[1, 3], th[2, 3], th[3, 2] = -0.1, 0.0, np.nan, 0.0
        th[4:8, 3] = (1e-3, 0.02, 3.0, 1.0)
    elif invalid:
        th[0, 2], th[1, 2], th[2, 2], th[3, 2] = 0.0, np.nan, -0.5, -1.0
    return th


def _sweep(pkg, eng, th):
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    return eng.download_lk(pkg.SMC_SET_PRED), info


def _set(pkg, eng, name, t, obs, family="model", **kw):
    fam, noise, dim, three = MODELS[name]
    src = CC.source(fam if family == "model" else family)
    eng.set_model_user(src, 2, t, obs, cond=CC.COND, noise=noise, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_likelihood_is_count_loglik_of_the_engines_own_predictions(pkg, method, name):
    family, noise, dim, three = MODELS[name]
    t, obs = _data(name)
    if not three:
        obs = CC.plant(t, obs)
    n = 512
    th = _population(name, n, 1)
    with pkg.HipEngine(n, dim, device=0) as eng:
        eng.set_prior(dict(list(PRIORS.items())[:dim]))
        _set(pkg, eng, name, t, obs, method=method)
        lk, info = _sweep(pkg, eng, th)
        lk_p, pred, pinfo = eng.predict_user(th)
    assert info["n_failed"] == 0 and info["rk_attempts"] == pinfo["rk_attempts"] and np.array_equal(lk, lk_p, equal_nan=True)
    if dim == 4:
        assert np.isneginf(lk[[0, 1, 3]]).all() and not np.isfinite(lk[2])
    else:
        assert np.isneginf(lk[[0, 2, 3]]).all() and not np.isfinite(lk[1])
    ref = pkg.user_models.count_loglik(pred, t, obs, th, family, noise)
    assert np.isfinite(lk[4:]).all() and np.isfinite(ref[4:]).all()
    err = _bar(lk[4:], ref[4:])
    print(f"{name} {method}: worst |lk - count_loglik(pred)| / max(1, |lk|) = {err:.3g}; lk from {lk[4:].min():.4g} to {lk[4:].max():.4g}")
    assert err <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("family", [1, 2], ids=["poisson", "negbin"])
def test_planted_means_counts_and_overdispersions(pkg, family):
    """dy/dt = 0, out = theta[0]: mu from 1e-300 to 1e6 (and 0, negative, NaN in front), y from 0 to 1e6, b from 1e-3 to 3."""
    um = pkg.user_models
    n, n_t = 512, 64
    rs = np.random.RandomState(3)
    y = np.concatenate([[0.0, 0.0, 1.0, 2.0], np.round(np.logspace(0.5, 6.0, n_t - 4))])
    t = np.linspace(0.0, 1.0, n_t)[None, :]
    obs = y[None, :, None]
    th = np.column_stack([np.logspace(-300.0, 6.0, n), np.exp(rs.uniform(np.log(1e-3), np.log(3.0), n))])
    th[:3, 0] = (0.0, -1.0, np.nan)
    th[3:40:4, 0] = rs.choice(y[y > 0], 10)                      # mu = y exactly somewhere
    th[n - 64:, 0] = np.exp(rs.uniform(np.log(0.5), np.log(2e6), 64))
    noise = None if family == 1 else {"additive": [("fixed", 1.0)], "proportional": [("param", 1)]}
    spec = {"additive": [("fixed", 1.0)]} if family == 1 else noise
    for zeros in (False, True):
        o = np.zeros_like(obs) if zeros else obs                 # all zeros: mu = 0 with y = 0 is x = 0
        with pkg.HipEngine(n, 2, device=0) as eng:
            eng.set_prior({"mu": {"dist": "uniform", "low": 0, "high": 1e7}, "b": {"dist": "uniform", "low": 0, "high": 5}})
            eng.set_model_user(CC.constant_source(family), 1, t, o, est_sigma=False, noise=noise)
            lk, info = _sweep(pkg, eng, th)
            lk_p, pred, _ = eng.predict_user(th)
        assert np.array_equal(lk, lk_p, equal_nan=True) and np.array_equal(pred[3:, 0, :, 0], np.repeat(th[3:, :1], n_t, axis=1))
        ref = um.count_loglik(pred, t, o, th, (family,), spec)
        assert np.isneginf(lk[1]) and np.isnan(lk[2]) and (lk[0] == 0.0 if zeros else np.isneginf(lk[0]))
        assert np.isfinite(lk[3:]).all() and np.isfinite(ref[3:]).all()
        err = _bar(lk[3:], ref[3:])
        print(f"family {family}{' (all zeros)' if zeros else ''}: worst |lk - count_loglik| / max(1, |lk|) = {err:.3g}; lk from {lk[3:].min():.4g} to {lk[3:].max():.4g}")
        assert err <= 1e-9


@pytest.mark.gpu
def test_all_zero_families_and_no_name_give_the_same_bits(pkg):
    t, obs = NC.make_data(0)
    n = 512
    th = np.column_stack([_population("negbin", n, 2, invalid=False)[:, :3], np.random.RandomState(2).uniform(0.005, 0.03, n)])
    cases = ({}, {"noise": {"additive": [("param", 2), ("param", 3)]}, "obs_scale": (1.0, 3.0)},
             {"noise": {"additive": [("param", 2), ("param", 3)], "proportional": [("fixed", 0.1), ("fixed", 0.0)]}})
    with pkg.HipEngine(n, 4, device=0) as eng:
        eng.set_prior(PRIORS)
        for kw in cases:
            got = []
            for fam in (None, (0, 0)):
                eng.set_model_user(CC.source(fam), 2, t, obs, cond=CC.COND, **kw)
                lk, info = _sweep(pkg, eng, th)
                got.append((lk, info, eng.predict_user(th)))
            (lk_a, info_a, pa), (lk_b, info_b, pb) = got
            assert np.array_equal(lk_a, lk_b) and info_a == info_b and np.all(np.isfinite(lk_a))
            assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1], equal_nan=True) and pa[2] == pb[2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poisson", "negbin"])
def test_early_rejection_is_exact_and_saves_attempts_on_counts(pkg, name):
    """A Metropolis sweep of 4096 proposals; start rejection stays at its default throughout."""
    family, noise, dim, three = MODELS[name]
    t, obs = _data(name, 3)
    n = 4096
    th = _population(name, n, 7, invalid=False)
    out = []
    with pkg.HipEngine(n, dim, device=0) as eng:
        eng.set_prior(dict(list(PRIORS.items())[:dim]))
        _set(pkg, eng, name, t, obs)
        lk, info = _sweep(pkg, eng, th)
        assert info["n_failed"] == 0 and np.all(np.isfinite(lk))
        for on in (False, True):
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_lk(pkg.SMC_SET_FILT, lk)
            eng.set_early_reject(on)
            mh = eng.mh_step_device_rng(0.5, 1.0, np.diag([0.004, 0.004, 2e-5, 1e-3][:dim]), 7, 3)
            out.append((mh, eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags()))
    (m0, p0, l0, a0), (m1, p1, l1, a1) = out
    print(f"{name}: accepted {m0['accepted_now']} of {n}; attempts {m0['rk_attempts']} without, {m1['rk_attempts']} with early rejection")
    assert m0["n_failed"] == 0 and m1["n_failed"] == 0 and 0 < m0["accepted_now"] < n
    assert m0["accepted_now"] == m1["accepted_now"] and np.array_equal(a0, a1) and np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert m1["rk_attempts"] < m0["rk_attempts"]


def _against_definition(pkg, eng, th, t, obs, family, noise, what, censor=None):
    lk, info = _sweep(pkg, eng, th)
    lk_p, pred, pinfo = eng.predict_user(th)
    assert info["n_failed"] == 0 and pinfo["n_failed"] == 0 and np.array_equal(lk, lk_p)
    ref = pkg.user_models.count_loglik(pred, t, obs, th, family, noise, censor=censor)
    assert np.all(np.isfinite(ref))
    err = _bar(lk, ref)
    print(f"{what}: worst |lk - count_loglik(pred)| / max(1, |lk|) = {err:.3g}")
    assert err <= 1e-9
    return pred


def _sir_weekly(theta, cond, weeks):
    """New infections per week by solve_ivp at tight tolerances: S(t_{i-1}) - S(t_i)."""
    from scipy.integrate import solve_ivp
    N, I0 = cond
    sol = solve_ivp(lambda t, y: [-theta[0] * y[0] * y[1] / N, theta[0] * y[0] * y[1] / N - theta[1] * y[1]], (0.0, weeks[-1]), [N - I0, I0],
                    t_eval=weeks, rtol=1e-10, atol=1e-10)
    return -np.diff(sol.y[0])


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_counts_of_an_accumulator_that_scheduled_events_reset(pkg, method):
    """The SIR model with weekly case counts at its smallest: 2 experiments x 8 reports.  A data time equal to an event time sees
    the accumulator before the reset, so the outputs are the weekly incidences."""
    um = pkg.user_models
    weeks = np.arange(0.0, 9.0)
    t = np.tile(weeks, (2, 1))
    cond = np.array([[10000.0, 10.0], [5000.0, 20.0]])
    true = np.array([1.6, 0.7, 0.3])
    ev_t = np.tile(weeks[1:8], (2, 1))
    rs = np.random.RandomState(8)
    inc = np.stack([_sir_weekly(true, c, weeks) for c in cond])
    obs = np.full((2, 9, 1), np.nan)
    obs[:, 1:, 0] = CC.negbin_draw(rs, inc, true[2])
    obs[1, 4, 0] = np.nan
    n = 512
    th = np.column_stack([rs.uniform(1.2, 2.0, n), rs.uniform(0.5, 0.9, n), rs.uniform(0.05, 0.8, n)])
    th[0] = true
    noise = {"additive": [("fixed", 1.0)], "proportional": [("param", 2)]}
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior({"beta": {"dist": "uniform", "low": 0, "high": 5}, "gamma": {"dist": "uniform", "low": 0, "high": 5}, "b": {"dist": "uniform", "low": 0, "high": 2}})
        eng.set_model_user(um.SIR_WEEKLY_CASES, 3, t, obs, cond=cond, noise=noise, events={"t": ev_t, "values": None}, method=method,
                           rtol=1e-8, atol=1e-8)
        pred = _against_definition(pkg, eng, th, t, obs, (2,), noise, f"SIR {method}")
    rel = np.max(np.abs(pred[0, :, 1:, 0] - inc) / inc)
    print(f"weekly incidence against solve_ivp: {rel:.3g}")
    assert np.all(pred[0, :, 0, 0] == 0.0) and rel <= 1e-5


@pytest.mark.gpu
def test_counts_go_with_measured_inputs(pkg):
    """F3 of tests/forced_linear_model.py (BDF, eight inputs, a ragged row) with its first output counted, negative binomial."""
    cid = "F3"
    c = FM.CASES[cid]
    t, values, _ = FM.make_data(cid)
    obs = np.where(np.isnan(t)[:, :, None], np.nan, values)
    obs[:, :, 0] = np.where(np.isnan(obs[:, :, 0]), np.nan, np.round(np.abs(obs[:, :, 0]) * 3.0))
    noise = {"additive": [("fixed", 1.0), ("param", 3)], "proportional": [("param", 4), ("fixed", 0.0)]}
    kw = dict(FM.model_kwargs(cid), noise=noise)
    with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
        eng.set_prior(FM.priors(cid))
        eng.set_model_user(CC.family_line((2, 0)) + c["source"], c["ns"], t, obs, **kw)
        _against_definition(pkg, eng, FM.population(cid), t, obs, (2, 0), noise, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poisson", "negbin"])
def test_a_censored_gaussian_output_beside_a_count(pkg, name):
    family, noise, dim, three = MODELS[name]
    t, obs = _data(name)
    values = np.where(np.isnan(t)[:, :, None], np.nan, obs)
    o, censor = pkg.user_models.censor_data(values, lower=[np.nanquantile(values[:, :, 0], 0.3), np.nan])
    assert (censor[:, :, 0] != 0).sum() > 15 and not censor[:, :, 1].any()
    n = 512
    th = _population(name, n, 4, invalid=False)
    with pkg.HipEngine(n, dim, device=0) as eng:
        eng.set_prior(dict(list(PRIORS.items())[:dim]))
        _set(pkg, eng, name, t, o, censor=censor)
        _against_definition(pkg, eng, th, t, o, family, noise, f"censored A beside {name}", censor=censor)
        bad = censor.copy()
        e, i = np.argwhere(np.isfinite(o[:, :, 1]) & ~np.isnan(t))[5]
        bad[e, i, 1] = 1
        with pytest.raises(ValueError, match=f"censor flags a value of a count output at row {e}, time {i}, output 1"):
            _set(pkg, eng, name, t, o, censor=bad)


@pytest.mark.gpu
def test_the_engine_refuses_in_the_librarys_words_and_the_library_refuses_alone(pkg):
    t, obs = _data("negbin")
    with pkg.HipEngine(64, 4, device=0) as eng:
        with pytest.raises(ValueError, match="a negative-binomial output needs a proportional entry"):
            eng.set_model_user(CC.source((0, 2)), 2, t, obs, cond=CC.COND)                       # the sigma rule has no b
        with pytest.raises(ValueError, match="3 entries for n_obs = 2 outputs"):
            eng.set_model_user(CC.source((0, 2, 1)), 2, t, obs, cond=CC.COND, noise=CC.NOISE_NB)
        with pytest.raises(ValueError, match="the name in a one-output source"):
            eng.set_model_user(CC.constant_source(1).replace("smc_user_obs_vec", "smc_user_obs"), 1, t, obs[:, :, 1])
        # past the Python checks: the library's own refusal through the struct
        um = pkg.user_models
        ai, af, pi, pf = um.noise_layout(CC.NOISE_POISSON, 2, 4)
        tt, oo, cc = np.ascontiguousarray(t), np.ascontiguousarray(obs), np.ascontiguousarray(CC.COND)
        spec = pkg.binding.UserModelSpec(source=CC.source((0, 2)).encode(), n_states=2, method=RK45, n_obs=2, t=_dp(tt), obs=_dp(oo), cond=_dp(cc),
                                         n_ex=4, n_t=30, n_cond=2, add_index=_ip(ai), add_fixed=_dp(af), rtol=1e-3, atol=1e-6)
        assert eng.L.smc_set_model_user_spec(eng.ctx, ctypes.byref(spec)) != 0
        msg = eng.L.smc_last_error(eng.ctx).decode()
        assert msg == "smc_set_model_user_spec: output 1: a negative-binomial output needs a proportional entry (its b_k: a parameter, or fixed > 0)", msg
        # noise=None: Gaussian outputs from est_sigma, the count at fixed 1 - the explicit specification's likelihood
        tp, op = _data("poisson")
        th = _population("poisson", 64, 9, invalid=False)
        eng2_lk = []
        with pkg.HipEngine(64, 3, device=0) as e3:
            e3.set_prior(dict(list(PRIORS.items())[:3]))
            for kw in ({}, {"noise": CC.NOISE_POISSON}):
                e3.set_model_user(CC.source((0, 1)), 2, tp, op, cond=CC.COND, **kw)
                eng2_lk.append(_sweep(pkg, e3, th)[0])
        assert np.all(np.isfinite(eng2_lk[0])) and _bar(eng2_lk[0], eng2_lk[1]) <= 1e-9


@pytest.mark.gpu
def test_designs_give_the_mean_and_replicated_counts_are_refused(pkg):
    t, obs = _data("negbin")
    n = 512
    th = _population("negbin", n, 5, invalid=False)
    t2 = np.tile(np.linspace(0.0, 12.0, 17), (3, 1))
    t2[1, 11:] = np.nan
    cond2 = np.array([[1.0, 300.0], [0.7, 100.0], [2.0, 500.0]])
    got = {}
    with pkg.HipEngine(n, 4, device=0) as eng:
        eng.set_prior(PRIORS)
        for name, fam in (("gauss", (0, 0)), ("count", (0, 2))):
            eng.set_model_user(CC.source(fam), 2, t, obs, cond=CC.COND, noise=CC.NOISE_NB if name == "count" else
                               {"additive": [("param", 2), ("fixed", 1.0)], "proportional": [("fixed", 0.0), ("param", 3)]})
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            pred, info = eng.predict_user_at(th, t=t2, cond=cond2)
            band = eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.05, 0.5), t=t2, cond=cond2, noise=False)
            got[name] = (pred, info, band, eng.predict_user_at(th)[0], eng.predict_user(th)[1])
        with pytest.raises(pkg.SmcError, match="replicated count draws need a Poisson / gamma sampler on the Philox stream"):
            eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.05, 0.5), t=t2, cond=cond2, noise=True, seed=11)
    a, b = got["gauss"], got["count"]
    assert np.array_equal(a[0], b[0], equal_nan=True) and a[1] == b[1] and a[1]["n_failed"] == 0 and np.isfinite(b[0][:, 0]).all()
    for key in ("mean", "sd", "lower", "upper", "n_finite"):
        assert np.array_equal(a[2][key], b[2][key], equal_nan=True), key
    assert np.array_equal(b[3], b[4], equal_nan=True) and np.array_equal(a[3], b[3], equal_nan=True)


@pytest.mark.gpu
def test_full_run_follows_the_chain_and_the_gaussian_declaration_does_not(pkg):
    t, obs = CC.make_data(0)
    n = 8192
    runs = {}
    for name, fam, noise, high in (("negbin", (0, 2), CC.NOISE_NB, CC.PRIOR_HIGH), ("gauss", None, CC.NOISE_GAUSS, CC.GAUSS_PRIOR_HIGH)):
        priors = {nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(CC.NAMES, high)}
        s = pkg.SMCSettings(n_particle=n, priors=priors)
        with pkg.HipEngine(n, 4, device=0) as eng:
            eng.set_prior(priors)
            eng.set_model_user(CC.source(fam), 2, t, obs, cond=CC.COND, rtol=1e-6, atol=1e-9, noise=noise)
            runs[name] = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3)
            assert runs[name]["gamma"] == 1.0
    m, sd = runs["negbin"]["p_pred"].mean(axis=0), runs["negbin"]["p_pred"].std(axis=0)
    mg = runs["gauss"]["p_pred"].mean(axis=0)
    print("mean", m, "sd", sd, "\n(mean - chain) / sd_chain", (m - CHAIN_MEAN) / CHAIN_SD, "sd / sd_chain", sd / CHAIN_SD)
    print(f"k2: negative-binomial run {m[1]:.5f}, Gaussian declaration {mg[1]:.5f}; chains {CHAIN_MEAN[1]:.5f} and {GAUSS_K2:.5f} (sd {CHAIN_SD[1]:.5f})")
    assert np.all(np.abs(m - CHAIN_MEAN) <= 0.5 * CHAIN_SD)
    assert np.all((sd / CHAIN_SD >= 0.75) & (sd / CHAIN_SD <= 1.33))
    assert abs(mg[1] - CHAIN_MEAN[1]) > abs(m[1] - CHAIN_MEAN[1])
