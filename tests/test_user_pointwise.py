"""Pointwise log-likelihood, WAIC and PIT of a user model (include/smc_hip.h: smc_user_pointwise, smc_user_pointwise_summary;
user_models.pointwise_loglik / pointwise_stats / pointwise_merge / pointwise_pit / waic; csrc/pointwise_kernels.hip).

CPU part: the NumPy definitions - their sums are the likelihoods that define the engine's lk, each term is SciPy's
logpdf / logcdf / logsf / logpmf, the statistics are logsumexp and nanvar, blocks merge into the whole; csrc/pointwise_reduce.h
on the host under -fsanitize=address,undefined against long double; the kernels compile for gfx950 without scratch.
GPU part: the device's terms against the definition applied to the device's own predictions (planted values, every family and
both entry points' sizes), real models against predict_user's lk, the per-cell statistics against NumPy on the device's own terms,
a closed form at n = 65536, staging groups and repeated calls bit for bit, and run_smc(pointwise=True) on one and several ranks.

Measured on an MI355X (worst |device - definition| / max(1, |l|) per family, planted values, bar 1e-9): Gaussian
4.4e-16, left-censored 1.1e-15, right-censored 1.0e-15, Poisson 5.5e-15, negative binomial 6.7e-15 (1.4e-12 with the lgamma form).  Real models, nansum(ll)
against predict_user's lk: 6.9e-14 at worst.  Closed form: lpd off by 1.9 se, pit by 1.7e-3."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

import censored_chain as CE
import count_chain as CC
import noise_model_chain as NC
import pointwise_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-based-sequential-monte-carlo-method-with-likelihood-tempering_amd", "csrc")
EPS = 2.0 ** -52


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _within(a, b, tol):
    """a and b agree: NaN where the other is, the same infinity, else |a - b| <= tol (tol broadcasts)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), a.shape)
    both_nan = np.isnan(a) & np.isnan(b)
    same_inf = np.isinf(a) & (a == b)
    with np.errstate(invalid="ignore"):
        close = np.abs(a - b) <= tol
    return bool(np.all(both_nan | same_inf | (close & np.isfinite(a) & np.isfinite(b))))


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _max_abs(ll):
    """per cell the largest finite |l| (0 where there is none)"""
    return np.max(np.where(np.isfinite(ll), np.abs(ll), 0.0), axis=0)


def _stats_agree(got, want, ll, what=""):
    """The bounds of the issue between two sets of raw statistics of the terms ll (n, ...): n and max exact, mean within
    n eps max|l|, sqrt(m2 / n) within 4 n eps max|l|, sum_exp within (n + 4) eps relative."""
    n = np.asarray(want["n"], dtype=np.float64)
    big = _max_abs(ll)
    assert np.array_equal(got["n"], want["n"]), what
    assert _bits(got["max"], want["max"]), what
    assert _within(got["mean"], want["mean"], n * EPS * big), what
    with np.errstate(all="ignore"):
        assert _within(np.sqrt(got["m2"] / n), np.sqrt(want["m2"] / n), 4 * n * EPS * big), what
        assert _within(got["sum_exp"], want["sum_exp"], (n + 4) * EPS * np.abs(want["sum_exp"])), what


# ---- CPU -----------------------------------------------------------------------------------------------------------

def _theta(rs, n, dim, five=False):
    cols = [rs.uniform(0.5, 1.2, n), rs.uniform(0.1, 0.6, n), rs.uniform(0.005, 0.05, n), rs.uniform(0.02, 1.0, n)]
    if five:
        cols = cols[:3] + [rs.uniform(0.005, 0.05, n), rs.uniform(0.0, 0.3, n)]
    return np.column_stack(cols)[:, :dim]


def _cpu_cases(um):
    """(name, t, obs, censor, family, noise, theta, pred, the sum's definition)"""
    rs = np.random.RandomState(5)
    n = 7
    cases = []
    t, obs = NC.make_data(3)
    th = _theta(rs, n, 5, five=True)
    pred = np.stack([NC.closed_form(k1, k2, t) for k1, k2 in th[:, :2]])
    cases.append(("noise", t, obs, None, None, NC.NOISE, th, pred, lambda p, x: um.noise_loglik(p, t, obs, x, NC.NOISE)))
    tc, values, lower, upper = CE.two_sided(3)
    oc, cc = CE.plant(*um.censor_data(values, lower, upper))
    predc = np.stack([NC.closed_form(k1, k2, tc) for k1, k2 in th[:, :2]])
    cases.append(("censored", tc, oc, cc, None, NC.NOISE, th, predc, lambda p, x: um.censored_loglik(p, tc, oc, cc, x, NC.NOISE)))
    for name, (family, noise, dim, three) in (("negbin", ((0, 2), CC.NOISE_NB, 4, False)), ("poisson", ((0, 1), CC.NOISE_POISSON, 3, False)),
                                              ("three", ((2, 1, 0), CC.NOISE_3, 4, True))):
        tk, ok = CC.make_data(11, b=0.0 if name == "poisson" else CC.B_TRUE, three=three)
        if not three:
            ok = CC.plant(tk, ok)
        thk = _theta(rs, n, dim)
        predk = np.stack([CC.closed_form(k1, k2, tk, three) for k1, k2 in thk[:, :2]])
        cases.append((name, tk, ok, None, family, noise, thk, predk,
                      (lambda tk, ok, family, noise: lambda p, x: um.count_loglik(p, tk, ok, x, family, noise))(tk, ok, family, noise)))
    return cases


def test_terms_sum_to_the_likelihoods_of_the_existing_definitions(pkg):
    um = pkg.user_models
    for name, t, obs, censor, family, noise, th, pred, total in _cpu_cases(um):
        ll = um.pointwise_loglik(pred, t, obs, th, noise, censor=censor, family=family)
        assert ll.shape == pred.shape
        seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
        assert np.array_equal(np.isnan(ll), np.broadcast_to(~seen[None], ll.shape)), name      # NaN exactly at the unobserved cells
        want = total(pred, th)
        cells = int(seen.sum())
        bound = cells * EPS * np.nansum(np.abs(ll), axis=(1, 2, 3))
        err = np.abs(np.nansum(ll, axis=(1, 2, 3)) - want)
        print(f"{name}: {cells} cells, worst |nansum - definition| {err.max():.3g} (bound {bound.min():.3g})")
        assert np.all(np.isfinite(want)) and np.all(err <= bound), name
        bad = th.copy()
        bad[0, 2] = 0.0                                    # an a_k = 0
        if family is not None and 2 in family:
            bad[1, 3], bad[2, 3] = -0.1, 0.0               # b_k < 0, b_k = 0 on the negative-binomial output
        elif th.shape[1] == 5:
            bad[1, 4] = -0.1
        llb = um.pointwise_loglik(pred, t, obs, bad, noise, censor=censor, family=family)
        wantb = total(pred, bad)
        rows = np.isneginf(wantb)
        assert rows[0] and rows.sum() >= 1 + (th.shape[1] >= 4) and not rows[3:].any(), name
        assert np.all(np.isneginf(llb[rows][:, seen])) and np.all(np.isnan(llb[rows][:, ~seen])), name
        assert np.array_equal(llb[~rows], ll[~rows], equal_nan=True), name


def test_every_term_is_scipys_log_density(pkg):
    """... by a plain loop, with the bar tests/test_user_counts.py holds count_loglik to against that loop: 1e-11 max(1, |l|)."""
    from scipy.stats import nbinom, norm, poisson
    um = pkg.user_models
    for name, t, obs, censor, family, noise, th, pred, _ in _cpu_cases(um):
        ll = um.pointwise_loglik(pred, t, obs, th, noise, censor=censor, family=family)
        ai, af, pi, pf = um.noise_layout(noise, obs.shape[2], th.shape[1])
        worst, terms = 0.0, 0
        for p, x in enumerate(th):
            for e, i, k in np.ndindex(obs.shape):
                y, f = obs[e, i, k], pred[p, e, i, k]
                if np.isnan(t[e, i]) or np.isnan(y):
                    continue
                a = x[ai[k]] if ai[k] >= 0 else af[k]
                b = 0.0 if pi is None else (x[pi[k]] if pi[k] >= 0 else pf[k])
                fam = 0 if family is None else family[k]
                sd = np.sqrt(a * a + (b * f) ** 2)
                if fam == 1:
                    ref = poisson.logpmf(y, f)
                elif fam == 2:
                    phi = 1.0 / b ** 2
                    ref = nbinom.logpmf(y, phi, phi / (phi + f))
                elif censor is not None and censor[e, i, k] < 0:
                    ref = norm.logcdf(y, loc=f, scale=sd)
                elif censor is not None and censor[e, i, k] > 0:
                    ref = norm.logsf(y, loc=f, scale=sd)
                else:
                    ref = norm.logpdf(y, loc=f, scale=sd)
                assert np.isfinite(ref)
                worst = max(worst, abs(ll[p, e, i, k] - ref) / max(1.0, abs(ref)))
                terms += 1
        print(f"{name}: worst |term - scipy| / max(1, |l|) = {worst:.3g} over {terms} terms")
        assert terms > 7 * 120 and worst <= 1e-11, name


def test_pit_is_the_mean_normal_cdf_on_quantified_gaussian_cells(pkg):
    from scipy.stats import norm
    um = pkg.user_models
    for name, t, obs, censor, family, noise, th, pred, _ in _cpu_cases(um):
        if name not in ("censored", "three"):
            continue
        pit = um.pointwise_pit(pred, t, obs, th, noise, censor=censor, family=family)
        ai, af, pi, pf = um.noise_layout(noise, obs.shape[2], th.shape[1])
        for e, i, k in np.ndindex(obs.shape):
            defined = not (np.isnan(t[e, i]) or np.isnan(obs[e, i, k]) or (censor is not None and censor[e, i, k] != 0) or (family is not None and family[k] != 0))
            if not defined:
                assert np.isnan(pit[e, i, k])
                continue
            a = th[:, ai[k]] if ai[k] >= 0 else af[k]
            b = 0.0 if pi is None else (th[:, pi[k]] if pi[k] >= 0 else pf[k])
            ref = np.mean(norm.cdf(obs[e, i, k], loc=pred[:, e, i, k], scale=np.sqrt(a * a + (b * pred[:, e, i, k]) ** 2)))
            assert abs(pit[e, i, k] - ref) <= 1e-14


def test_statistics_are_logsumexp_and_nanvar_with_the_edge_cells_as_defined(pkg):
    from scipy.special import logsumexp
    um = pkg.user_models
    rs = np.random.RandomState(2)
    n, cells = 501, 40
    ll = -3.0 + 4.0 * rs.standard_normal((n, cells))
    ll[rs.uniform(size=ll.shape) < 0.2] = np.nan
    ll[:, 0] = np.nan                                       # n = 0
    ll[:, 1] = np.nan
    ll[17, 1] = -2.5                                        # n = 1
    ll[:, 2] = -np.inf                                      # all -inf
    ll[:, 3] = np.where(np.arange(n) % 2 == 0, -np.inf, np.nan)
    ll[40, 3] = -7.25                                       # one finite value among -inf
    st = um.pointwise_stats(ll)
    assert st["n"][0] == 0 and all(np.isnan(st[k][0]) for k in ("max", "sum_exp", "mean", "m2", "lpd", "var"))
    assert st["n"][1] == 1 and st["max"][1] == -2.5 and st["lpd"][1] == -2.5 and st["mean"][1] == -2.5 and st["m2"][1] == 0.0 and np.isnan(st["var"][1])
    assert st["n"][2] == n and np.isneginf(st["max"][2]) and np.isneginf(st["lpd"][2]) and np.isneginf(st["mean"][2]) and np.isnan(st["m2"][2])
    assert st["max"][3] == -7.25 and st["sum_exp"][3] == 1.0 and st["lpd"][3] == -7.25 + np.log(1.0 / st["n"][3]) and np.isneginf(st["mean"][3])
    body = slice(4, None)
    m = st["n"][body]
    with np.errstate(all="ignore"):
        lse = logsumexp(np.where(np.isnan(ll), -np.inf, ll), axis=0)[body] - np.log(m)
    assert np.all(np.abs(st["lpd"][body] - lse) <= 1e-13 * np.maximum(1.0, np.abs(lse)))
    var = np.nanvar(ll[:, body], axis=0, ddof=1)
    assert np.all(np.abs(st["var"][body] - var) <= 1e-12 * var)
    # identical particles: nothing varies, elpd_waic is the sum of the terms
    same = np.tile(np.round(16.0 * (-3.0 + rs.standard_normal(cells))) / 16.0, (64, 1))      # multiples of 1/16: every sum is exact
    w = um.waic(um.pointwise_stats(same))
    assert w["p_waic"] == 0.0 and w["n_cells"] == cells and w["lppd"] == w["elpd_waic"] and abs(w["elpd_waic"] - same[0].sum()) <= cells * EPS * np.abs(same[0]).sum()
    # waic's own sums: cells with n >= 2 only
    w = um.waic(st)
    use = st["n"] >= 2
    point = (st["lpd"] - st["var"])[use]
    assert w["n_cells"] == int(use.sum()) and not use[0] and not use[1]
    assert np.isneginf(w["lppd"]) or w["lppd"] == np.sum(st["lpd"][use])
    wb = um.waic({k: v[body] for k, v in st.items()})
    pb = (st["lpd"] - st["var"])[body]
    assert wb["elpd_waic"] == wb["lppd"] - wb["p_waic"] and abs(wb["se"] - np.sqrt(pb.size * np.var(pb, ddof=1))) <= 1e-12 * wb["se"]
    assert np.array_equal(wb["pointwise"], pb) and point.size == w["n_cells"]
    # disjoint blocks merge into the whole
    pit = rs.uniform(size=cells)
    for blocks in (2, 3, 7):
        cuts = np.unique(np.concatenate([[0, n], (n * np.arange(1, blocks) * np.arange(2, blocks + 1)) // (blocks * (blocks + 1))]))
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            s = um.pointwise_stats(ll[lo:hi])
            s["pit"] = np.where(s["n"] > 0, pit, np.nan)
            parts.append(s)
        assert len(parts) == blocks
        merged = um.pointwise_merge(parts)
        _stats_agree(merged, st, ll, f"{blocks} blocks")
        assert _within(merged["lpd"], st["lpd"], 1e-12) and _within(merged["var"], st["var"], 1e-9 * np.nan_to_num(st["var"], posinf=0.0))
        assert _within(merged["pit"], np.where(st["n"] > 0, pit, np.nan), (st["n"] + 4) * EPS)


def test_reduction_rules_on_the_host_under_sanitizers(tmp_path):
    """csrc/pointwise_reduce.h as a stand-alone program: thread partials, tree and merge against long double at lengths 1, 2, 511,
    512, 513 and 70001, with NaN and -inf among the values."""
    assert shutil.which("g++"), "needs g++"
    exe = str(tmp_path / "pointwise_reduce_hostcheck")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "hostcheck", "pointwise_reduce_hostcheck.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0 and "0 failures" in run.stdout and "FAIL" not in run.stdout
    assert all(f"len {n:6d}" in run.stdout for n in (1, 2, 511, 512, 513, 70001))


def test_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc) or shutil.which(hipcc), "needs hipcc"
    run = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-fast-math", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "pointwise_kernels.hip"), "-o",
                          str(tmp_path / "pointwise_kernels.co")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    usage = {}
    name = None
    for line in run.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+(\w[\w ]*?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kernels = {k: v for k, v in usage.items() if "pw_terms_kernel" in k or "pw_cell_kernel" in k}
    print(kernels)
    assert len(kernels) == 2
    for k, v in kernels.items():
        assert v["ScratchSize"] == 0, (k, v)


# ---- GPU -----------------------------------------------------------------------------------------------------------

N_LIST = (1, 2, 63, 64, 65, 2047, 2048, 2049, 5000)
PLANTED = [("one", 1), ("one", 8), ("sigma_est", 8), ("sigma_est", 32), ("sigma_fixed", 8), ("sigma_fixed", 32), ("noise", 8),
           ("noise", 32), ("noise", 264), ("censored", 32), ("censored", 264), ("counts", 36), ("counts", 264)]


def _definition(um, pred, d, th):
    return um.pointwise_loglik(pred, d["t"], d["obs"], th, d["noise"], d["obs_scale"], d["censor"], d["family"])


def _family_of_cells(d, shape):
    """per cell a label: gaussian, left, right, poisson, negbin"""
    lab = np.full(shape, "gaussian", dtype=object)
    if d["censor"] is not None:
        lab[d["censor"] < 0], lab[d["censor"] > 0] = "left", "right"
    if d["family"] is not None:
        for k, f in enumerate(d["family"]):
            if f:
                lab[:, :, k] = "poisson" if f == 1 else "negbin"
    return lab


@pytest.mark.gpu
@pytest.mark.parametrize("name,cells", PLANTED)
def test_device_terms_are_the_definition_on_the_devices_own_predictions(pkg, name, cells):
    """Planted values: the device's ll against pointwise_loglik of the device's own pred; the NaN and -inf masks exactly equal and
    |delta| <= 1e-9 max(1, |l|) per term.  n_local = 2048, so 2049 and 5000 host particles run in chunks.
    Measured: Gaussian 4.4e-16, left 1.1e-15, right 1.0e-15, Poisson 5.5e-15, negative binomial 6.7e-15 (264 cells; 1.4e-12 with the lgamma form)."""
    um = pkg.user_models
    v = PM.VARIANTS[name]
    worst = {}
    with pkg.HipEngine(2048, v["dim"], device=0) as eng:
        eng.set_prior(PM.priors(name))
        d = PM.make(name, cells, seed=cells)
        eng.set_model_user(PM.source(name), 1, d["t"], d["obs"], cond=d["cond"], **d["kw"])
        for n in N_LIST:
            th = PM.population(name, n, seed=n, invalid=n >= 63)
            lk, pred, info = eng.predict_user(th)
            ll, info2 = eng.pointwise_loglik(th)
            assert info2 == info and info["n_failed"] == 0
            want_pred = PM.planted(name, th, d)
            assert np.array_equal(pred, want_pred, equal_nan=True)                    # the model plants what the test uploaded
            ref = _definition(um, pred, d, th).reshape(ll.shape)
            assert np.array_equal(np.isnan(ll), np.isnan(ref)) and np.array_equal(np.isneginf(ll), np.isneginf(ref)), (name, n)
            assert not np.isposinf(ll).any()
            lab = np.broadcast_to(_family_of_cells(d, ref.shape[1:])[None], ref.shape)
            fin = np.isfinite(ref)
            err = np.where(fin, np.abs(ll - np.where(fin, ref, 0.0)) / np.maximum(1.0, np.abs(np.where(fin, ref, 0.0))), 0.0)
            for f in np.unique(lab[fin]):
                worst[f] = max(worst.get(f, 0.0), float(err[(lab == f) & fin].max()))
            assert err.max() <= 1e-9, (name, n, err.max())
            if n >= 63 and name != "sigma_fixed":
                assert np.isneginf(ll).any()
            if name == "counts" and n >= 63:          # mu = 0 under y > 0 is -inf, under y = 0 it is 0
                assert np.any((ll == 0.0) & (lab == "poisson"))
    print(f"{name}, {cells} cells: worst |device - definition| / max(1, |l|) per family: " + ", ".join(f"{k} {x:.3g}" for k, x in sorted(worst.items())))


def _real_models(pkg):
    um = pkg.user_models
    rs = np.random.RandomState(8)
    n = 512
    out = {}
    t, obs = NC.make_data(1)
    scale = (1.0, 2.0)
    th = np.column_stack([rs.uniform(0.5, 1.2, n), rs.uniform(0.1, 0.6, n), rs.uniform(0.005, 0.05, n)])
    out["gaussian"] = dict(source=um.CONSECUTIVE_REACTIONS_AB, ns=2, t=t, obs=obs, th=th, censor=None, family=None,
                           noise={"additive": [("param", 2)] * 2}, obs_scale=scale, kw=dict(cond=NC.A0[:, None], obs_scale=scale))
    t, obs, censor, _ = CE.full_run_data(1)
    th = np.column_stack([th[:, :2], rs.uniform(0.005, 0.05, n), rs.uniform(0.005, 0.05, n), rs.uniform(0.0, 0.3, n)])
    out["censored"] = dict(source=um.CONSECUTIVE_REACTIONS_AB, ns=2, t=t, obs=obs, th=th, censor=censor, family=None, noise=NC.NOISE,
                           obs_scale=None, kw=dict(cond=NC.A0[:, None], noise=NC.NOISE, censor=censor))
    t, obs = CC.make_data(1)
    th = np.column_stack([th[:, :3], rs.uniform(0.02, 1.0, n)])
    out["negbin"] = dict(source=CC.source((0, 2)), ns=2, t=t, obs=obs, th=th, censor=None, family=(0, 2), noise=CC.NOISE_NB, obs_scale=None,
                         kw=dict(cond=CC.COND, noise=CC.NOISE_NB))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
@pytest.mark.parametrize("model", ["gaussian", "censored", "negbin"])
def test_real_models_sum_to_predict_users_lk(pkg, model, method):
    um = pkg.user_models
    c = _real_models(pkg)[model]
    th = c["th"]
    with pkg.HipEngine(512, th.shape[1], device=0) as eng:
        eng.set_prior({f"p{j}": {"dist": "uniform", "low": 0, "high": 10} for j in range(th.shape[1])})
        eng.set_model_user(c["source"], c["ns"], c["t"], c["obs"], method=method, **c["kw"])
        lk, pred, info = eng.predict_user(th)
        ll, info2 = eng.pointwise_loglik(th)
    assert info2 == info and info["n_failed"] == 0 and np.all(np.isfinite(lk))
    total = np.nansum(ll, axis=(1, 2, 3))
    err = np.max(np.abs(total - lk) / np.maximum(1.0, np.abs(lk)))
    ref = um.pointwise_loglik(pred, c["t"], c["obs"], th, c["noise"], c["obs_scale"], c["censor"], c["family"])
    assert np.array_equal(np.isnan(ll), np.isnan(ref))
    term = np.nanmax(np.abs(ll - ref) / np.maximum(1.0, np.abs(ref)))
    print(f"{model} {method}: worst |nansum(ll) - lk| / max(1, |lk|) = {err:.3g}, worst term against the definition {term:.3g}")
    assert err <= 1e-9 and term <= 1e-9


def _summary_checks(pkg, eng, d, th, which, what):
    um = pkg.user_models
    n = th.shape[0]
    eng.upload_particles(which, th)
    got = eng.pointwise_summary(which)
    ll, _ = eng.pointwise_loglik(eng.download_particles(which))
    _, pred, _ = eng.predict_user(th)
    want = um.pointwise_stats(ll)
    _stats_agree(got, want, ll, what)
    assert _within(got["lpd"], want["lpd"], 1e-12 * np.maximum(1.0, np.abs(np.nan_to_num(want["lpd"], neginf=0.0)))) and np.array_equal(np.isnan(got["var"]), np.isnan(want["var"])), what
    pit = um.pointwise_pit(pred, d["t"], d["obs"], th, d["noise"], d["obs_scale"], d["censor"], d["family"])
    assert _within(got["pit"], pit, (n + 4) * EPS), what
    w = um.waic(got)
    assert all(np.array_equal(np.asarray(got["waic"][k]), np.asarray(w[k]), equal_nan=True) for k in w), what
    return got, want, pit


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 65, 2049, 70001])
def test_summary_is_numpy_on_the_devices_own_terms(pkg, n):
    """Only the reduction is under test: pointwise_summary against pointwise_stats of the downloaded ll of the same set; the PIT
    against NumPy's Phi on the device's pred.  Cells with 0, 1, 2, 3 finite particles sit next to full ones; with every Poisson mean
    0 the cells of a positive count are all -inf."""
    name, cells = "counts", 36
    d = PM.make(name, cells, seed=3)
    m = PM.finite(d, n)
    with pkg.HipEngine(n, PM.VARIANTS[name]["dim"], device=0) as eng:
        eng.set_prior(PM.priors(name))
        eng.set_model_user(PM.source(name), 1, d["t"], d["obs"], cond=d["cond"], **d["kw"])
        th = PM.population(name, n, seed=n + 1)
        got, want, pit = _summary_checks(pkg, eng, d, th, pkg.SMC_SET_FILT, f"n = {n}")
        shape = d["obs"].shape
        assert got["n"].shape == shape and got["n_failed"] == 0 and got["kernel_ms"]["pointwise"] > 0
        seen = ~np.isnan(d["obs"]) & ~np.isnan(d["t"])[:, :, None]
        assert np.array_equal(got["n"], np.where(seen, m[:, None, None], 0))      # the gates' counts, cell by cell
        assert set(np.unique(got["n"])) >= {0, min(1, n), min(2, n), min(3, n), n}
        assert np.all(np.isnan(got["pit"][~seen])) and np.all(np.isnan(got["pit"][:, :, 1:]))
        full = seen[:, :, 0] & (m[:, None] > 0)
        assert np.all((got["pit"][:, :, 0][full] >= 0) & (got["pit"][:, :, 0][full] <= 1))
        th0 = th.copy()
        th0[:, 1] = 0.0
        got0, want0, _ = _summary_checks(pkg, eng, d, th0, pkg.SMC_SET_PRED, f"n = {n}, Poisson means 0")
        dead = seen[:, :, 1] & (d["obs"][:, :, 1] > 0) & (m[:, None] > 0)
        assert dead.any() and np.all(np.isneginf(got0["max"][:, :, 1][dead])) and np.all(np.isneginf(got0["lpd"][:, :, 1][dead]))
        assert np.all(np.isnan(got0["sum_exp"][:, :, 1][dead]))


@pytest.mark.gpu
def test_closed_form_of_the_constant_model_at_65536_particles(pkg):
    """Particles iid N(m, v), the constant model with sigma fixed: lpd_c within 5 standard errors of log N(y_c; m, sigma^2 + v),
    se = sqrt((E[p^2] - E[p]^2) / n) / E[p] with E[p^2] = N(y; m, sigma^2 / 2 + v) / (2 sigma sqrt pi); pit_c within 5 x 0.5 / sqrt n
    of Phi((y_c - m) / sqrt(sigma^2 + v)).  In NumPy alone the worst over 200 seeds x 4 cells is 3.1 se."""
    from scipy.stats import norm
    n, m, v, sigma = 65536, 0.3, 0.04, 0.1
    y = np.array([[0.3, 0.5, 0.9, -0.2]])
    src = ("__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = 0.0; }\n"
           "__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) { dydt[0] = 0.0; }\n"
           "__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return theta[0]; }\n")
    th = m + np.sqrt(v) * np.random.RandomState(20240531).standard_normal((n, 1))
    with pkg.HipEngine(n, 1, device=0) as eng:
        eng.set_prior({"mu": {"dist": "uniform", "low": -10, "high": 10}})
        eng.set_model_user(src, 1, np.arange(4.0)[None, :], y, est_sigma=False, sigma_fixed=sigma)
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        got = eng.pointwise_summary()
    assert got["n"].shape == (1, 4, 1) and np.all(got["n"] == n)
    p1 = norm.pdf(y, m, np.sqrt(sigma ** 2 + v))
    p2 = norm.pdf(y, m, np.sqrt(sigma ** 2 / 2 + v)) / (2 * sigma * np.sqrt(np.pi))
    se = np.sqrt((p2 - p1 ** 2) / n) / p1
    dl = (got["lpd"][0, :, 0] - np.log(p1[0])) / se[0]
    dp = got["pit"][0, :, 0] - norm.cdf((y[0] - m) / np.sqrt(sigma ** 2 + v))
    print(f"lpd off by {np.abs(dl).max():.3g} se (bound 5), pit off by {np.abs(dp).max():.3g} (bound {2.5 / np.sqrt(n):.3g})")
    assert np.abs(dl).max() <= 5 and np.abs(dp).max() <= 5 * 0.5 / np.sqrt(n)


_KEYS = ("n", "max", "sum_exp", "mean", "m2", "pit", "lpd", "var")


def _same_bits(a, b):
    return all(_bits(a[k], b[k]) for k in _KEYS)


@pytest.mark.gpu
def test_staging_groups_repeats_untouched_sets_and_refusals(pkg):
    name, cells, n = "noise", 264, 3000
    d = PM.make(name, cells, seed=4)
    th = PM.population(name, n, seed=9)
    with pkg.HipEngine(n, 6, device=0) as eng:
        with pytest.raises(pkg.SmcError, match="no user model has been set"):
            eng.pointwise_summary()
        with pytest.raises(pkg.SmcError, match="no user model has been set"):
            eng.pointwise_loglik(th)
        nn = np.empty(cells, dtype=np.int64)
        a = [np.empty(cells) for _ in range(5)]
        i64p = ctypes.POINTER(ctypes.c_int64)
        assert eng.L.smc_user_pointwise_summary(eng.ctx, pkg.SMC_SET_FILT, 0, nn.ctypes.data_as(i64p), *[_dp(x) for x in a], None, None, None) != 0
        assert "smc_user_pointwise_summary: no user model has been set" in eng.L.smc_last_error(eng.ctx).decode()
        assert eng.L.smc_user_pointwise(eng.ctx, _dp(th), n, _dp(np.empty((n, cells))), None, None) != 0
        assert "smc_user_pointwise: no user model has been set" in eng.L.smc_last_error(eng.ctx).decode()
        eng.set_prior(PM.priors(name))
        eng.set_model_user(PM.source(name), 1, d["t"], d["obs"], cond=d["cond"], **d["kw"])
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        eng.loglik(pkg.SMC_SET_PRED)
        eng.upload_particles(pkg.SMC_SET_FILT, th[::-1].copy())
        eng.upload_lk(pkg.SMC_SET_FILT, eng.download_lk(pkg.SMC_SET_PRED)[::-1].copy())

        def state():
            return [eng.download_particles(pkg.SMC_SET_PRED), eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_PRED),
                    eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags().astype(np.float64)]
        before = state()
        one = eng.pointwise_summary()
        again = eng.pointwise_summary()
        assert _same_bits(one, again)                                                   # a repeated call: the same bits
        with pytest.raises(pkg.SmcError, match=r"smc_user_pointwise_summary: one experiment of the design needs \d+ B of staging") as e:
            eng.pointwise_summary(max_staging_bytes=1)
        assert "max_staging_bytes allows 1 B" in str(e.value)
        need = int(re.search(r"needs (\d+) B", str(e.value)).group(1))
        n_t, n_obs = d["t"].shape[1], 2
        assert 2 * n * n_t * n_obs * 8 <= need <= (2 + 1 / 8) * n * n_t * n_obs * 8 + n * 40 + cells * 48 + 4096
        grouped = eng.pointwise_summary(max_staging_bytes=need)                         # room for one experiment, not for two
        assert _same_bits(one, grouped)
        with pytest.raises(pkg.SmcError, match=rf"needs {need} B"):
            eng.pointwise_summary(max_staging_bytes=need - 1)
        pred_set = eng.pointwise_summary(pkg.SMC_SET_PRED)
        for k in ("max", "n"):                                                          # the other set: the same particles in reverse order
            assert _bits(pred_set[k], one[k])
        after = state()
        for x, y in zip(before, after):
            assert _bits(x, y)
        with pytest.raises(pkg.SmcError, match="set must be SMC_SET_PRED or SMC_SET_FILT"):
            eng.pointwise_summary(which=7)
        assert eng.L.smc_user_pointwise_summary(eng.ctx, pkg.SMC_SET_FILT, 0, nn.ctypes.data_as(i64p), *[_dp(x) for x in a[:4]], None, None, None, None) != 0
        assert "smc_user_pointwise_summary: NULL result array" in eng.L.smc_last_error(eng.ctx).decode()
        assert eng.L.smc_user_pointwise(eng.ctx, _dp(th), n, None, None, None) != 0
        assert "smc_user_pointwise: NULL result array" in eng.L.smc_last_error(eng.ctx).decode()
        with pytest.raises(ValueError, match="particles must be"):
            eng.pointwise_loglik(th[:, :3])


@pytest.mark.gpu
def test_full_run_returns_the_posteriors_pointwise_statistics(pkg):
    um = pkg.user_models
    t, obs = NC.make_data(0)
    n = 4096
    pri = {"k1": {"dist": "uniform", "low": 0, "high": 3}, "k2": {"dist": "uniform", "low": 0, "high": 3}, "sigma": {"dist": "uniform", "low": 0, "high": 0.5}}
    s = pkg.SMCSettings(n_particle=n, priors=pri)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(pri)
        eng.set_model_user(um.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None])
        out = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3, pointwise=True)
        after = eng.pointwise_summary(pkg.SMC_SET_PRED)
        plain = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3)
        with pytest.raises(ValueError, match="user model"):
            eng.model = ("mm", 4, 30)
            pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3, pointwise=True)
    assert out["gamma"] == 1.0 and "pointwise" not in plain and set(out) == set(plain) | {"pointwise"}
    assert np.array_equal(out["p_pred"], plain["p_pred"]) and out["logZ"] == plain["logZ"]
    pw = out["pointwise"]
    assert _same_bits(pw, after)
    w = um.waic(pw)
    assert all(np.array_equal(np.asarray(pw["waic"][k]), np.asarray(w[k]), equal_nan=True) for k in w)
    seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
    assert w["n_cells"] == int(seen.sum()) and np.all(pw["n"][seen] == n) and np.isfinite(w["elpd_waic"]) and 0 < w["p_waic"] < 10
    pit = pw["pit"][seen]
    print(f"elpd_waic {w['elpd_waic']:.2f} +- {w['se']:.2f}, p_waic {w['p_waic']:.2f}, PIT histogram {np.histogram(pit, 10, (0, 1))[0]}")
    assert np.all((pit > 0) & (pit < 1)) and 0.3 < pit.mean() < 0.7


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_merge_into_the_one_rank_statistics(pkg, world):
    """run_smc's path for several ranks (rank threads on one GPU, the arrangement of tests/test_user_sharded.py): every rank's block
    statistics allgathered and merged in rank order equal the one-rank statistics of the same uploaded population."""
    from _thread_comm import ThreadWorld
    driver = sys.modules[pkg.__name__ + ".driver"]
    name, cells, n = "counts", 36, 6144
    d = PM.make(name, cells, seed=6)
    th = PM.population(name, n, seed=12)

    def engine(n_local):
        e = pkg.HipEngine(n_local, 6, device=0, n_global=n)
        e.set_prior(PM.priors(name))
        e.set_model_user(PM.source(name), 1, d["t"], d["obs"], cond=d["cond"], **d["kw"])
        return e
    with engine(n) as eng:
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        ref = eng.pointwise_summary(pkg.SMC_SET_PRED)
        ll, _ = eng.pointwise_loglik(th)
    nl = n // world
    tw = ThreadWorld(world)
    engines = [engine(nl) for _ in range(world)]
    outs, errs = [None] * world, []

    def work(r):
        try:
            engines[r].upload_particles(pkg.SMC_SET_PRED, np.ascontiguousarray(th[r * nl:(r + 1) * nl]))
            outs[r] = driver._pointwise_all_ranks(engines[r], tw.comm(r), {"which": pkg.SMC_SET_PRED})
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            tw.barrier.abort()
    ths = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    for e in engines:
        e.close()
    if errs:
        raise errs[0]
    for r in range(world):
        _stats_agree(outs[r], ref, ll, f"rank {r} of {world}")
        assert _within(outs[r]["pit"], ref["pit"], (ref["n"] + 4) * EPS)
        assert _same_bits(outs[r], outs[0])                                    # every rank returns the same whole
        assert outs[r]["n_failed"] == 0
        w = pkg.user_models.waic(outs[r])
        assert all(np.array_equal(np.asarray(outs[r]["waic"][k]), np.asarray(w[k]), equal_nan=True) for k in w)
    assert set(np.unique(ref["n"])) >= {0, 1, 2, 3, 40, n}
