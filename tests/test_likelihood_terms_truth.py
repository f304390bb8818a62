"""Every kind of likelihood term of a user model - Gaussian with additive and proportional noise, left- and right-censored,
Poisson, negative binomial, and the Poisson floor - against its mathematical value at 60 digits (tests/likelihood_terms_truth.py:
the grids, the planted models and the formulas; tests/golden/likelihood_terms_truth.npz: the values, written with mpmath), under
ONE bar for the NumPy definitions, the C text on the host and the device:

    |term - truth| <= 1e-11 max(1, |truth|);   a sum (a particle's lk) within the sum of its terms' bars.

The other tests of these terms compare the device with the definitions of user_models.py, which follow the kernels operation for
operation: they pin the transcription and cannot see an error of the formula.  For b in {1e-7, 1e-8} (record only: phi + y no
longer holds y) the negative binomial is asserted finite and >= 0, and its error printed.

CPU: the fixture against its generator (mpmath, if present); count_floor, count_excess, censor_excess, noise_loglik and
pointwise_loglik against the fixture; csrc/user_censor.h, csrc/user_count.h and csrc/count_floor.h as a stand-alone program under
-fsanitize=address,undefined against the fixture.
GPU: every term through the pointwise path (the hipcc-compiled text, csrc/pointwise_kernels.hip: pw_term) and every particle's lk
through the run-time compiled solve kernels, RK45 (fused expressions) and BDF (every operation rounded alone); loglik and
predict_user give the same bits.

Measured, worst error / max(1, |truth|) per family and path (NumPy 2.2, SciPy 1.15, glibc; MI355X):
                                     definitions   C text, host   device, pointwise path
    count_floor                      1.7e-15       3.7e-15        (host code: the off-experiment Poisson cells, under the bar)
    Poisson excess / term            7.9e-15       7.9e-15        7.9e-15
    negative binomial, b >= 1e-6     3.3e-14       3.3e-14        3.3e-14   (worst at b = 1e-5; b >= 0.01: 5.6e-15)
      record only, b = 1e-7 / 1e-8   6.1e-13 / 1.0e-10   the same   the same
    censored, left and right         7.8e-16       3.4e-16        3.4e-16
    Gaussian                         1.6e-16       -              1.6e-16
  lk through the solve kernels, worst share of the sum of the terms' bars, the same under RK45 and BDF: Poisson 1e-3, negative
  binomial 3.3e-3 (b >= 1e-6; 0.021 at b = 1e-7, 3.2 at b = 1e-8), censored 5.6e-5, Gaussian 3.8e-5.
  The device's lgamma, log, log1p, erfc and erfcx leave every path where the C library leaves it: no work-round was needed.
The forms this replaced (user_models.py of the parent commit against the same fixture): Poisson y (d - log1p(d)) 9.2e-10 at
y = 2^53, mu = y (1 - 1e-9), two entries over the bar; the negative binomial's lgamma differences over the bar in 32 to 149 of
the 192 entries of every b - a relative error of 0.3 to 1 at y = 2^53 for every b, 1.2e-10 to 2.9e-10 at y = 1e6, and
2.2e-7 / 1.8e-5 / 4.7e-3 absolute at b = 1e-4 / 1e-5 / 1e-6 with y = 1 ... 7 and mu = y."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import likelihood_terms_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_BAR = T.B.size - T.N_B_RECORD
WIDE = {f"p{j}": {"dist": "uniform", "low": -1e300, "high": 1e300} for j in range(4)}


@pytest.fixture(scope="module")
def fx():
    return T.load()


def _inf_masks_agree(got, truth):
    return np.array_equal(np.isposinf(got), np.isposinf(truth)) and np.array_equal(np.isneginf(got), np.isneginf(truth)) and not np.isnan(got).any()


def _check_negbin(what, nb, fx):
    """nb (y, f, b), minus the log-pmf, against the fixture: the infinities exactly, the bar down to b = 1e-6, the record-only b
    finite (or the stated +inf) and >= 0, their error printed"""
    assert _inf_masks_agree(nb, fx["nb_x"]), what
    e = T.rel(nb, fx["nb_x"])
    print(f"{what}: negative binomial per b " + ", ".join(f"{b:g}: {v:.3g}" for b, v in zip(T.B, e.max(axis=(0, 1)))))
    j, i, k = np.unravel_index(np.argmax(e[:, :, :N_BAR]), e[:, :, :N_BAR].shape)
    assert e[:, :, :N_BAR].max() <= T.BAR, (what, T.Y[j], T.MU[j, i], T.B[k], e[j, i, k])
    assert np.all(nb[:, :, N_BAR:] >= 0.0), what


def _check_counts(what, floor, pois, nb, fx):
    """floor (y,), pois (y, f) the Poisson excess, nb (y, f, b) against the fixture"""
    e_floor, e_pois = T.rel(floor, fx["floor"]).max(), T.rel(pois, fx["pois_x"])
    print(f"{what}: floor {e_floor:.3g}, Poisson {e_pois.max():.3g}")
    assert _inf_masks_agree(pois, fx["pois_x"]) and e_floor <= T.BAR, what
    j, i = np.unravel_index(np.argmax(e_pois), e_pois.shape)
    assert e_pois.max() <= T.BAR, (what, T.Y[j], T.MU[j, i], e_pois.max())
    _check_negbin(what, nb, fx)


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_fixture_holds_the_grids_and_is_small(fx):
    assert {k: v.shape for k, v in fx.items()} == T.shapes() and all(v.dtype == np.float64 for v in fx.values())
    assert os.path.getsize(T.FIXTURE) < 64 * 1024
    dead = (T.MU == 0.0) & (T.Y[:, None] > 0)
    assert np.array_equal(np.isposinf(fx["pois_x"]), dead) and np.array_equal(np.isposinf(fx["nb_x"]), np.broadcast_to(dead[:, :, None], fx["nb_x"].shape))
    assert np.array_equal(np.isneginf(fx["pois_lk"]), dead) and not any(np.isnan(v).any() for v in fx.values())
    assert np.all(fx["pois_x"][1:, T.F_ONE] == 0.0) and fx["floor"][0] == 0.0 and np.all(fx["pois_x"][0] == T.F)
    for n in range(len(T.SCALES)):
        th, j = T.gc_particles(T.SCALES[n])
        assert np.all(np.isfinite(fx[f"gc_lk_{n}"])) and np.all(fx[f"gc_l_{n}"] <= 0.0) and set(j) == {T.LEFT, T.RIGHT, T.GAUSS}
        assert fx[f"gc_l_{n}"].min() < -4e307 and np.sum(fx[f"gc_l_{n}"][j != T.GAUSS] == 0.0) >= 2 * 2 * len(T.RATIOS)      # z = -1e154; z >= 40


def test_fixture_against_its_generator(fx):
    """a fixed sample of 200 entries, recomputed with mpmath: the same bits"""
    pytest.importorskip("mpmath")
    picks = T.sample(200)
    assert len(picks) == 200 and {nm for nm, _ in picks} == set(fx)
    bad = [(nm, idx) for nm, idx in picks if np.float64(T.entry(nm, idx)).tobytes() != fx[nm][idx].tobytes()]
    assert not bad, bad[:5]


def test_count_definitions_meet_the_bar(pkg, fx):
    um = pkg.user_models
    y = T.Y
    _check_counts("definitions", um.count_floor(y), um.count_excess(y[:, None], T.MU, 0.0, 1),
                  um.count_excess(y[:, None, None], T.MU[:, :, None], T.B[None, None, :], 2), fx)
    # the same through pointwise_loglik on the planted predictions, and its sums
    t, obs, cond = T.count_data()
    for family, noise, x in ((1, {"additive": [("fixed", 1.0)]}, fx["pois_x"] + fx["floor"][:, None]), (2, T.NOISE_NB, fx["nb_x"])):
        th, j = T.count_particles(family)
        ll = um.pointwise_loglik(T.count_planted(th), t, obs, th, noise, family=(family,))[:, :, 1, 0]
        own = ll[T.mask(j, y.size)].reshape(x.shape)
        keep = (slice(None),) * 2 + ((slice(0, N_BAR),) if family == 2 else ())
        assert _inf_masks_agree(own, -x) and T.rel(own, -x)[keep].max() <= T.BAR, family
        name = "pois" if family == 1 else "nb"
        lk = ll.sum(axis=1).reshape(x.shape)
        assert _inf_masks_agree(lk, fx[name + "_lk"]), family
        with np.errstate(invalid="ignore"):
            assert np.all((np.abs(lk - fx[name + "_lk"]) <= fx[name + "_bar"])[keep] | np.isinf(lk)[keep]), family


def _gc_z(th, j, s):
    """z of the censored particles as pw_term forms it"""
    f, a, b = th[:, 0], th[:, 1], th[:, 2]
    r = np.where(j == T.LEFT, T.L_CENS, -T.L_CENS) - f
    return np.where(j == T.LEFT, r, -r) / np.sqrt((a * s) ** 2 + (b * f) ** 2)


def test_censored_and_gaussian_definitions_meet_the_bar(pkg, fx):
    um = pkg.user_models
    t, obs, censor, cond = T.gc_data()
    for n, s in enumerate(T.SCALES):
        th, j = T.gc_particles(s)
        truth, cens, gauss = fx[f"gc_l_{n}"], j != T.GAUSS, j == T.GAUSS
        z = _gc_z(th, j, s)[cens]
        assert z.min() == -1e154 and np.any(z == 40.0) and np.any((z == 0.0) & np.signbit(z)) and np.any((z == 0.0) & ~np.signbit(z))
        e_cens = T.rel(-um.censor_excess(z), truth[cens]).max()
        pred = T.gc_planted(th)
        g = um.noise_loglik(pred[gauss][:, 2:], t[2:], obs[2:], th[gauss], T.NOISE_GC, (s,))
        e_gauss = T.rel(g, truth[gauss]).max()
        ll = um.pointwise_loglik(pred, t, obs, th, T.NOISE_GC, (s,), censor)[:, :, 1, 0]
        e_pw = T.rel(ll[T.mask(j, 3)], truth).max()
        e_lk = np.max(np.abs(ll.sum(axis=1) - fx[f"gc_lk_{n}"]) / fx[f"gc_bar_{n}"])
        print(f"obs_scale {s}: censor_excess {e_cens:.3g}, noise_loglik {e_gauss:.3g}, pointwise_loglik {e_pw:.3g}, sums {e_lk:.3g} of their bars")
        assert e_cens <= T.BAR and e_gauss <= T.BAR and e_pw <= T.BAR and e_lk <= 1.0
        off = ~T.mask(j, 3)
        assert np.all(ll[:, :2][off[:, :2]] == 0.0)                  # off its experiment a particle's censored terms are exactly 0


def test_the_c_text_on_the_host_under_sanitizers(fx, tmp_path):
    """csrc/user_censor.h, csrc/user_count.h and csrc/count_floor.h as a program of their own (g++, sanitizers, no contraction):
    every count entry of the fixture and every censored z, passed as a binary file."""
    assert shutil.which("g++"), "needs g++"
    exe = str(tmp_path / "likelihood_terms_hostcheck")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "hostcheck", "likelihood_terms_hostcheck.cpp")], check=True)
    y, mu, b = np.broadcast_arrays(T.Y[:, None, None], T.MU[:, :, None], T.B[None, None, :])
    zs = [_gc_z(*T.gc_particles(s), s)[T.gc_particles(s)[1] != T.GAUSS] for s in T.SCALES]
    rec = np.concatenate([
        np.column_stack([np.zeros(T.Y.size), T.Y, np.zeros(T.Y.size), np.zeros(T.Y.size)]),
        np.column_stack([np.ones(T.MU.size), y[:, :, 0].ravel(), mu[:, :, 0].ravel(), np.zeros(T.MU.size)]),
        np.column_stack([np.full(y.size, 2.0), y.ravel(), mu.ravel(), (b * b).ravel()]),
        np.column_stack([np.full(sum(z.size for z in zs), 3.0), np.concatenate(zs), np.zeros((sum(z.size for z in zs), 2))])])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    rec.astype("<f8").tofile(src)
    run = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert run.returncode == 0 and f"{rec.shape[0]} terms" in run.stderr, run.stderr[-3000:]
    out = np.fromfile(dst, dtype="<f8")
    assert out.size == rec.shape[0]
    n0, n1, n2 = T.Y.size, T.Y.size + T.MU.size, T.Y.size + T.MU.size + y.size
    _check_counts("host program", out[:n0], out[n0:n1].reshape(T.MU.shape), out[n1:n2].reshape(y.shape), fx)
    at = n2
    for n, s in enumerate(T.SCALES):
        cens = T.gc_particles(s)[1] != T.GAUSS
        e = T.rel(-out[at:at + zs[n].size], fx[f"gc_l_{n}"][cens]).max()
        print(f"host program, obs_scale {s}: censor_excess {e:.3g}")
        assert e <= T.BAR
        at += zs[n].size


# ---- GPU -----------------------------------------------------------------------------------------------------------

_RUNS = {}


def _run(pkg, key, source, th, method, **kw):
    """One engine per (model, method), shared by the tests: the device's pred and pointwise terms, and lk from a sweep and from
    predict_user.  At most 2048 particles at a time."""
    if (key, method) in _RUNS:
        return _RUNS[key, method]
    n = th.shape[0]
    parts = -(-n // 2048)
    size = -(-n // parts)
    out = {"lk": [], "lk_sweep": [], "pred": [], "ll": []}
    with pkg.HipEngine(size, th.shape[1], device=0) as eng:
        eng.set_prior({k: WIDE[k] for k in list(WIDE)[:th.shape[1]]})
        eng.set_model_user(source, 1, method=method, **kw)
        for p in range(parts):
            chunk = th[p * size:(p + 1) * size]
            m = chunk.shape[0]
            chunk = np.concatenate([chunk, np.repeat(chunk[-1:], size - m, axis=0)])
            eng.upload_particles(pkg.SMC_SET_PRED, chunk)
            eng.loglik(pkg.SMC_SET_PRED)
            out["lk_sweep"].append(eng.download_lk(pkg.SMC_SET_PRED)[:m])
            lk, pred, _ = eng.predict_user(chunk)
            ll, _ = eng.pointwise_loglik(chunk)
            out["lk"].append(lk[:m])
            out["pred"].append(pred[:m])
            out["ll"].append(ll[:m])
    _RUNS[key, method] = {k: np.concatenate(v) for k, v in out.items()}
    return _RUNS[key, method]


def _count_run(pkg, family, method):
    """the grid's particles and three more: a NaN mean, a negative mean, and an overdispersion of 0"""
    th, j = T.count_particles(family)
    th = np.concatenate([th, [[np.nan, 0.3, 1.0], [-1.0, 0.3, 1.0], [2.0, 0.0, 1.0]]])
    t, obs, cond = T.count_data()
    kw = dict(t=t, obs=obs, cond=cond, est_sigma=False, noise=None if family == 1 else T.NOISE_NB)
    return th, j, _run(pkg, f"count{family}", T.count_source(family), th, method, **kw)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("family", [1, 2], ids=["poisson", "negbin"])
def test_device_count_terms_through_the_pointwise_path(pkg, fx, family):
    th, j, run = _count_run(pkg, family, "RK45")
    n = j.size
    assert np.array_equal(run["pred"][:, :, 1:], T.count_planted(th)[:, :, 1:], equal_nan=True)      # the model plants what was uploaded
    ll = run["ll"][:, :, 1, 0]
    assert np.all(np.isnan(run["ll"][:, :, 0])) and not np.isposinf(ll).any()
    assert np.array_equal(np.isnan(ll[n:]), [[e == 1 for e in range(T.Y.size)], [False] * T.Y.size, [False] * T.Y.size])
    assert np.isneginf(ll[n + 1, 1]) and (np.all(np.isneginf(ll[n + 2])) if family == 2 else np.isfinite(ll[n + 2]).all())
    own = ll[:n][T.mask(j, T.Y.size)]
    if family == 1:
        x = (fx["pois_x"] + fx["floor"][:, None])
        assert _inf_masks_agree(own.reshape(x.shape), -x)
        e = T.rel(own.reshape(x.shape), -x)
        print(f"device, pointwise path: Poisson term {e.max():.3g}")
        assert e.max() <= T.BAR, (np.unravel_index(np.argmax(e), e.shape), e.max())
        off = ll[:n][~T.mask(j, T.Y.size)].reshape(n, -1)                      # off its experiment: the floor alone
        assert T.rel(off, -np.array([np.delete(fx["floor"], q) for q in j])).max() <= T.BAR
    else:
        _check_negbin("device, pointwise path", -own.reshape(fx["nb_x"].shape), fx)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
@pytest.mark.parametrize("family", [1, 2], ids=["poisson", "negbin"])
def test_device_count_lk_through_the_solve_kernels(pkg, fx, family, method):
    th, j, run = _count_run(pkg, family, method)
    n = j.size
    assert _same_bits(run["lk"], run["lk_sweep"])
    assert np.array_equal(run["pred"][:, :, 1:], T.count_planted(th)[:, :, 1:], equal_nan=True)
    name = "pois" if family == 1 else "nb"
    truth, bars = fx[name + "_lk"], fx[name + "_bar"]
    lk = run["lk"][:n].reshape(truth.shape)
    assert np.isnan(run["lk"][n]) and np.isneginf(run["lk"][n + 1]) and (family == 1 or np.isneginf(run["lk"][n + 2]))
    assert _inf_masks_agree(lk, truth)
    with np.errstate(invalid="ignore"):
        share = np.where(np.isinf(truth), 0.0, np.abs(lk - truth) / bars)
    per_b = share.max(axis=(0, 1)) if family == 2 else share.max()
    print(f"device, {method}: {name} lk, worst share of the bar {np.array2string(np.asarray(per_b), precision=3)}")
    assert (share if family == 1 else share[:, :, :N_BAR]).max() <= 1.0, np.unravel_index(np.argmax(share), share.shape)
    if family == 2:
        assert np.all(lk[np.isfinite(truth)] <= 0.0)                  # every excess clamped at >= 0, and no floor


def _gc_run(pkg, n, method):
    """the grid's particles and two more: a NaN prediction in the left-censored cell, and a = 0"""
    s = T.SCALES[n]
    th, j = T.gc_particles(s)
    th = np.concatenate([th, [[np.nan, 0.7, 0.1, 0.0], [1.0, 0.0, 0.1, 2.0]]])
    t, obs, censor, cond = T.gc_data()
    return th, j, _run(pkg, f"gc{n}", T.gc_source(), th, method, t=t, obs=obs, cond=cond, noise=T.NOISE_GC, obs_scale=(s,), censor=censor)


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(T.SCALES)), ids=[f"scale{s}" for s in T.SCALES])
def test_device_censored_and_gaussian_terms_through_the_pointwise_path(pkg, fx, n):
    th, j, run = _gc_run(pkg, n, "RK45")
    m = j.size
    assert np.array_equal(run["pred"][:, :, 1:], T.gc_planted(th)[:, :, 1:], equal_nan=True)
    ll = run["ll"][:, :, 1, 0]
    assert np.all(np.isnan(run["ll"][:, :, 0])) and not np.isposinf(ll).any()
    assert np.array_equal(np.isnan(ll[m:]), [[True, False, False], [False] * 3]) and np.all(np.isneginf(ll[m + 1])) and not np.isinf(ll[:m]).any()
    e = T.rel(ll[:m][T.mask(j, 3)], fx[f"gc_l_{n}"])
    worst = {k: e[j == q].max() for k, q in (("left", T.LEFT), ("right", T.RIGHT), ("Gaussian", T.GAUSS))}
    print(f"device, pointwise path, obs_scale {T.SCALES[n]}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert e.max() <= T.BAR, (th[np.argmax(e)], e.max())
    assert np.all(ll[:m, :2][~T.mask(j, 3)[:, :2]] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
@pytest.mark.parametrize("n", range(len(T.SCALES)), ids=[f"scale{s}" for s in T.SCALES])
def test_device_censored_and_gaussian_lk_through_the_solve_kernels(pkg, fx, n, method):
    th, j, run = _gc_run(pkg, n, method)
    m = j.size
    assert _same_bits(run["lk"], run["lk_sweep"])
    assert np.array_equal(run["pred"][:, :, 1:], T.gc_planted(th)[:, :, 1:], equal_nan=True)
    lk = run["lk"][:m]
    assert np.isnan(run["lk"][m]) and np.isneginf(run["lk"][m + 1]) and np.all(np.isfinite(lk))
    share = np.abs(lk - fx[f"gc_lk_{n}"]) / fx[f"gc_bar_{n}"]
    worst = {k: share[j == q].max() for k, q in (("left", T.LEFT), ("right", T.RIGHT), ("Gaussian", T.GAUSS))}
    print(f"device, {method}, obs_scale {T.SCALES[n]}: lk, worst share of the bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert share.max() <= 1.0, (th[np.argmax(share)], share.max())
