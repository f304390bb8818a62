"""User models with a noise model (include/smc_hip.h: smc_set_model_user4): a noise level per output and a proportional part,
sd_ik^2 = (a_k s_k)^2 + (b_k f_ik)^2.  CPU part: the kernels compile in both variants, the rules of a specification in the library
and in NumPy, user_models.noise_loglik against a plain loop and against the single-sigma formula, the sign of the excess terms.
GPU part: the likelihood against noise_loglik of the engine's own predictions, the equivalences with the smc_set_model_user3
path, exact early rejection, predictive noise, a full run against a Metropolis chain on the closed form
(tests/noise_model_chain.py), and the LDS refusal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import noise_model_chain as NC
from test_k8_uniform_control import _innermost_loop

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-fast-math"]   # csrc/Makefile
RK45, BDF = 0, 1
NAMES = ("k1", "k2", "a0", "a1", "b0")
PRIORS = {nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(NAMES, NC.PRIOR_HIGH)}
ADD_ONLY = {"additive": NC.NOISE["additive"]}
# the reference posterior for data seed 0: `python tests/noise_model_chain.py 0 250000` (acceptance 0.267; the means of the two
# half chains differ by at most 0.03 sd; the truth lies within 1.5 sd)
CHAIN_MEAN = np.array([0.79228, 0.29754, 0.01138, 0.02025, 0.07783])
CHAIN_SD = np.array([0.00623, 0.00172, 0.00107, 0.00153, 0.01294])


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _fp(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_noise_sources_compile_with_and_without_the_proportional_part(pkg):
    um = pkg.user_models
    for src, ns, method in ((um.CONSECUTIVE_REACTIONS_AB, 2, RK45), (um.CONSECUTIVE_REACTIONS_AB, 2, BDF), (um.ROBERTSON_AC, 3, BDF)):
        for prop in (0, 1):
            log = ctypes.create_string_buffer(16384)
            rc = pkg.lib().smc_user_model_check4(src.encode(), ns, 5, method, 2, prop, log, 16384)
            assert rc == 0, (ns, method, prop, log.value.decode(errors="replace"))
    assert pkg.lib().smc_user_model_check4(um.CONSECUTIVE_REACTIONS_AB.encode(), 2, 5, RK45, 9, 0, None, 0) == 2


BAD_SPECS = [      # (additive, proportional or None, a word of the reason)
    ([("param", 5), ("param", 3)], None, "add_index"),
    ([("param", -2), ("param", 3)], None, "add_index"),
    ([("fixed", 0.0), ("param", 3)], None, "add_fixed"),
    ([("fixed", -0.1), ("param", 3)], None, "add_fixed"),
    ([("fixed", np.nan), ("param", 3)], None, "add_fixed"),
    ([("fixed", np.inf), ("param", 3)], None, "add_fixed"),
    ([("param", 2), ("param", 3)], [("param", 7), ("fixed", 0.0)], "prop_index"),
    ([("param", 2), ("param", 3)], [("fixed", -1e-3), ("fixed", 0.0)], "prop_fixed"),
    ([("param", 2), ("param", 3)], [("fixed", np.nan), ("fixed", 0.0)], "prop_fixed"),
]


def _raw(entries):
    """(index, fixed) arrays of a list of entries without any check"""
    idx = np.array([int(v) if kind == "param" else -1 for kind, v in entries], dtype=np.int32)
    fix = np.array([0.0 if kind == "param" else float(v) for kind, v in entries])
    return idx, fix


def test_bad_specifications_are_refused_by_the_library_and_by_noise_layout(pkg):
    L, um = pkg.lib(), pkg.user_models
    ai, af, pi, pf = um.noise_layout(NC.NOISE, 2, 5)
    assert ai.tolist() == [2, 3] and pi.tolist() == [4, -1] and pf.tolist() == [0.0, 0.0]
    assert L.smc_user_noise_check(2, 5, _ip(ai), _fp(af), _ip(pi), _fp(pf)) == 0
    assert um.noise_layout(ADD_ONLY, 2, 5)[2:] == (None, None)
    assert L.smc_user_noise_check(2, 5, _ip(ai), _fp(af), None, None) == 0
    for add, prop, word in BAD_SPECS:
        a_i, a_f = _raw(add)
        p_i, p_f = _raw(prop) if prop else (None, None)
        assert L.smc_user_noise_check(2, 5, _ip(a_i), _fp(a_f), _ip(p_i), _fp(p_f)) != 0, (add, prop)
        assert word.encode() in L.smc_last_error(None), (add, prop, L.smc_last_error(None))
        with pytest.raises(ValueError):
            um.noise_layout({"additive": add, **({"proportional": prop} if prop else {})}, 2, 5)
    # the wrong number of entries: the C arrays carry no length, n_obs out of range and a half-given proportional part do
    for noise in ({"additive": [("param", 2)]}, {"additive": [("param", 2)] * 3},
                  {"additive": NC.NOISE["additive"], "proportional": [("fixed", 0.0)]}, {"proportional": NC.NOISE["proportional"]}):
        with pytest.raises(ValueError):
            um.noise_layout(noise, 2, 5)
    assert L.smc_user_noise_check(9, 5, _ip(ai), _fp(af), None, None) != 0 and b"n_obs" in L.smc_last_error(None)
    assert L.smc_user_noise_check(2, 5, _ip(ai), _fp(af), _ip(pi), None) != 0 and b"both" in L.smc_last_error(None)
    assert L.smc_user_noise_check(2, 5, None, None, None, None) != 0 and b"NULL" in L.smc_last_error(None)


def _random_case(seed, n=7):
    rs = np.random.RandomState(seed)
    t, obs = NC.make_data(seed)
    theta = np.column_stack([rs.uniform(0.1, 2, n), rs.uniform(0.05, 1, n), rs.uniform(0.005, 0.05, n), rs.uniform(0.005, 0.05, n),
                             rs.uniform(0.0, 0.3, n)])
    pred = np.stack([NC.closed_form(k1, k2, t) for k1, k2 in theta[:, :2]])
    return t, obs, theta, pred


def test_noise_loglik_agrees_with_a_plain_triple_loop(pkg):
    t, obs, theta, pred = _random_case(11)
    scale = np.array([1.0, 3.0])
    lk = pkg.user_models.noise_loglik(pred, t, obs, theta, NC.NOISE, obs_scale=scale)
    ref = np.zeros(theta.shape[0])
    n_seen = 0
    for p, th in enumerate(theta):
        a, b = (th[2], th[3]), (th[4], 0.0)
        for e in range(t.shape[0]):
            for i in range(t.shape[1]):
                if np.isnan(t[e, i]):
                    continue
                for k in range(2):
                    if np.isnan(obs[e, i, k]):
                        continue
                    n_seen += p == 0
                    sd = np.sqrt((a[k] * scale[k]) ** 2 + (b[k] * pred[p, e, i, k]) ** 2)
                    ref[p] += -0.5 * np.log(2 * np.pi) - np.log(sd) - (obs[e, i, k] - pred[p, e, i, k]) ** 2 / (2 * sd * sd)
    assert 150 < n_seen < 4 * 30 * 2 - 24           # NaN observations and the ragged row are in the data
    np.testing.assert_allclose(lk, ref, rtol=1e-12, atol=0)
    bad = theta.copy()
    bad[0, 2], bad[1, 3], bad[2, 4] = 0.0, -0.01, -1e-9
    assert np.isneginf(pkg.user_models.noise_loglik(pred, t, obs, bad, NC.NOISE)[:3]).all()
    assert np.isfinite(pkg.user_models.noise_loglik(pred, t, obs, bad, NC.NOISE)[3:]).all()
    empty = np.full_like(obs, np.nan)
    assert np.array_equal(pkg.user_models.noise_loglik(pred, t, empty, theta, NC.NOISE), np.zeros(theta.shape[0]))


def _single_sigma_loglik(pred, obs, t, scale, sigma):
    """include/smc_hip.h, smc_set_model_user3: sum_e [-m_e / 2 log(2 pi sigma^2) - sum log s_k - sum (r / s_k)^2 / (2 sigma^2)]"""
    seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
    r = np.where(seen, (obs[None] - np.where(seen[None], pred, 0.0)) / scale, 0.0)
    m = seen.sum(axis=(1, 2))
    ls = np.sum(np.where(seen, np.log(scale), 0.0), axis=(1, 2))
    s2 = sigma * sigma
    return np.sum(-0.5 * m[None] * np.log(2 * np.pi * s2)[:, None] - ls[None], axis=1) - np.sum(r * r, axis=(1, 2, 3)) / (2 * s2)


def test_one_shared_sigma_is_the_existing_formula(pkg):
    t, obs, theta, pred = _random_case(12)
    scale = np.array([1.0, 3.0])
    shared = {"additive": [("param", 2), ("param", 2)]}
    lk = pkg.user_models.noise_loglik(pred, t, obs, theta, shared, obs_scale=scale)
    np.testing.assert_allclose(lk, _single_sigma_loglik(pred, obs, t, scale, theta[:, 2]), rtol=1e-12, atol=0)
    fixed = {"additive": [("fixed", 0.02), ("fixed", 0.02)]}
    lk = pkg.user_models.noise_loglik(pred, t, obs, theta, fixed)
    np.testing.assert_allclose(lk, _single_sigma_loglik(pred, obs, t, np.ones(2), np.full(theta.shape[0], 0.02)), rtol=1e-12, atol=0)


def test_every_excess_term_is_non_negative_and_completes_the_density():
    """x = 1/2 log1p((b f / (a s))^2) + r^2 / (2 sd^2), as the kernels form it (w = 1 / (2 (a s)^2), q = (b / (a s))^2, u = q f^2,
    x = 1/2 log1p(u) + r^2 w / (1 + u)): >= 0, and floor + x is the negative log density without its constant."""
    rs = np.random.RandomState(5)
    n = 100000
    a, s = 10 ** rs.uniform(-6, 2, n), 10 ** rs.uniform(-3, 3, n)
    b = np.where(rs.uniform(size=n) < 0.2, 0.0, 10 ** rs.uniform(-6, 2, n))
    f, obs = rs.standard_normal(n) * 10 ** rs.uniform(-4, 4, n), rs.standard_normal(n) * 10 ** rs.uniform(-4, 4, n)
    w, q = 1.0 / (2.0 * (a * s) ** 2), b * b / (a * s) ** 2
    u, r = q * f * f, obs - f
    x = 0.5 * np.log1p(u) + r * r * w / (1.0 + u)
    assert np.all(x >= 0.0)
    assert np.all((r * r * w)[b == 0.0] == x[b == 0.0])          # without a proportional part the excess is r^2 w
    sd2 = (a * s) ** 2 + (b * f) ** 2
    ref = 0.5 * np.log(sd2) + r * r / (2 * sd2)
    np.testing.assert_allclose(np.log(a * s) + x, ref, rtol=1e-10, atol=1e-10)


def test_dump_source4_writes_the_eight_files_and_the_switches(pkg, tmp_path):
    src = pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode()
    for prop in (0, 1):
        d = tmp_path / f"p{prop}"
        d.mkdir()
        assert pkg.lib().smc_user_model_dump_source4(src, 2, 5, RK45, 2, prop, str(d).encode()) == 0
        assert sorted(os.listdir(d)) == ["philox.h", "reject_bound.h", "rk45_math.h", "smc_user_model.hip", "solve_sched.h", "sweep_args.h",
                                         "user_item_ops.h", "user_obs_args.h"]
        head = (d / "smc_user_model.hip").read_text()[:400]
        assert "#define SMC_USER_NOISE 1\n" in head and f"#define SMC_USER_NOISE_PROP {prop}\n" in head
    d = tmp_path / "three"
    d.mkdir()
    assert pkg.lib().smc_user_model_dump_source3(src, 2, 5, RK45, 2, str(d).encode()) == 0
    assert "#define SMC_USER_NOISE" not in (d / "smc_user_model.hip").read_text()[:400]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc from ROCm")
@pytest.mark.parametrize("prop", [0, 1], ids=["additive", "combined"])
def test_noise_rk45_sweep_kernel_keeps_four_waves_and_a_scratch_free_bulk_loop(pkg, tmp_path, prop):
    """As the smc_set_model_user3 kernel (tests/test_user_model_multiobs.py): <= 128 VGPRs, no scratch traffic in the bulk attempt
    loop, no scratch store in any attempt loop - the weights live in registers, log1p and the division in the rare output branch."""
    d = str(tmp_path)
    assert pkg.lib().smc_user_model_dump_source4(pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode(), 2, 5, RK45, 2, prop, d.encode()) == 0
    asm = os.path.join(d, "u.s")
    subprocess.run([HIPCC, *FLAGS, "-I", d, "-DSMC_ISA_MARKS", "-S", "--cuda-device-only", "-o", asm, os.path.join(d, "smc_user_model.hip")],
                   check=True, stderr=subprocess.DEVNULL, timeout=900)
    lines = open(asm).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("smc_user_solve_kernel:"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [l.strip() for l in lines[start:end]]
    nv = int(re.search(r"; NumVgprs: (\d+)", "\n".join(lines[end:end + 60])).group(1))
    assert nv <= 128, f"smc_user_solve_kernel: {nv} VGPRs, more than four waves per SIMD allow"
    seen = 0
    for mark in ("bulk_attempt", "lane_tail_attempt", "uniform_tail_attempt"):
        for i, l in enumerate(body):
            if "MARK " + mark in l:
                seen += 1
                lab, back = _innermost_loop(body, i)
                loop = body[lab:back + 1]
                assert not [x for x in loop if x.startswith("scratch_store")], mark
                if mark == "bulk_attempt":
                    assert not [x for x in loop if x.startswith("scratch_")], mark
    assert seen >= 3


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _bar(lk, ref):
    return np.max(np.abs(lk - ref) / np.maximum(1.0, np.abs(ref)))


def _population(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([NC.K_TRUE[0] * (1 + 0.1 * rs.standard_normal(n)), NC.K_TRUE[1] * (1 + 0.1 * rs.standard_normal(n)),
                            rs.uniform(0.005, 0.03, n), rs.uniform(0.01, 0.05, n), rs.uniform(0.02, 0.2, n)])


def _sweep(pkg, eng, th):
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    return eng.download_lk(pkg.SMC_SET_PRED), info


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_likelihood_is_noise_loglik_of_the_engines_own_predictions(pkg, method):
    t, obs = NC.make_data(0)
    n = 512
    th = _population(n, 1)
    th[0, 2], th[1, 3], th[2, 4], th[3, 2] = 0.0, -0.01, -1e-6, np.nan          # a <= 0, b < 0: -inf
    scale = (1.0, 3.0)
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], method=method, obs_scale=scale,
                           noise=NC.NOISE)
        lk, info = _sweep(pkg, eng, th)
        lk_p, pred, pinfo = eng.predict_user(th)
    assert info["n_failed"] == 0 and pinfo["n_failed"] == 0 and info["rk_attempts"] == pinfo["rk_attempts"]
    assert np.array_equal(lk, lk_p)
    assert np.isneginf(lk[:3]).all() and not np.isfinite(lk[3]) and np.isfinite(lk[4:]).all()
    ref = pkg.user_models.noise_loglik(pred, t, obs, th, NC.NOISE, obs_scale=scale)
    err = _bar(lk[4:], ref[4:])
    print(f"{method}: worst |lk - noise_loglik(pred)| / max(1, |lk|) = {err:.3g}")
    assert err <= 1e-9


@pytest.mark.gpu
def test_equivalences_with_the_single_sigma_path(pkg):
    t, obs = NC.make_data(0)
    n = 512
    src, um = pkg.user_models.CONSECUTIVE_REACTIONS_AB, pkg.user_models
    th = _population(n, 2)
    th[:, 4] = th[:, 2]                                          # sigma, the last parameter
    kw = dict(cond=NC.A0[:, None])
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        # (i) the degenerate specification takes the smc_set_model_user3 path: its bits
        eng.set_model_user(src, 2, t, obs, **kw)
        lk3, info3 = _sweep(pkg, eng, th)
        eng.set_model_user(src, 2, t, obs, noise={"additive": [("param", 4), ("param", 4)]}, **kw)
        lk_i, info_i = _sweep(pkg, eng, th)
        assert np.array_equal(lk3, lk_i) and info3 == info_i
        eng.set_model_user(src, 2, t, obs, est_sigma=False, sigma_fixed=0.02, **kw)
        lk3f, info3f = _sweep(pkg, eng, th)
        eng.set_model_user(src, 2, t, obs, noise={"additive": [("fixed", 0.02), ("fixed", 0.02)]}, **kw)
        lk_if, info_if = _sweep(pkg, eng, th)
        assert np.array_equal(lk3f, lk_if) and info3f == info_if
        # (ii) two sigma parameters that hold equal values (th[:, 2] == th[:, 4]): the noise kernels
        eng.set_model_user(src, 2, t, obs, noise={"additive": [("param", 2), ("param", 4)]}, **kw)
        lk_ii, info_ii = _sweep(pkg, eng, th)
        assert info_ii["n_failed"] == 0 and info_ii["rk_attempts"] == info3["rk_attempts"]
        print(f"(ii) {_bar(lk_ii, lk3):.3g}")
        assert _bar(lk_ii, lk3) <= 1e-9
        # (iii) one sigma with obs_scale (1, 3) is additive parameters (sigma, 3 sigma) without obs_scale
        th3 = th.copy()
        th3[:, 3] = 3.0 * th3[:, 4]
        eng.set_model_user(src, 2, t, obs, obs_scale=(1.0, 3.0), **kw)
        lk_s, _ = _sweep(pkg, eng, th3)
        eng.set_model_user(src, 2, t, obs, noise={"additive": [("param", 4), ("param", 3)]}, **kw)
        lk_iii, _ = _sweep(pkg, eng, th3)
        print(f"(iii) {_bar(lk_iii, lk_s):.3g}")
        assert _bar(lk_iii, lk_s) <= 1e-9
        # (iv) the proportional variant with every b = 0 is the additive-only variant
        th4 = _population(n, 3)
        th4[:, 4] = 0.0
        eng.set_model_user(src, 2, t, obs, obs_scale=(1.0, 3.0), noise=ADD_ONLY, **kw)
        lk_a, info_a = _sweep(pkg, eng, th4)
        eng.set_model_user(src, 2, t, obs, obs_scale=(1.0, 3.0), noise=NC.NOISE, **kw)
        lk_iv, info_iv = _sweep(pkg, eng, th4)
        assert info_a["rk_attempts"] == info_iv["rk_attempts"]
        print(f"(iv) {_bar(lk_iv, lk_a):.3g}")
        assert _bar(lk_iv, lk_a) <= 1e-9
        _, pred, _ = eng.predict_user(th4)
    assert _bar(lk_a, um.noise_loglik(pred, t, obs, th4, ADD_ONLY, obs_scale=(1.0, 3.0))) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [ADD_ONLY, NC.NOISE], ids=["additive", "combined"])
def test_early_rejection_is_exact_and_saves_attempts(pkg, noise):
    t, obs = NC.make_data(3)
    n = 4096
    th = _population(n, 7)
    out = []
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], noise=noise)
        lk, info = _sweep(pkg, eng, th)
        assert info["n_failed"] == 0
        for on in (False, True):
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_lk(pkg.SMC_SET_FILT, lk)
            eng.set_early_reject(on)
            mh = eng.mh_step_device_rng(0.5, 1.0, np.diag([0.004, 0.004, 2e-5, 2e-5, 1e-3]), 7, 3)
            out.append((mh, eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags()))
    (m0, p0, l0, a0), (m1, p1, l1, a1) = out
    print(f"accepted {m0['accepted_now']} of {n}; attempts {m0['rk_attempts']} without, {m1['rk_attempts']} with early rejection")
    assert m0["n_failed"] == 0 and 0 < m0["accepted_now"] < n
    assert m0["accepted_now"] == m1["accepted_now"] and np.array_equal(a0, a1) and np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert m1["rk_attempts"] < m0["rk_attempts"]


@pytest.mark.gpu
def test_predictive_noise_has_the_particles_own_sd(pkg):
    t, obs = NC.make_data(0)
    n = 16384
    th = np.tile(NC.THETA_TRUE * np.array([1.0, 1.0, 1.5, 0.7, 1.2]), (n, 1))
    scale = np.array([1.0, 3.0])
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], obs_scale=scale, noise=NC.NOISE)
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        _, pred, _ = eng.predict_user(th[:1])
        clean = eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.5,))
        noisy = eng.predictive_summary(pkg.SMC_SET_PRED, probs=(0.5,), noise=True, seed=11)
    f = pred[0]
    ok = ~np.isnan(f)
    assert ok.sum() == (3 * 30 + 18) * 2 and np.array_equal(np.isnan(clean["mean"]), ~ok)
    # without noise nothing is drawn: every order statistic IS the prediction, and sd is zero up to the rounding of the mean of n
    # equal numbers (the bound of tests/test_user_predictive.py; a sum of 16384 copies of f is not exact, so neither is "== 0")
    assert np.array_equal(clean["lower"][0][ok], f[ok]) and np.array_equal(clean["upper"][0][ok], f[ok])
    assert np.all(clean["sd"][ok] <= 4 * n * np.finfo(float).eps * np.abs(f[ok]).max())
    sd = np.sqrt((th[0, 2:4] * scale) ** 2 + (np.array([th[0, 4], 0.0]) * f) ** 2)
    z_mean = np.abs(noisy["mean"] - f)[ok] / (sd[ok] / np.sqrt(n))
    z_sd = np.abs(noisy["sd"] / sd - 1.0)[ok] * np.sqrt(2 * n)
    print(f"worst mean {z_mean.max():.2f} and sd {z_sd.max():.2f} standard errors over {ok.sum()} cells")
    assert z_mean.max() <= 5.0 and z_sd.max() <= 5.0


@pytest.mark.gpu
def test_full_run_follows_the_chain_on_the_closed_form(pkg):
    t, obs = NC.make_data(0)
    n = 8192
    s = pkg.SMCSettings(n_particle=n, priors=PRIORS)
    with pkg.HipEngine(n, 5, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=NC.A0[:, None], rtol=1e-6, atol=1e-9, noise=NC.NOISE)
        out = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3, predictive={"probs": (0.05, 0.95), "noise": True})
    assert out["gamma"] == 1.0
    m, sd = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
    print("mean", m, "sd", sd, "\n(mean - chain) / sd_chain", (m - CHAIN_MEAN) / CHAIN_SD, "sd / sd_chain", sd / CHAIN_SD)
    assert np.all(np.abs(m - CHAIN_MEAN) <= 0.5 * CHAIN_SD)
    assert np.all((sd / CHAIN_SD >= 0.75) & (sd / CHAIN_SD <= 1.33))
    # the predictive band of replicated observations under the noise model: 90 % of it should hold about 90 % of the data
    band = out["predictive"]
    seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
    inside = (obs >= band["lower"][0]) & (obs <= band["upper"][1])
    assert 0.8 <= inside[seen].mean() <= 0.98


@pytest.mark.gpu
def test_an_image_the_lds_table_cannot_hold_is_refused_with_the_bytes(pkg):
    """8 experiments x 518 times x 2 outputs: smc_set_model_user3's image fits the table by 64 B, the noise block (40 + 8 n_ex words)
    does not."""
    n_ex, n_t = 8, 518
    t = np.tile(np.linspace(0.0, 10.0, n_t), (n_ex, 1))
    obs = np.zeros((n_ex, n_t, 2))
    cond = np.ones((n_ex, 1))
    src = pkg.user_models.CONSECUTIVE_REACTIONS_AB
    with pkg.HipEngine(64, 5, device=0) as eng:
        eng.set_model_user(src, 2, t, obs, cond=cond)
        with pytest.raises(pkg.SmcError, match=r"154368 B needed, 153600 B available"):
            eng.set_model_user(src, 2, t, obs, cond=cond, noise=ADD_ONLY)
        with pytest.raises(ValueError):
            eng.set_model_user(src, 2, t, obs, cond=cond, noise={"additive": [("param", 5), ("param", 3)]})
        ai, af = np.array([5, 3], dtype=np.int32), np.zeros(2)
        st = eng.L.smc_set_model_user4(eng.ctx, src.encode(), 2, 2, _fp(t), _fp(obs), _fp(cond), None, n_ex, n_t, 1, _ip(ai), _fp(af),
                                       None, None, 1e-3, 1e-6, 0)
        assert st != 0 and b"add_index" in eng.L.smc_last_error(eng.ctx)
