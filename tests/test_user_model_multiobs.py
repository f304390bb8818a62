"""User models with several observed outputs, missing data (NaN), ragged experiments and predictions (include/smc_hip.h:
smc_set_model_user3, smc_user_predict).  CPU part: the multi-output sources compile for gfx950 under RK45 and BDF, the ABI
refuses what it must, the NumPy data rules, and the RK45 sweep kernel's registers.  GPU part: bit-identity with the
one-output path, SciPy comparisons output by output, predictions, early rejection and a full run."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import robertson_bdf_bound as RB
from test_k8_uniform_control import _innermost_loop
from test_user_model import DIVERGING

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-fast-math"]   # csrc/Makefile
RK45, BDF = 0, 1
PRIORS = {"k1": {"dist": "uniform", "low": 0, "high": 3}, "k2": {"dist": "uniform", "low": 0, "high": 3},
          "sigma": {"dist": "uniform", "low": 0, "high": 1}}


def _check3(pkg, src, ns, method, n_obs, dim=3):
    log = ctypes.create_string_buffer(16384)
    rc = pkg.lib().smc_user_model_check3(src.encode(), ns, dim, method, n_obs, log, 16384)
    return rc, log.value.decode(errors="replace")


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_two_output_sources_compile_under_rk45_and_bdf(pkg):
    um = pkg.user_models
    for src, ns, method in ((um.CONSECUTIVE_REACTIONS_AB, 2, RK45), (um.CONSECUTIVE_REACTIONS_AB, 2, BDF), (um.ROBERTSON_AC, 3, BDF)):
        rc, log = _check3(pkg, src, ns, method, 2)
        assert rc == 0, log
    rc, log = _check3(pkg, um.MICHAELIS_MENTEN, 1, RK45, 1)       # one output through smc_user_obs
    assert rc == 0, log


def test_named_but_undefined_obs_vec_and_bad_n_obs(pkg):
    um = pkg.user_models
    for method in (RK45, BDF):
        rc, log = _check3(pkg, um.CONSECUTIVE_REACTIONS + "// smc_user_obs_vec: later\n", 2, method, 1)
        assert rc == 1 and "smc_user_obs_vec" in log
        rc, log = _check3(pkg, um.CONSECUTIVE_REACTIONS, 2, method, 2)      # two outputs need smc_user_obs_vec
        assert rc == 1 and "smc_user_obs_vec" in log
        for n_obs in (0, 9):
            assert _check3(pkg, um.CONSECUTIVE_REACTIONS_AB, 2, method, n_obs)[0] == 2
            assert pkg.lib().smc_user_model_dump_source3(um.CONSECUTIVE_REACTIONS_AB.encode(), 2, 3, method, n_obs, b"/nonexistent") == 2


def test_obs_layout_helper(pkg):
    um = pkg.user_models
    t = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 0.5, np.nan, np.nan], [1.0, 2.0, 4.0, np.nan]])
    obs = np.ones((3, 4, 2))
    obs[0, 1, 0] = np.nan
    obs[1, 2:, :] = np.inf                     # at NaN times: ignored whatever it holds
    obs[2, :, 1] = np.nan
    out = um.obs_layout(t, obs, (1.0, 3.0))
    assert out["n_t_e"].tolist() == [4, 2, 3]
    assert out["m_e"].tolist() == [7, 4, 3]
    np.testing.assert_allclose(out["sum_log_scale"], [4 * np.log(3.0), 2 * np.log(3.0), 0.0], rtol=0, atol=1e-15)
    assert um.obs_layout(t, obs)["sum_log_scale"].tolist() == [0.0, 0.0, 0.0]
    bad_t = t.copy()
    bad_t[0, 1] = np.nan                       # NaN followed by a number
    with pytest.raises(ValueError, match="trailing"):
        um.obs_layout(bad_t, obs)
    bad_t = t.copy()
    bad_t[0, 2] = 1.0                          # not strictly increasing
    with pytest.raises(ValueError, match="increasing"):
        um.obs_layout(bad_t, obs)
    with pytest.raises(ValueError, match="no finite time"):
        um.obs_layout(np.full((1, 3), np.nan), np.ones((1, 3, 1)))
    for s in ((1.0, 0.0), (1.0, -2.0), (np.nan, 1.0)):
        with pytest.raises(ValueError, match="obs_scale"):
            um.obs_layout(t, obs, s)
    with pytest.raises(ValueError):
        um.obs_layout(t, np.ones((3, 4)))      # obs must be 3-D
    with pytest.raises(ValueError):
        um.obs_layout(t, np.ones((3, 4, 9)))   # more than SMC_USER_MAX_OBS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc from ROCm")
def test_two_output_rk45_kernel_registers_and_scratch(pkg, tmp_path):
    """CONSECUTIVE_REACTIONS_AB, n_obs = 2, dumped and compiled off line: the sweep kernel still fits four waves per SIMD
    (<= 128 VGPRs) and has no scratch traffic in its bulk attempt loop and no scratch store in any attempt loop."""
    d = str(tmp_path)
    assert pkg.lib().smc_user_model_dump_source3(pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode(), 2, 3, RK45, 2, d.encode()) == 0
    assert sorted(os.listdir(d)) == ["philox.h", "reject_bound.h", "rk45_math.h", "smc_user_model.hip", "solve_sched.h", "sweep_args.h",
                                     "user_item_ops.h", "user_obs_args.h"]
    asm = os.path.join(d, "u.s")
    subprocess.run([HIPCC, *FLAGS, "-I", d, "-DSMC_ISA_MARKS", "-S", "--cuda-device-only", "-o", asm, os.path.join(d, "smc_user_model.hip")],
                   check=True, stderr=subprocess.DEVNULL, timeout=900)
    text = open(asm).read()
    assert "smc_user_predict_kernel:" in text
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("smc_user_solve_kernel:"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [l.strip() for l in lines[start:end]]
    nv = int(re.search(r"; NumVgprs: (\d+)", "\n".join(lines[end:end + 60])).group(1))
    assert nv <= 128, f"smc_user_solve_kernel: {nv} VGPRs, more than four waves per SIMD allow"
    for mark in ("bulk_attempt", "lane_tail_attempt", "uniform_tail_attempt"):
        for i, l in enumerate(body):
            if "MARK " + mark in l:
                lab, back = _innermost_loop(body, i)
                loop = body[lab:back + 1]
                assert not [x for x in loop if x.startswith("scratch_store")], mark
                if mark == "bulk_attempt":
                    assert not [x for x in loop if x.startswith("scratch_")], mark


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _run(pkg, eng, th):
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    return eng.download_lk(pkg.SMC_SET_PRED), info


def _mm_population(n, seed):
    rs = np.random.RandomState(seed)
    th = np.array([1.2254, 0.5218, 0.02048]) + rs.standard_normal((n, 3)) * np.array([0.05, 0.05, 0.002])
    th[: n // 4] = rs.uniform(0.05, 5, size=(n // 4, 3))
    return th


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_one_output_through_the_new_path_is_bit_identical(pkg, data, method):
    """The MM user model: (a) 2-D obs and obs[..., None] give the same bits and attempts; (b) an all-NaN last experiment
    is the same as leaving it out; (c) a ragged row equals an engine whose t ends at that row's last time."""
    n = 2048
    th = _mm_population(n, 4)
    src = pkg.user_models.MICHAELIS_MENTEN
    t, P, S0 = np.asarray(data.t), np.asarray(data.P_obs), np.asarray(data.S0)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_model_user(src, 1, t, P, cond=S0[:, None], method=method)
        lk_a, info_a = _run(pkg, eng, th)
        eng.set_model_user(src, 1, t, P[..., None], cond=S0[:, None], method=method)
        lk_b, info_b = _run(pkg, eng, th)
        assert np.array_equal(lk_a, lk_b) and info_a == info_b
        # (b) one more experiment, never measured
        t2 = np.vstack([t, t[:1]])
        P2 = np.concatenate([P[..., None], np.full((1, t.shape[1], 1), np.nan)])
        eng.set_model_user(src, 1, t2, P2, cond=np.append(S0, S0[0])[:, None], method=method)
        lk_c, _ = _run(pkg, eng, th)
        assert np.array_equal(lk_a, lk_c)
        # (c) experiment 0 alone, its row cut after 5 times: as NaN times and as a shorter t
        L = 5
        tr = t[:1].copy()
        tr[0, L:] = np.nan
        eng.set_model_user(src, 1, tr, P[:1, :, None], cond=S0[:1, None], method=method)
        lk_d, info_d = _run(pkg, eng, th)
        eng.set_model_user(src, 1, t[:1, :L], P[:1, :L], cond=S0[:1, None], method=method)
        lk_e, info_e = _run(pkg, eng, th)
        assert np.array_equal(lk_d, lk_e) and info_d == info_e


@pytest.mark.gpu
def test_two_identical_outputs_double_the_loglik(pkg):
    src = pkg.user_models.CONSECUTIVE_REACTIONS_AB.replace("out[0] = y[0];", "out[0] = y[1];")
    rs = np.random.RandomState(5)
    t = np.tile(np.linspace(0.0, 10.0, 20), (3, 1))
    obs = rs.uniform(0, 1, t.shape)
    th = np.column_stack([rs.uniform(0.1, 2, 512), rs.uniform(0.05, 1, 512), rs.uniform(0.01, 0.5, 512)])
    with pkg.HipEngine(512, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS, 2, t, obs, cond=[[1.0], [2.0], [0.5]])
        lk1, _ = _run(pkg, eng, th)
        eng.set_model_user(src, 2, t, np.stack([obs, obs], axis=2), cond=[[1.0], [2.0], [0.5]])
        lk2, _ = _run(pkg, eng, th)
    assert np.max(np.abs(lk2 - 2 * lk1) / np.abs(2 * lk1)) <= 1e-12


def _ab_data(seed=0):
    """Four experiments of A -> B -> C with A and B measured, scattered NaNs and experiment 2 cut after 18 of 30 times."""
    rs = np.random.RandomState(seed)
    n_ex, n_t = 4, 30
    t = np.tile(np.linspace(0.0, 10.0, n_t), (n_ex, 1))
    t[2, 18:] = np.nan
    A0 = np.array([1.0, 2.0, 0.5, 1.5])
    k_true, sig_true, scale = (0.8, 0.3), 0.01, np.array([1.0, 3.0])
    tt = np.nan_to_num(t)
    a = A0[:, None] * np.exp(-k_true[0] * tt)
    b = A0[:, None] * k_true[0] / (k_true[1] - k_true[0]) * (np.exp(-k_true[0] * tt) - np.exp(-k_true[1] * tt))
    obs = np.stack([a, b], axis=2) + sig_true * scale * rs.standard_normal((n_ex, n_t, 2))
    obs[rs.uniform(size=obs.shape) < 0.15] = np.nan
    obs[1, 5, :] = np.nan
    return t, obs, A0, k_true, sig_true, scale


def _np_loglik(pred, obs, t, scale, sigma):
    """The likelihood of include/smc_hip.h (smc_set_model_user3) from model outputs pred (n, n_ex, n_t, n_obs)."""
    seen = ~np.isnan(obs) & ~np.isnan(t)[:, :, None]
    r = np.where(seen, (obs[None] - pred) / scale, 0.0)
    m = seen.sum(axis=(1, 2))
    ls = np.sum(np.where(seen, np.log(scale), 0.0), axis=(1, 2))
    s2 = sigma * sigma
    return np.sum(-0.5 * m[None] * np.log(2 * np.pi * s2)[:, None] - ls[None], axis=1) - np.sum(r * r, axis=(1, 2, 3)) / (2 * s2)


@pytest.mark.gpu
def test_consecutive_ab_follows_scipy_output_by_output(pkg):
    from scipy.integrate import solve_ivp
    t, obs, A0, _, _, scale = _ab_data()
    n_ex, n_t = t.shape
    rs = np.random.RandomState(1)
    n = 128
    th = np.column_stack([rs.uniform(0.1, 2, n), rs.uniform(0.05, 1, n), rs.uniform(0.005, 0.05, n)])
    ref = np.full((n, n_ex, n_t, 2), np.nan)
    for p, (k1, k2, _) in enumerate(th):
        for e in range(n_ex):
            te = t[e][~np.isnan(t[e])]
            sol = solve_ivp(lambda _t, y: [-k1 * y[0], k1 * y[0] - k2 * y[1]], [te[0], te[-1]], [A0[e], 0.0], method="RK45",
                            t_eval=te, rtol=1e-3, atol=1e-6)
            ref[p, e, :te.size] = sol.y.T
    lk_ref = _np_loglik(ref, obs, t, scale, th[:, 2])
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=scale)
        lk, info = _run(pkg, eng, th)
        lk_p, pred, pinfo = eng.predict_user(th)
        lk_again = eng.download_lk(pkg.SMC_SET_PRED)
    assert info["n_failed"] == 0 and pinfo["n_failed"] == 0 and pinfo["rk_attempts"] == info["rk_attempts"]
    assert np.array_equal(lk_p, lk) and np.array_equal(lk_again, lk)        # the resident set is untouched
    assert pred.shape == (n, n_ex, n_t, 2)
    assert np.array_equal(np.isnan(pred), np.isnan(ref))                     # NaN exactly past the ragged row's end
    assert np.nanmax(np.abs(pred - ref)) < 1e-9
    assert np.max(np.abs(lk - lk_ref) / np.maximum(1.0, np.abs(lk_ref))) < 1e-6


@pytest.mark.gpu
def test_robertson_ac_follows_scipy_bdf(pkg):
    from scipy.integrate import solve_ivp
    th0, _ = RB.population(n=48, seed=13)
    rs = np.random.RandomState(2)
    t = RB.T.copy()
    t[3, 12:] = np.nan
    n_ex, n_t = t.shape
    scale = np.array([1.0, 0.02])

    def solve(k1, k3, a0, te):
        s = solve_ivp(lambda _t, y: RB.rhs(_t, y, k1, k3), [te[0], te[-1]], [a0, 0.0, 0.0], method="BDF", t_eval=te,
                      rtol=RB.RTOL, atol=RB.ATOL, jac=lambda _t, y: RB.jac(_t, y, k1, k3))
        return s.y[[0, 2]].T
    clean = np.full((n_ex, n_t, 2), np.nan)
    for e in range(n_ex):
        te = t[e][~np.isnan(t[e])]
        clean[e, :te.size] = solve(RB.K_TRUE[0], RB.K_TRUE[1], RB.A0[e], te)
    obs = clean + RB.SIGMA_TRUE * scale * rs.standard_normal(clean.shape)
    obs[rs.uniform(size=obs.shape) < 0.1] = np.nan
    n = th0.shape[0]
    ref = np.full((n, n_ex, n_t, 2), np.nan)
    for p, (k1, k3, _) in enumerate(th0):
        for e in range(n_ex):
            te = t[e][~np.isnan(t[e])]
            ref[p, e, :te.size] = solve(k1, k3, RB.A0[e], te)
    lk_ref = _np_loglik(ref, obs, t, scale, th0[:, 2])
    seen = ~np.isnan(obs)[None] & ~np.isnan(ref)
    r = np.where(seen, obs[None] - ref, 0.0)
    delta = np.where(seen, RB.K_BOUND * (RB.ATOL + RB.RTOL * np.abs(np.nan_to_num(ref))), 0.0)
    bound = np.sum((2 * np.abs(r) * delta + delta * delta) / scale ** 2, axis=(1, 2, 3)) / (2 * th0[:, 2] ** 2)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior({"k1": {"dist": "uniform", "low": 0, "high": 0.2}, "k3": {"dist": "uniform", "low": 0, "high": 5e4},
                       "sigma": {"dist": "uniform", "low": 0, "high": 0.1}})
        eng.set_model_user(pkg.user_models.ROBERTSON_AC, 3, t, obs, cond=RB.A0[:, None], rtol=RB.RTOL, atol=RB.ATOL,
                           method="BDF", obs_scale=scale)
        lk, info = _run(pkg, eng, th0)
        lk_p, pred, pinfo = eng.predict_user(th0)
    assert info["n_failed"] == 0 and np.array_equal(lk, lk_p)
    assert np.array_equal(np.isnan(pred), np.isnan(ref))
    dp = RB.K_BOUND * (RB.ATOL + RB.RTOL * np.abs(np.nan_to_num(ref)))
    assert np.all(np.abs(np.nan_to_num(pred - ref)) <= dp)
    err = np.abs(lk - lk_ref)
    assert np.all(err <= bound + 1e-9 * np.abs(lk_ref)), f"worst ratio {np.max(err / bound):.3g}"


@pytest.mark.gpu
def test_predict_user_matches_the_builtin_predictions_and_failure_rows(pkg, data):
    n = 1024
    th = _mm_population(n, 6)
    t, P, S0 = np.asarray(data.t), np.asarray(data.P_obs), np.asarray(data.S0)
    with pkg.HipEngine(n // 2, 3, device=0) as eng:          # n > n_local: two chunks
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_model_mm(t, P, S0)
        lk_a, pred_a, info_a = eng.loglik_host(th, want_pred=True)
        eng.set_model_user(pkg.user_models.MICHAELIS_MENTEN, 1, t, P, cond=S0[:, None])     # the one-output path
        lk_b, pred_b, info_b = eng.predict_user(th)
    assert info_a["n_failed"] == 0 and info_b["n_failed"] == 0 and info_a["rk_attempts"] == info_b["rk_attempts"]
    assert pred_b.shape == pred_a.shape + (1,)
    assert np.max(np.abs(pred_b[..., 0] - pred_a)) < 1e-12
    assert np.max(np.abs(lk_a - lk_b) / np.maximum(1.0, np.abs(lk_a))) < 1e-10
    m = 64
    tt = np.linspace(0.0, 2.0, 10)[None, :]
    thd = np.column_stack([np.full(m, 0.5), np.full(m, 1.0), np.full(m, 0.1)])
    for method in ("RK45", "BDF"):
        with pkg.HipEngine(m, 3, device=0) as eng:
            eng.set_prior(pkg.SMCSettings().priors)
            eng.set_model_user(DIVERGING, 1, tt, np.zeros_like(tt)[..., None], method=method)
            _, pred, info = eng.predict_user(thd)
        assert info["n_failed"] == m
        bad = np.isnan(pred[:, 0, :, 0])
        first = bad.argmax(axis=1)
        assert np.all(bad.any(axis=1)) and np.all(first >= 1)
        assert all(bad[p, first[p]:].all() and not bad[p, :first[p]].any() for p in range(m)), method


@pytest.mark.gpu
def test_masked_ragged_two_output_metropolis_sweep_with_early_rejection(pkg):
    t, obs, A0, k_true, sig_true, scale = _ab_data(seed=3)
    n = 4096
    rs = np.random.RandomState(7)
    th = np.column_stack([k_true[0] * (1 + 0.1 * rs.standard_normal(n)), k_true[1] * (1 + 0.1 * rs.standard_normal(n)),
                          rs.uniform(0.005, 0.03, n)])
    out = []
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=scale)
        lk, info = _run(pkg, eng, th)
        assert info["n_failed"] == 0
        for on in (False, True):
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_lk(pkg.SMC_SET_FILT, lk)
            eng.set_early_reject(on)
            mh = eng.mh_step_device_rng(0.5, 1.0, np.diag([0.004, 0.004, 0.002]), 7, 3)
            out.append((mh, eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags()))
    (m0, p0, l0, a0), (m1, p1, l1, a1) = out
    assert m0["n_failed"] == 0 and 0 < m0["accepted_now"] < n
    assert m0["accepted_now"] == m1["accepted_now"] and np.array_equal(a0, a1) and np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert m1["rk_attempts"] <= m0["rk_attempts"]


@pytest.mark.gpu
def test_two_output_full_run_recovers_the_constants_and_predicts_c(pkg):
    t, obs, A0, k_true, sig_true, scale = _ab_data(seed=0)
    n = 8192
    s = pkg.SMCSettings(n_particle=n, priors=PRIORS)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=scale)
        out = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3)
        assert out["gamma"] == 1.0
        m, sd = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
        assert np.all(np.abs(m[:2] - np.array(k_true)) < 5 * sd[:2] + 0.02) and abs(m[2] - sig_true) < 0.004, (m, sd)
        # the unmeasured product C as a third output (an all-NaN column adds nothing to the likelihood)
        obs3 = np.concatenate([obs, np.full(obs.shape[:2] + (1,), np.nan)], axis=2)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_ABC, 2, t, obs3, cond=A0[:, None], obs_scale=(1.0, 3.0, 1.0))
        post = out["p_pred"][:256]
        _, pred, info = eng.predict_user(post)
    assert info["n_failed"] == 0 and pred.shape == (256, 4, 30, 3)
    tt = t[None]
    c_true = A0[None, :, None] * (1 - (k_true[1] * np.exp(-k_true[0] * tt) - k_true[0] * np.exp(-k_true[1] * tt)) / (k_true[1] - k_true[0]))
    c_mean = np.mean(pred[..., 2], axis=0)
    ok = ~np.isnan(t)
    assert np.all(np.isnan(c_mean[~ok]))
    assert np.max(np.abs(c_mean[ok] - c_true[0][ok])) < 0.02


@pytest.mark.gpu
def test_shape_and_data_errors_are_refused(pkg):
    t = np.linspace(0.0, 1.0, 5)[None, :]
    with pkg.HipEngine(64, 3, device=0) as eng:
        with pytest.raises(ValueError):
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, np.zeros((1, 4, 2)), cond=[[1.0]])
        with pytest.raises(ValueError, match="obs_scale"):
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, np.zeros((1, 5, 2)), cond=[[1.0]], obs_scale=(1.0, 0.0))
        bad = t.copy()
        bad[0, 2] = np.nan
        with pytest.raises(ValueError, match="trailing"):
            eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, bad, np.zeros((1, 5, 2)), cond=[[1.0]])
        # the library refuses the same data on its own
        obs = np.zeros((1, 5, 2))
        st = eng.L.smc_set_model_user3(eng.ctx, pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode(), 2, 2,
                                       bad.ctypes.data_as(pkg.binding.c_dp), obs.ctypes.data_as(pkg.binding.c_dp),
                                       np.ones(1).ctypes.data_as(pkg.binding.c_dp), None, 1, 5, 1, 1, 5.0, 1e-3, 1e-6, 0)
        assert st != 0 and b"trailing" in eng.L.smc_last_error(eng.ctx)
        assert eng.L.smc_set_model_user3(eng.ctx, pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode(), 2, 9,
                                         t.ctypes.data_as(pkg.binding.c_dp), obs.ctypes.data_as(pkg.binding.c_dp),
                                         np.ones(1).ctypes.data_as(pkg.binding.c_dp), None, 1, 5, 1, 1, 5.0, 1e-3, 1e-6, 0) != 0
