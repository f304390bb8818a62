"""Posterior predictive bands of user models (include/smc_hip.h: smc_user_predict_at, smc_user_predict_summary).  CPU part: the
ABI, the rank rule of the quantiles against NumPy, the design rules, and the selection core (csrc/predictive_select.h) compiled
for the host against np.sort.  GPU part: predictions on a design other than the data's against SciPy, the summaries against
NumPy on the downloaded particles (order statistics bit for bit), failed solves, staging groups, untouched state, the noise
term's moments, and a full run with run_smc(predictive=...)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import robertson_bdf_bound as RB
from test_user_model import DIVERGING
from test_user_model_multiobs import PRIORS, _ab_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "tests", "hostcheck", "predictive_select_hostcheck.cpp")
EPS = 2.0 ** -52
SIZES = (1, 2, 3, 5, 64, 4095, 4096, 5000, 65536)
PROBS = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
ROB_PRIORS = {"k1": {"dist": "uniform", "low": 0, "high": 1}, "k3": {"dist": "uniform", "low": 0, "high": 2e5},
              "sigma": {"dist": "uniform", "low": 0, "high": 0.1}}
# DIVERGING fails for every particle; here only for those with theta[1] > 0.5, so that a set can hold both kinds
DIVERGING_SOME = DIVERGING.replace("(t > 1.0)", "(t > 1.0 && theta[1] > 0.5)")
assert DIVERGING_SOME != DIVERGING


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_abi_declares_binds_and_exports_both_functions(pkg):
    names = {"smc_user_predict_at", "smc_user_predict_summary"}
    assert names <= set(pkg.header_symbols())
    assert names <= set(pkg.binding.SIGNATURES)
    L = pkg.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert names <= exported
    assert L.smc_abi_version() == 3
    assert len(pkg.binding.SIGNATURES["smc_user_predict_at"][1]) == 10
    assert len(pkg.binding.SIGNATURES["smc_user_predict_summary"][1]) == 20


def test_quantile_ranks_pick_numpys_elements(pkg):
    rs = np.random.RandomState(0)
    q = np.array(PROBS)
    for m in SIZES:
        x = np.sort(rs.standard_normal(m) * 10.0 ** rs.uniform(-3, 3))
        lo, hi, frac = pkg.user_models.quantile_ranks(m, q)
        assert lo.dtype == np.int64 and np.all((0 <= lo) & (lo <= hi) & (hi <= m - 1) & (hi - lo <= 1))
        assert np.array_equal(x[lo], np.quantile(x, q, method="lower")), m
        assert np.array_equal(x[hi], np.quantile(x, q, method="higher")), m
        lin = x[lo] + (x[hi] - x[lo]) * frac
        ref = np.quantile(x, q, method="linear")
        assert np.all(np.abs(lin - ref) <= 4 * EPS * np.abs(ref)), (m, np.max(np.abs(lin - ref) / np.abs(ref)))
    lo, hi, frac = pkg.user_models.quantile_ranks(np.array([[1], [5]]), q[None, :])       # one count per cell broadcasts
    assert lo.shape == (2, q.size) and np.all(lo[0] == 0) and hi[1, -1] == 4
    with pytest.raises(ValueError):
        pkg.user_models.quantile_ranks(0, q)
    with pytest.raises(ValueError):
        pkg.user_models.quantile_ranks(5, [1.5])


def test_design_layout_rules_and_wording(pkg):
    um = pkg.user_models
    t = np.array([[0.0, 1.0, 2.0, 3.0], [0.0, 0.5, np.nan, np.nan], [1.0, 2.0, 4.0, np.nan]])
    cond = np.array([[1.0], [2.0], [0.7]])
    assert um.design_layout(t, cond, 1).tolist() == [4, 2, 3]
    assert um.design_layout(t, None, 0).tolist() == [4, 2, 3]
    obs = np.ones(t.shape + (1,))

    def both(bad_t, match):
        with pytest.raises(ValueError, match=match) as d:
            um.design_layout(bad_t, cond[: len(bad_t)], 1)
        with pytest.raises(ValueError, match=match) as o:
            um.obs_layout(bad_t, obs[: len(bad_t)])
        # the same rule in the same words
        assert str(d.value).replace("design_layout: ", "") == str(o.value).replace("obs_layout: ", "")
    bad = t.copy()
    bad[0, 1] = np.nan
    both(bad, "trailing")
    both(np.full((1, 4), np.nan), "no finite time")
    bad = t.copy()
    bad[0, 2] = 1.0
    both(bad, "increasing")
    bad = t.copy()
    bad[0, 3] = np.inf
    both(bad, "infinite")
    for c, k in ((cond[:2], 1), (cond, 2), (None, 1), (np.ones((3, 1, 1)), 1)):
        with pytest.raises(ValueError, match="cond_new"):
            um.design_layout(t, c, k)
    with pytest.raises(ValueError):
        um.design_layout(t[0], cond, 1)


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("ps")
    so = str(d / "libps.so")
    base = ["g++", "-O1", "-g", "-shared", "-fPIC", "-o", so, HOSTCHECK]
    san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base, check=True)
    L = ctypes.CDLL(so)
    L.ps_key.restype, L.ps_key.argtypes = ctypes.c_uint64, [ctypes.c_double]
    L.ps_value.restype, L.ps_value.argtypes = ctypes.c_double, [ctypes.c_uint64]
    dp, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)
    L.ps_select.restype, L.ps_select.argtypes = ctypes.c_longlong, [dp, ctypes.c_longlong, lp, ctypes.c_int, dp]
    L.ps_ranks.restype, L.ps_ranks.argtypes = None, [ctypes.c_longlong, ctypes.c_double, lp, lp, dp]
    return L


def _special_doubles(rs, n):
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308, 1e-310, -1e-310,
                     np.inf, -np.inf, np.nan, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0, 1.0 + EPS])
    body = rs.standard_normal(n) * 10.0 ** rs.uniform(-300, 300, n)
    return np.concatenate([tiny, body, body[:7]])         # with ties


def test_selection_core_on_the_host_against_np_sort(ps):
    rs = np.random.RandomState(5)
    x = _special_doubles(rs, 3000)
    finite = x[np.isfinite(x)]
    keys = np.array([ps.ps_key(float(v)) for v in x], dtype=np.uint64)
    assert np.all(keys[~np.isfinite(x)] == np.uint64(2 ** 64 - 1)) and np.all(keys[np.isfinite(x)] != np.uint64(2 ** 64 - 1))
    fk = keys[np.isfinite(x)]
    order = np.argsort(fk, kind="stable")
    assert np.array_equal(finite[order], np.sort(finite))                   # key order is value order (-0 == +0 as values)
    back = np.array([ps.ps_value(int(k)) for k in fk])
    assert np.array_equal(back.view(np.uint64), finite.view(np.uint64))     # and the key gives the very bits back
    assert ps.ps_key(-0.0) < ps.ps_key(0.0)
    for m in (1, 2, 3, 64, 777, finite.size):
        y = np.ascontiguousarray(rs.permutation(finite)[:m])
        y_all = np.ascontiguousarray(rs.permutation(np.concatenate([y, [np.nan, np.inf, -np.inf]])))
        ranks = np.arange(m, dtype=np.int64) if m <= 64 else np.unique(np.concatenate([[0, m - 1], rs.randint(0, m, 40)])).astype(np.int64)
        out = np.empty(ranks.size)
        got_m = ps.ps_select(y_all.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), y_all.size,
                             ranks.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), ranks.size,
                             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert got_m == m
        assert np.array_equal(out, np.sort(y)[ranks]), m
    lo, hi, fr = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
    for m in SIZES:                                                        # the device's rank rule is user_models.quantile_ranks
        for q in PROBS:
            ps.ps_ranks(m, q, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(fr))
            pos = (m - 1) * q
            assert (lo.value, hi.value) == (int(np.floor(pos)), int(np.ceil(pos))) and fr.value == pos - np.floor(pos)


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _ab_population(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([rs.uniform(0.1, 2, n), rs.uniform(0.05, 1, n), rs.uniform(0.005, 0.05, n)])


def _rob_population(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([RB.K_TRUE[0] * 10.0 ** rs.uniform(-1, 1, n), RB.K_TRUE[1] * 10.0 ** rs.uniform(-1, 1, n),
                            rs.uniform(0.005, 0.05, n)])


def _set_case(pkg, eng, method):
    """RK45: CONSECUTIVE_REACTIONS_AB on _ab_data's ragged data; BDF: ROBERTSON_AC on Robertson's.  Returns the data design,
    a new design (other times, a row cut short, an initial concentration not among the data's) and a population maker."""
    if method == "RK45":
        t, obs, A0, _, _, scale = _ab_data()
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=scale)
        t_new = np.tile(np.linspace(0.0, 14.0, 41), (3, 1))
        t_new[1, 17:] = np.nan
        return t, A0[:, None], t_new, np.array([[0.75], [1.0], [3.0]]), _ab_population
    rs = np.random.RandomState(4)
    t = RB.T.copy()
    t[3, 12:] = np.nan
    obs = rs.uniform(0, 1, t.shape + (2,))
    obs[rs.uniform(size=obs.shape) < 0.1] = np.nan
    eng.set_prior(ROB_PRIORS)
    eng.set_model_user(pkg.user_models.ROBERTSON_AC, 3, t, obs, cond=RB.A0[:, None], rtol=RB.RTOL, atol=RB.ATOL, method="BDF",
                       obs_scale=(1.0, 0.02))
    t_new = np.tile(np.linspace(0.0, 60.0, 25), (2, 1))
    t_new[0, 9:] = np.nan
    return t, RB.A0[:, None], t_new, np.array([[0.8], [1.2]]), _rob_population


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_predict_at_without_a_design_is_predict_user_bit_for_bit(pkg, method):
    n = 300
    with pkg.HipEngine(128, 3, device=0) as eng:          # n > n_local: three chunks
        *_, pop = _set_case(pkg, eng, method)
        th = pop(n, 1)
        _, pred, info = eng.predict_user(th)
        pred_at, info_at = eng.predict_user_at(th)
    assert pred_at.shape == pred.shape
    assert np.array_equal(pred_at.view(np.uint64), pred.view(np.uint64))
    assert info_at == info and info["rk_attempts"] > 0


def _ab_scipy(th, t, A0):
    from scipy.integrate import solve_ivp
    ref = np.full((th.shape[0],) + t.shape + (2,), np.nan)
    for p, (k1, k2, _) in enumerate(th):
        for e in range(t.shape[0]):
            te = t[e][~np.isnan(t[e])]
            sol = solve_ivp(lambda _t, y: [-k1 * y[0], k1 * y[0] - k2 * y[1]], [te[0], te[-1]], [A0[e], 0.0], method="RK45",
                            t_eval=te, rtol=1e-3, atol=1e-6)
            ref[p, e, :te.size] = sol.y.T
    return ref


@pytest.mark.gpu
def test_a_new_design_follows_scipy_and_runs_in_groups_past_the_lds_cap(pkg):
    t, obs, A0, _, _, scale = _ab_data()
    n = 96
    th = _ab_population(n, 2)
    t_new = np.tile(np.linspace(0.0, 18.0, 73), (5, 1))       # a finer grid and a longer horizon than the data's 30 times to t = 10
    t_new[3, 40:] = np.nan
    t_new[4] = np.linspace(2.0, 9.0, 73)                       # another initial time
    A0_new = np.array([1.0, 2.0, 0.5, 1.5, 3.25])            # 3.25 is no experiment of the data
    with pkg.HipEngine(64, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=scale)
        lk0, pred0, _ = eng.predict_user(th)
        pred, info = eng.predict_user_at(th, t_new, A0_new[:, None])
        lk1, pred1, _ = eng.predict_user(th)                                   # the data side is as it was
        assert np.array_equal(lk0, lk1) and np.array_equal(pred0.view(np.uint64), pred1.view(np.uint64))
        ref = _ab_scipy(th, t_new, A0_new)
        assert info["n_failed"] == 0 and pred.shape == (n, 5, 73, 2)
        assert np.array_equal(np.isnan(pred), np.isnan(ref))                     # NaN exactly past the short row's end
        assert np.isnan(pred[:, 3, 40:]).all() and not np.isnan(pred[:, 3, :40]).any()
        err = np.nanmax(np.abs(pred - ref))
        print(f"new design against solve_ivp(RK45): max |pred - ref| = {err:.3g}")
        assert err < 1e-9
        # 70 rows of 73 times: more than the kernel's LDS table holds at once (the same rows as DATA are refused)
        rs = np.random.RandomState(3)
        t_big = np.tile(np.linspace(0.0, 12.0, 73), (70, 1)) * rs.uniform(0.5, 1.5, (70, 1))
        t_big[11, 60:] = np.nan
        c_big = rs.uniform(0.3, 3.0, (70, 1))
        with pytest.raises(pkg.SmcError, match="too large"):
            with pkg.HipEngine(64, 3, device=0) as e2:
                e2.set_prior(PRIORS)
                e2.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t_big, np.zeros((70, 73, 2)), cond=c_big)
        big, binfo = eng.predict_user_at(th, t_big, c_big)
        by_hand = np.concatenate([eng.predict_user_at(th, t_big[a:a + 35], c_big[a:a + 35])[0] for a in (0, 35)], axis=1)
        assert binfo["n_failed"] == 0 and big.shape == (n, 70, 73, 2)
        assert np.array_equal(big.view(np.uint64), by_hand.view(np.uint64))
        assert np.isnan(big[:, 11, 60:]).all() and not np.isnan(np.delete(big, 11, axis=1)).any()
        # one row that cannot fit is refused with the bytes
        with pytest.raises(pkg.SmcError, match=r"\d+ B needed, \d+ B available"):
            eng.predict_user_at(th, np.linspace(0.0, 1.0, 6000)[None], [[1.0]])
        # the rules are checked before anything reaches the library
        with pytest.raises(ValueError, match="increasing"):
            eng.predict_user_at(th, [[0.0, 1.0, 1.0]], [[1.0]])
        with pytest.raises(ValueError, match="cond_new"):
            eng.predict_user_at(th, [[0.0, 1.0, 2.0]], None)
        # a one-output model of smc_set_model_user predicts on a design too: B of the same reactions
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS, 2, np.nan_to_num(t, nan=11.0), np.zeros(t.shape), cond=A0[:, None])
        one, oinfo = eng.predict_user_at(th, t_new, A0_new[:, None])
    assert oinfo["n_failed"] == 0 and one.shape == (n, 5, 73, 1)
    assert np.array_equal(np.isnan(one[..., 0]), np.isnan(ref[..., 1]))
    assert np.nanmax(np.abs(one[..., 0] - ref[..., 1])) < 1e-9


def _check_summary(pkg, out, pred, probs, n):
    """out of predictive_summary against NumPy on pred (n, n_ex, n_t, n_obs) of the same particles."""
    import warnings
    q = np.asarray(probs)
    m = np.sum(np.isfinite(pred), axis=0)
    assert np.array_equal(out["n_finite"], m)
    some = m > 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lower = np.nanquantile(pred, q, axis=0, method="lower")
        upper = np.nanquantile(pred, q, axis=0, method="higher")
        linear = np.nanquantile(pred, q, axis=0, method="linear")
        mean, sd = np.nanmean(pred, axis=0), np.nanstd(pred, axis=0)
        big = np.maximum(np.nanmax(np.abs(pred), axis=0), 1e-300)             # a cell of zeros: the differences are 0 too
    for name in ("mean", "sd", "lower", "upper", "quantile"):
        assert np.isnan(out[name][..., ~some]).all(), name                        # a cell nobody reached
    assert np.array_equal(out["lower"][:, some].view(np.uint64), lower[:, some].view(np.uint64))
    assert np.array_equal(out["upper"][:, some].view(np.uint64), upper[:, some].view(np.uint64))
    e_mean = np.max(np.abs(out["mean"][some] - mean[some]) / big[some])
    e_sd = np.max(np.abs(out["sd"][some] - sd[some]) / big[some])
    e_q = np.max(np.abs(out["quantile"][:, some] - linear[:, some]) / np.maximum(np.abs(linear[:, some]), 1e-300))
    print(f"mean {e_mean:.3g} (bound {n * EPS:.3g}), sd {e_sd:.3g} (bound {4 * n * EPS:.3g}), quantile {e_q:.3g} (bound {4 * EPS:.3g})")
    assert e_mean <= n * EPS and e_sd <= 4 * n * EPS and e_q <= 4 * EPS
    return int(some.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("design", ["data", "new"])
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_summary_is_numpy_on_the_downloaded_particles(pkg, method, design):
    n = 5000                                                  # not a multiple of 64
    probs = (0.025, 0.25, 0.5, 0.975, 1.0)
    with pkg.HipEngine(n, 3, device=0) as eng:
        t, cond, t_new, cond_new, pop = _set_case(pkg, eng, method)
        kw = {} if design == "data" else {"t": t_new, "cond": cond_new}
        shape = (t if design == "data" else t_new).shape
        eng.upload_particles(pkg.SMC_SET_PRED, pop(n, 10))
        eng.upload_particles(pkg.SMC_SET_FILT, pop(n, 11))
        for which in (pkg.SMC_SET_PRED, pkg.SMC_SET_FILT):
            out = eng.predictive_summary(which, probs=probs, **kw)
            pred, info = eng.predict_user_at(eng.download_particles(which), **kw)
            assert out["mean"].shape == shape + (2,) and out["lower"].shape == (len(probs),) + shape + (2,)
            assert out["n_failed"] == info["n_failed"] == 0 and out["rk_attempts"] == info["rk_attempts"]
            assert out["kernel_ms"]["predict"] > 0 and out["kernel_ms"]["summary"] > 0
            reached = _check_summary(pkg, out, pred, probs, n)
            assert reached == int(np.sum(~np.isnan(t if design == "data" else t_new))) * 2


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["RK45", "BDF"])
def test_failed_solves_leave_the_count_and_the_order_statistics_to_the_finite(pkg, method):
    n = 1000
    rs = np.random.RandomState(8)
    mixed = np.column_stack([rs.uniform(0.2, 3.0, n), np.where(rs.uniform(size=n) < 0.4, 0.9, 0.1), np.full(n, 0.1)])
    failing = mixed.copy()
    failing[:, 1] = 0.9
    tt = np.linspace(0.0, 2.0, 12)[None, :]
    probs = (0.05, 0.5, 0.95)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_model_user(DIVERGING_SOME, 1, tt, np.zeros_like(tt)[..., None], method=method)
        eng.upload_particles(pkg.SMC_SET_PRED, mixed)
        eng.upload_particles(pkg.SMC_SET_FILT, failing)
        for which, th in ((pkg.SMC_SET_PRED, mixed), (pkg.SMC_SET_FILT, failing)):
            out = eng.predictive_summary(which, probs=probs)
            pred, info = eng.predict_user_at(th)
            assert out["n_failed"] == info["n_failed"] == int(np.sum(th[:, 1] > 0.5))
            _check_summary(pkg, out, pred, probs, n)
            m = out["n_finite"][0, :, 0]
            assert np.all(np.diff(m) <= 0) and m[0] == n                       # falls along the row
            if which == pkg.SMC_SET_PRED:
                assert m[-1] == int(np.sum(th[:, 1] <= 0.5)) and 0 < m[-1] < n   # the last time: only those that do not fail
            else:
                assert m[-1] == 0 and np.isnan(out["quantile"][:, 0, -1, 0]).all() and np.isnan(out["mean"][0, -1, 0])


def _bytes_of_one_experiment(pkg, eng, **kw):
    with pytest.raises(pkg.SmcError, match=r"needs \d+ B") as e:
        eng.predictive_summary(max_staging_bytes=1, **kw)
    return int(re.search(r"needs (\d+) B", str(e.value)).group(1))


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.float64).view(np.uint64), np.asarray(b[k], dtype=np.float64).view(np.uint64))
               for k in ("mean", "sd", "lower", "upper", "quantile", "n_finite")) and \
        (a["n_failed"], a["rk_attempts"]) == (b["n_failed"], b["rk_attempts"])


@pytest.mark.gpu
def test_staging_groups_do_not_change_a_bit_and_too_little_is_refused(pkg):
    n = 3000
    with pkg.HipEngine(n, 3, device=0) as eng:
        t, cond, t_new, cond_new, pop = _set_case(pkg, eng, "RK45")
        eng.upload_particles(pkg.SMC_SET_FILT, pop(n, 12))
        for kw in ({}, {"t": t_new, "cond": cond_new}):
            one = eng.predictive_summary(**kw)
            again = eng.predictive_summary(**kw)
            assert _same_bits(one, again)                                        # a repeated call: the same bits
            need = _bytes_of_one_experiment(pkg, eng, **kw)
            n_t = (t_new if kw else t).shape[1]
            assert need >= 2 * n * n_t * 2 * 8                                   # predictions and keys of one experiment
            grouped = eng.predictive_summary(max_staging_bytes=need, **kw)      # room for one experiment, not for two
            assert _same_bits(one, grouped)
            with pytest.raises(pkg.SmcError, match=rf"needs {need} B"):
                eng.predictive_summary(max_staging_bytes=need - 1, **kw)


# the two-output reactions with a cost hint (include/smc_hip.h: smc_user_cost) that puts about four particles in ten of the
# populations below on the stiff list (cost > 220) and one in ten among the solo solves (cost > 3700)
AB_WITH_COST = "__device__ double smc_user_cost(const double *theta) { return theta[0] > 0.9 ? 5000.0 : (theta[0] > 0.8 ? 300.0 : 0.0); }\n"


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["plain", "cost_hint", "bdf"])
def test_summary_leaves_sets_lk_flags_and_work_totals_alone(pkg, model):
    """Two engines run upload / loglik / sweep / sweep / sweep; one of them predicts in between the first two sweeps - both
    summaries, ungrouped and in groups of one experiment, the pointwise summary and predict_user_at on a design of six groups' worth.
    What the predictions run on is not the model's: the sets, lk and flags are untouched by them, and every later sweep is the
    twin's bit for bit.  cost_hint: with stiff_first the scan lists and their alternating counters run in every launch, the
    predictions' too; bdf: the per-item work counters are part of what a launch writes.
    The second sweep runs without early rejection: where a certainly rejected solve stops is not part of the result, so with
    it rk_attempts and the BDF work totals differ between two runs of the same code (see the full-run test below); without it
    every count of the sweep must be the twin's.  The third runs with it again and is held to its results."""
    t, obs, A0, k_true, _, scale = _ab_data(seed=3)
    n = 4096 if model == "plain" else 512
    rs = np.random.RandomState(7)
    th = np.column_stack([k_true[0] * (1 + 0.1 * rs.standard_normal(n)), k_true[1] * (1 + 0.1 * rs.standard_normal(n)),
                          rs.uniform(0.005, 0.03, n)])
    source = pkg.user_models.CONSECUTIVE_REACTIONS_AB + (AB_WITH_COST if model == "cost_hint" else "")
    step = np.diag([0.004, 0.004, 0.002])
    t_new = np.tile(np.linspace(0.0, 12.0, 50), (6, 1))
    design = {"t": t_new, "cond": np.linspace(0.5, 3.0, 6)[:, None]}

    def run(predict):
        with pkg.HipEngine(n, 3, device=0) as eng:
            eng.set_prior(PRIORS)
            eng.set_stiff_first(True)
            eng.set_model_user(source, 2, t, obs, cond=A0[:, None], obs_scale=scale, method="BDF" if model == "bdf" else "RK45")
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            eng.loglik(pkg.SMC_SET_PRED)
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_lk(pkg.SMC_SET_FILT, eng.download_lk(pkg.SMC_SET_PRED))
            mh = eng.mh_step_device_rng(0.5, 1.0, step, 7, 3)
            assert 0 < mh["accepted_now"] < n

            def state():
                return [eng.download_particles(pkg.SMC_SET_PRED), eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_PRED),
                        eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags().astype(np.float64),
                        np.asarray(list(eng.work_totals().values()) if isinstance(eng.work_totals(), dict) else eng.work_totals(), dtype=np.float64)]
            out = {"before": state()}
            if predict:
                eng.predictive_summary(pkg.SMC_SET_FILT)
                eng.predictive_summary(pkg.SMC_SET_PRED, noise=True, seed=5, **design)
                need = _bytes_of_one_experiment(pkg, eng, **design)
                eng.predictive_summary(pkg.SMC_SET_PRED, noise=True, seed=5, max_staging_bytes=need, **design)     # six groups
                eng.pointwise_summary(pkg.SMC_SET_FILT)
                pred, info = eng.predict_user_at(np.concatenate([th, th[:37]]), **design)                           # two chunks
                assert info["n_failed"] == 0 and not np.isnan(pred).any()
            out["after"] = state()
            eng.set_early_reject(False)
            out["mh2"] = eng.mh_step_device_rng(0.5, 1.0, step, 7, 4)
            out["work2"] = eng.user_sweep_counters() if model == "bdf" else None
            out["state2"] = state()
            eng.set_early_reject(True)
            mh3 = eng.mh_step_device_rng(0.5, 1.0, step, 7, 5)
            out["mh3"] = {k: mh3[k] for k in ("accepted_now", "accepted_ever", "n_failed")}
            out["state3"] = state()
        return out
    with_pred, twin = run(True), run(False)
    assert with_pred["before"][4].sum() > 0
    for a, b in zip(with_pred["before"], with_pred["after"]):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # ... and the next sweeps are what they would have been
    assert with_pred["mh2"] == twin["mh2"] and with_pred["mh2"]["n_failed"] == 0 and 0 < with_pred["mh2"]["accepted_now"] < n
    assert with_pred["mh3"] == twin["mh3"] and 0 < with_pred["mh3"]["accepted_now"] < n
    if model == "bdf":
        print(f"BDF work of the second sweep: {with_pred['work2']}")
        assert with_pred["work2"] == twin["work2"] and with_pred["work2"]["steps"] > 0
    for key in ("state2", "state3"):
        for a, b in zip(with_pred[key][:5], twin[key][:5]):      # both sets, both lk, the flags
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), key


@pytest.mark.gpu
def test_noise_is_reproducible_and_has_the_moments_of_the_observation_model(pkg):
    t, obs, A0, _, _, scale = _ab_data()
    n = 65536
    sigma = 0.05
    s_k = np.array([1.0, 3.0])
    probs = (0.025, 0.975)
    seed = 20240229                                             # fixed here, not tuned
    th = np.tile([0.8, 0.3, 0.123], (n, 1))                    # identical particles
    ok = ~np.isnan(t)
    se = 1.0 / np.sqrt(n)
    z975 = 1.959963984540054
    phi = np.exp(-0.5 * z975 ** 2) / np.sqrt(2 * np.pi)
    q_tol = 5 * np.sqrt(0.025 * 0.975 / n) / phi
    assert abs(q_tol - 0.052) < 1e-3
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=s_k, est_sigma=False,
                           sigma_fixed=sigma)
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        pred = eng.predict_user_at(th[:1])[0][0]
        plain = eng.predictive_summary(probs=probs)
        assert np.array_equal(plain["lower"][0][ok], pred[ok]) and np.array_equal(plain["upper"][1][ok], pred[ok])
        assert np.all(plain["sd"][ok] <= 4 * n * EPS * np.abs(pred[ok]).max())
        a = eng.predictive_summary(probs=probs, noise=True, seed=seed)
        b = eng.predictive_summary(probs=probs, noise=True, seed=seed)
        other = eng.predictive_summary(probs=probs, noise=True, seed=seed + 1)
        need = _bytes_of_one_experiment(pkg, eng, probs=probs)
        grouped = eng.predictive_summary(probs=probs, noise=True, seed=seed, max_staging_bytes=need)
        assert _same_bits(a, b) and _same_bits(a, grouped)
        assert not np.array_equal(a["mean"][ok], other["mean"][ok])
        assert np.isnan(a["mean"][~ok]).all()
        dm = (a["mean"] - pred)[ok] / (sigma * s_k)
        ds = a["sd"][ok] / (sigma * s_k) - 1.0
        ql = (a["quantile"][0] - pred)[ok] / (sigma * s_k)
        qu = (a["quantile"][1] - pred)[ok] / (sigma * s_k)
        print(f"fixed sigma: max |mean| {np.abs(dm).max():.3g} (bound {5 * se:.3g}), max |sd - 1| {np.abs(ds).max():.3g} "
              f"(bound {5 * se / np.sqrt(2):.3g}), quantiles off by {max(np.abs(ql + z975).max(), np.abs(qu - z975).max()):.3g} (bound {q_tol:.3g})")
        assert np.abs(dm).max() <= 5 * se and np.abs(ds).max() <= 5 * se / np.sqrt(2)
        assert np.abs(ql + z975).max() <= q_tol and np.abs(qu - z975).max() <= q_tol
        # sigma estimated: half the particles 0.1, half 0.2
        th2 = th.copy()
        th2[: n // 2, 2], th2[n // 2:, 2] = 0.1, 0.2
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, t, obs, cond=A0[:, None], obs_scale=s_k)
        eng.upload_particles(pkg.SMC_SET_FILT, th2)
        c = eng.predictive_summary(probs=probs, noise=True, seed=seed)
        ds2 = c["sd"][ok] / (s_k * np.sqrt((0.01 + 0.04) / 2)) - 1.0
        print(f"two sigmas: max |sd / expected - 1| {np.abs(ds2).max():.3g} (bound {5 * se / np.sqrt(2):.3g})")
        assert np.abs(ds2).max() <= 5 * se / np.sqrt(2)


@pytest.mark.gpu
def test_full_run_returns_the_band_of_the_unmeasured_product(pkg):
    t, obs, A0, k_true, sig_true, scale = _ab_data(seed=0)
    n = 8192
    s = pkg.SMCSettings(n_particle=n, priors=PRIORS)
    obs3 = np.concatenate([obs, np.full(obs.shape[:2] + (1,), np.nan)], axis=2)
    grid = np.linspace(0.0, 12.0, 200)[None, :]
    a0_new = 2.75                                               # a fifth initial concentration
    runs = []
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(PRIORS)
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS_ABC, 2, t, obs3, cond=A0[:, None], obs_scale=(1.0, 3.0, 1.0))
        for predictive in (None, {"t": grid, "cond": [[a0_new]], "probs": (0.025, 0.5, 0.975)}):
            runs.append(pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3, predictive=predictive))
        with pytest.raises(ValueError, match="user model"):
            eng.model = ("mm", 4, 30)
            pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3, predictive={})
    plain, out = runs
    assert "predictive" not in plain and out["gamma"] == 1.0
    assert set(out) == set(plain) | {"predictive"}
    assert np.array_equal(out["p_pred"], plain["p_pred"]) and np.array_equal(out["lk"], plain["lk"])
    assert out["logZ"] == plain["logZ"] and out["step"] == plain["step"] and len(out["records"]) == len(plain["records"])
    assert [r["gamma_new"] for r in out["records"]] == [r["gamma_new"] for r in plain["records"]]
    assert [(r["last_j"], r["n_accept"], r["n_offspring"]) for r in out["records"]] == \
        [(r["last_j"], r["n_accept"], r["n_offspring"]) for r in plain["records"]]
    # the counts of the run; not wall times, and not the RK45 attempts: two runs of the same code, neither with predictive=, did
    # not share those to the last unit (7800248 against 7800189; early rejection is on, and where a certainly rejected solve
    # stops is not part of the result)
    skip = ("rk_attempts", "rk_attempts_mh", "ess_search_s")
    assert {k: v for k, v in out["stats"].items() if k not in skip} == {k: v for k, v in plain["stats"].items() if k not in skip}
    pr = out["predictive"]
    assert pr["quantile"].shape == (3, 1, 200, 3) and pr["n_failed"] == 0 and np.all(pr["n_finite"] == n)
    assert np.all(pr["lower"] <= pr["quantile"]) and np.all(pr["quantile"] <= pr["upper"])
    width = pr["quantile"][2, 0, 1:, 2] - pr["quantile"][0, 0, 1:, 2]
    assert np.all(width > 0)                                                    # past t = 0, where C = 0 for every particle
    tt = grid[0]
    c_true = a0_new * (1 - (k_true[1] * np.exp(-k_true[0] * tt) - k_true[0] * np.exp(-k_true[1] * tt)) / (k_true[1] - k_true[0]))
    off = np.max(np.abs(pr["quantile"][1, 0, :, 2] - c_true))
    print(f"median of C against the closed form: {off:.3g} (bound 0.02); widest 95 % band {width.max():.3g}")
    assert off < 0.02
