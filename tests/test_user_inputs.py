"""Time-varying measured inputs of a user model (include/smc_hip.h: smc_set_model_user5, smc_input; csrc/user_input.h;
user_models.input_layout / input_value; HipEngine.set_model_user(inputs=)).  The models, data, exact solutions, SciPy references
and the K table live in tests/forced_linear_model.py.

CPU part: every refusal of the data rules, in NumPy and through smc_user_input_check, in the same words; input_value against
np.interp within the derived bound 8 * 2^-53 * max(|u[j]|, |u[j+1]|) (slope, product, sum and t - tk[j] each contribute at most
half an ulp relative to a quantity no larger than 2 max(|u[j]|, |u[j+1]|)), exact at knots and inside its bracket; the exact
solutions against F1's closed form; SciPy within the committed K; SciPy's RK45 insensitive to how the input is rounded; the
sources compile for gfx950 and F1's source without inputs is refused with the stated message.

GPU part: the lookup alone through a model whose outputs are smc_input itself (equal at knots, inside the bracket, within the
derived bound, under RK45 and BDF, on the data's and on a design's inputs); F1 - F3 within K (atol + rtol |y|) of the exact
solution; SciPy restated; the likelihood as its formula; a Metropolis sweep bit for bit with and without early rejection; the
predictive summary with design inputs; inputs=None against smc_set_model_user5 with n_in = 0; a short run_smc on F1.

Measured on an MI355X (tolerance units to the exact solution / K; distance to SciPy; BDF: device / SciPy steps, LU, Jacobians):
    F1 22.88 / 45.763   1.2e-11
    F2  8.51 / 17.029   15961 / 15956   6625 / 6622   1702 / 1697
    F3  6.03 / 10.407   243577 / 243416   55947 / 55882   9322 / 9269
The likelihood lies within 1.1e-14 of its formula in every case; run_smc on F1 (1024 particles, seed 3) ends with the planted
parameters 0.83, 0.49 and 0.85 posterior standard deviations from the posterior mean, logZ = 51.94."""
import ctypes

import numpy as np
import pytest

import forced_linear_model as FM
from test_user_model_multiobs import _np_loglik
from test_user_predictive import _check_summary

ALL = list(FM.CASES)
EPS = np.finfo(float).eps
_dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- CPU: the data rules -----------------------------------------------------------------------------------------------

def _good(n_ex=2, n_knot=4, n_in=2):
    t = np.tile(np.arange(n_knot, dtype=np.float64), (n_ex, 1))
    return t, np.ones((n_ex, n_knot, n_in))


def _refusals():
    out = []
    t, u = _good(); t[1, 1] = np.nan
    out.append((t, u, "row 1 of in_t has a NaN knot before a number at knot 2"))
    t, u = _good(); t[0, :] = np.nan
    out.append((t, u, "row 0 of in_t has no finite knot"))
    t, u = _good(); t[1, 2] = t[1, 1]
    out.append((t, u, "row 1 of in_t is not strictly increasing at knot 2"))
    t, u = _good(); t[0, 3] = np.inf
    out.append((t, u, "row 0 of in_t holds an infinite knot at knot 3"))
    t, u = _good(); u[1, 2, 1] = np.nan
    out.append((t, u, "row 1 of in_u is not finite at knot 2 of input 1"))
    t, u = _good(); u[0, 0, 0] = -np.inf
    out.append((t, u, "row 0 of in_u is not finite at knot 0 of input 0"))
    t, u = _good(); u[0, 1, 1], u[0, 2, 1], t[0, 2] = 1e308, -1e308, 1.0 + 1e-6
    out.append((t, u, "row 0 of in_u has a slope that overflows at knot 2 of input 1"))
    t, u = _good(n_in=9)
    out.append((t, u, "n_in = 9 outside 1 .. 8 (SMC_USER_MAX_INPUTS)"))
    t, u = _good(n_in=1)
    out.append((t, u[:, :, :0], "n_in = 0 outside 1 .. 8 (SMC_USER_MAX_INPUTS)"))
    t, u = _good(n_ex=1, n_knot=4097, n_in=1)
    out.append((t, u, "n_knot = 4097 above the knot capacity 4096 (SMC_USER_MAX_KNOTS)"))
    return out


@pytest.mark.parametrize("case", range(10))
def test_input_layout_refuses_in_the_librarys_words(pkg, case):
    t, u, why = _refusals()[case]
    um, L = pkg.user_models, pkg.lib()
    with pytest.raises(ValueError) as ei:
        um.input_layout(t, u, t.shape[0])
    assert str(ei.value).startswith("input_layout: " + why), str(ei.value)
    tc, uc = np.ascontiguousarray(t), np.ascontiguousarray(u)
    assert L.smc_user_input_check(_dp(tc), _dp(uc), t.shape[0], u.shape[2], t.shape[1]) != 0
    msg = L.smc_last_error(None).decode()
    assert msg.startswith("smc_user_input_check: " + why), msg


def test_input_layout_accepts_and_counts(pkg):
    um, L = pkg.user_models, pkg.lib()
    t, u = _good(n_ex=3, n_knot=5, n_in=3)
    t[1, 3:], t[2, 1:] = np.nan, np.nan
    u[1, 3:], u[2, 2] = np.nan, np.inf                 # ignored past a row's knots
    assert list(um.input_layout(t, u, 3)) == [5, 3, 1]
    assert L.smc_user_input_check(_dp(t), _dp(np.ascontiguousarray(u)), 3, 3, 5) == 0
    assert list(um.input_layout(t, u[:, :, 0], 3)) == [5, 3, 1]          # 2-D u: one input
    with pytest.raises(ValueError, match="in_t must be"):                # shape mismatch
        um.input_layout(t, u[:, :4], 3)
    with pytest.raises(ValueError, match="in_t must be"):
        um.input_layout(t, u, 2)
    for cid in ALL:
        inp = FM.make_inputs(cid)
        um.input_layout(inp["t"], inp["u"], FM.CASES[cid]["n_ex"])
    assert pkg.binding.SMC_USER_MAX_INPUTS == 8 and pkg.binding.SMC_USER_MAX_KNOTS >= 256 and L.smc_abi_version() == 3


# ---- CPU: input_value ---------------------------------------------------------------------------------------------------

def _check_lookup(got, tk, u, t, what):
    """got against np.interp within the derived bound, equal at knots, inside the bracket."""
    ref = np.interp(t, tk, u)
    bound = FM.lookup_bound(tk, u, t)
    assert np.all(np.abs(got - ref) <= bound), (what, np.max(np.abs(got - ref) - bound))
    on = np.isin(t, tk)
    assert np.array_equal(got[on], u[np.searchsorted(tk, t[on])]), what
    lo, hi = FM.bracket(tk, u, t)
    assert np.all((got >= lo) & (got <= hi)), what


def test_input_value_is_np_interp_exact_at_knots_and_inside_its_bracket(pkg):
    iv = pkg.user_models.input_value
    rows = FM.planted_rows(1)
    for r, m in enumerate(FM.PLANTED_M):
        tk, u = rows["t"][r, :m], rows["u"][r, :m, 0]
        if m >= 3:
            assert abs((tk[2] - tk[1]) - 1e-6) < 1e-12
        t = np.concatenate([[tk[0] - 1.0, tk[0] - 1e-300], tk, FM.ULP_UP(tk), FM.ULP_DOWN(tk), [tk[-1] + 1.0, 1e300]])
        _check_lookup(iv(tk, u, t), tk, u, t, f"planted m = {m}")
    planted = rows["u"][~np.isnan(rows["t"])].ravel()
    assert {1e150, 1e-150, -1e150, -1e-150} <= set(planted) and np.any((planted == 0.0) & np.signbit(planted)) and np.any((planted == 0.0) & ~np.signbit(planted))
    rs = np.random.RandomState(11)
    for _ in range(200):
        m = int(rs.randint(1, 40))
        tk = np.cumsum(rs.uniform(1e-3, 2.0, m)) - 3.0
        u = rs.standard_normal(m) * 10.0 ** rs.randint(-5, 6)
        t = np.concatenate([rs.uniform(tk[0] - 1.0, tk[-1] + 1.0, 300), tk])
        _check_lookup(iv(tk, u, t), tk, u, t, "random")
    assert iv([2.0], [7.0], np.array([-1.0, 2.0, 9.0])).tolist() == [7.0, 7.0, 7.0]          # one knot: a constant


# ---- CPU: the references ------------------------------------------------------------------------------------------------

def test_exact_solution_agrees_with_f1s_closed_form():
    """expm of the augmented system against the closed form of a segment, to 1e-3 tolerance units at (1e-9, 1e-6)."""
    t, _, cond = FM.make_data("F1")
    inp = FM.make_inputs("F1")
    th = FM.population("F1")
    ex = FM.reference("F1")["exact"]
    worst = 0.0
    for e in range(3):
        tk, u = FM._row(inp, e)
        for p in range(th.shape[0]):
            cl = FM.f1_closed_row(th[p], cond[e, 0], tk, u, t[e])
            worst = max(worst, np.max(np.abs(cl - ex[p, e, :, 0]) / (FM.TIGHT[1] + FM.TIGHT[0] * np.abs(cl))))
    print(f"F1: expm against the closed form, worst {worst:.3g} tolerance units")
    assert worst <= 1e-3
    m = [int(np.sum(~np.isnan(r))) for r in inp["t"]]
    assert m == [1, 5, 3] and abs((inp["t"][1, 2] - inp["t"][1, 1]) - 1e-6) < 1e-12


def test_the_cases_are_what_the_issue_asks():
    c = FM.CASES
    assert (c["F1"]["method"], c["F1"]["ns"], c["F1"]["n_in"], c["F1"]["n_ex"]) == ("RK45", 1, 1, 3)
    assert (c["F2"]["method"], c["F2"]["ns"], c["F2"]["n_in"], c["F2"]["n_obs"]) == ("BDF", 2, 2, 2) and "smc_user_jac" in c["F2"]["source"]
    assert (c["F3"]["method"], c["F3"]["n_in"], c["F3"]["n_cond"]) == ("BDF", 8, 3) and "smc_user_jac" not in c["F3"]["source"]
    assert "smc_input(cond, 0, t)" in c["F3"]["source"] and "smc_input(cond, 7, t)" in c["F3"]["source"] and "cond[2]" in c["F3"]["source"]
    assert "proportional" in c["F3"]["noise"]
    th = FM.population("F2")
    assert np.all(th[:, 1] / th[:, 0] > 600.0)          # RK45's stability limit h k2 <= 3.3: thousands of steps over 8 time units
    obs = FM.make_data("F2")[1]
    assert np.isnan(obs[..., 1]).any() and not np.isnan(obs[..., 0]).any()
    assert all(v["n"] <= 256 for v in c.values())


@pytest.mark.parametrize("cid", ALL)
def test_scipy_stays_within_the_committed_K_of_the_exact_solution(cid):
    r = FM.reference(cid)["ratio"]
    print(f"{cid}: worst |y_scipy - y_exact| / (atol + rtol |y|) = {r:.4f}, K = {FM.K[cid]}")
    assert r <= FM.K[cid]


def test_scipy_rk45_does_not_depend_on_how_the_input_is_rounded(pkg):
    """The precondition of the 1e-9 restatement bound of the GPU part: SciPy's own F1 results with np.interp and with
    input_value(...) (1 +- 2^-52) agree to 1e-11 max(1, |y|)."""
    iv = pkg.user_models.input_value
    t, _, cond = FM.make_data("F1")
    inp = FM.make_inputs("F1")
    th = FM.population("F1")
    ref = FM.reference("F1")["scipy"]
    worst = 0.0
    for sign in (1.0, -1.0):
        look = lambda tt, tk, uk: float(iv(tk, uk, tt)) * (1.0 + sign * 2.0 ** -52)
        for e in range(3):
            tk, u = FM._row(inp, e)
            for p in range(0, th.shape[0], 2):
                y = FM.scipy_solve("F1", th[p], cond[e], tk, u, t[e], lookup=look)[0]
                worst = max(worst, np.max(np.abs(y - ref[p, e]) / np.maximum(1.0, np.abs(ref[p, e]))))
    print(f"F1: SciPy with np.interp against input_value (1 +- 2^-52): worst {worst:.3g} max(1, |y|)")
    assert worst <= 1e-11


def _check5(pkg, cid, n_in=None):
    c = FM.CASES[cid]
    log = ctypes.create_string_buffer(16384)
    noise = 0 if c["noise"] is None else 1 + int("proportional" in c["noise"])
    rc = pkg.lib().smc_user_model_check5(c["source"].encode(), c["ns"], c["dim"], int(c["method"] == "BDF"), c["n_obs"], noise, c["n_cond"],
                                         c["n_in"] if n_in is None else n_in, c["n_knot"], log, 16384)
    return rc, log.value.decode(errors="replace")


@pytest.mark.parametrize("cid", ALL)
def test_case_sources_compile_for_gfx950(pkg, cid):
    rc, log = _check5(pkg, cid)
    assert rc == 0, log


def test_a_source_with_smc_input_needs_a_model_with_inputs(pkg, tmp_path):
    rc, log = _check5(pkg, "F1", n_in=0)
    assert rc == 1 and "smc_input: this model has no inputs" in log, log
    L, src = pkg.lib(), FM.F1_SOURCE.encode()
    log = ctypes.create_string_buffer(16384)
    assert L.smc_user_model_check3(src, 1, 3, 0, 1, log, 16384) == 1 and b"this model has no inputs" in log.value
    assert L.smc_user_model_check5(src, 1, 3, 0, 1, 0, 1, 9, 4, log, 16384) == 2          # n_in out of range
    assert L.smc_user_model_check5(src, 1, 3, 0, 1, 0, 1, 1, 4097, log, 16384) == 2       # above the knot capacity
    # smc_input and what it needs are in the text only with inputs: without them the dump is dump_source4's, file for file
    plain = pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode()
    a, b, w = tmp_path / "a", tmp_path / "b", tmp_path / "w"
    for d in (a, b, w):
        d.mkdir()
    assert L.smc_user_model_dump_source4(plain, 2, 4, 0, 2, 1, str(a).encode()) == 0
    assert L.smc_user_model_dump_source5(plain, 2, 4, 0, 2, 2, 3, 0, 0, str(b).encode()) == 0
    assert L.smc_user_model_dump_source5(plain, 2, 4, 0, 2, 2, 3, 2, 9, str(w).encode()) == 0
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and "user_input.h" not in names
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
        assert b"smc_input" not in (a / name).read_bytes(), name
    assert sorted(p.name for p in w.iterdir()) == sorted(names + ["user_input.h"])
    head = (w / "smc_user_model.hip").read_text()
    assert "#define SMC_USER_NCOND 3\n#define SMC_USER_NIN 2\n#define SMC_USER_KCAP 16\n" in head


# ---- GPU: the lookup alone ------------------------------------------------------------------------------------------------

LOOKUPS = {"rk45_1x256": ("RK45", 1, 256, FM.PLANTED_M), "bdf_8x256": ("BDF", 8, 256, FM.PLANTED_M),
           "bdf_1x1": ("BDF", 1, 1, (1,)), "rk45_8x8": ("RK45", 8, 8, (8, 5))}


def _lookup_design(rows):
    """t (n_ex, n_t) of planted_times per row (ragged), all-NaN obs."""
    tt = [FM.planted_times(r) for r in rows["t"]]
    t = np.full((len(tt), max(len(x) for x in tt)), np.nan)
    for e, x in enumerate(tt):
        t[e, :len(x)] = x
    return t


def _check_device_lookup(pkg, pred, rows, t, what):
    for e in range(t.shape[0]):
        tk_full = rows["t"][e]
        m = int(np.sum(~np.isnan(tk_full)))
        tk, tt = tk_full[:m], t[e][~np.isnan(t[e])]
        assert np.all(np.isnan(pred[e, tt.size:]))
        for k in range(rows["u"].shape[2]):
            _check_lookup(pred[e, :tt.size, k], tk, rows["u"][e, :m, k], tt, f"{what}: row {e} (m = {m}), input {k}")
            # ... and the NumPy definition itself, within the same bound
            ref = pkg.user_models.input_value(tk, rows["u"][e, :m, k], tt)
            assert np.all(np.abs(pred[e, :tt.size, k] - ref) <= FM.lookup_bound(tk, rows["u"][e, :m, k], tt))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LOOKUPS))
def test_the_lookup_alone(pkg, name):
    method, n_in, n_knot, ms = LOOKUPS[name]
    rows = FM.planted_rows(n_in, n_knot, ms)
    t = _lookup_design(rows)
    n_ex = t.shape[0]
    obs = np.full(t.shape + (n_in,), np.nan)
    th = np.array([[0.3, 0.05], [0.7, 0.02], [1.1, 0.08]])
    with pkg.HipEngine(3, 2, device=0) as eng:
        eng.set_prior({"a": {"dist": "uniform", "low": 0, "high": 2}, "s": {"dist": "uniform", "low": 0, "high": 1}})
        eng.set_model_user(FM.lookup_source(n_in), 1, t, obs, method=method, inputs=rows)
        lk, pred, info = eng.predict_user(th)
        assert info["n_failed"] == 0 and np.all(lk == 0.0)
        assert np.array_equal(pred[0], pred[1], equal_nan=True) and np.array_equal(pred[0], pred[2], equal_nan=True)
        _check_device_lookup(pkg, pred[0], rows, t, name)
        # a design of its own with inputs that differ from the data's: the rows in reverse order, values negated, fewer
        # experiments, and knots stored narrower than the data's where they fit
        keep = slice(None, None, -1) if n_ex > 1 else slice(None)
        design = {"t": rows["t"][keep][:max(1, n_ex - 1)].copy(), "u": -rows["u"][keep][:max(1, n_ex - 1)].copy()}
        t2 = _lookup_design(design)
        pred2, info2 = eng.predict_user_at(th, t=t2, inputs=design)
        assert info2["n_failed"] == 0 and np.array_equal(pred2[0], pred2[2], equal_nan=True)
        _check_device_lookup(pkg, pred2[0], design, t2, name + " (design)")
        with pytest.raises(pkg.SmcError, match="the model has inputs and the design has no matching design inputs"):
            eng.predict_user_at(th, t=t2)


# ---- GPU: F1 - F3 -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def run(request, pkg):
    """One engine per case, compiled once; the population's predictions and sweep are shared by the tests of the case."""
    cid = request.param
    c = FM.CASES[cid]
    t, obs, _ = FM.make_data(cid)
    th = FM.population(cid)
    with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
        try:
            eng.set_prior(FM.priors(cid))
            eng.set_model_user(c["source"], c["ns"], t, obs, **FM.model_kwargs(cid))
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            info = eng.loglik(pkg.SMC_SET_PRED)
            out = {"cid": cid, "c": c, "eng": eng, "th": th, "t": t, "obs": obs, "info": info, "lk": eng.download_lk(pkg.SMC_SET_PRED),
                   "ctr": eng.user_sweep_counters() if c["method"] == "BDF" else None}
            out["lk_p"], out["pred"], out["pinfo"] = eng.predict_user(th)
        except pkg.SmcError as e:      # a device error: no further case is started on a GPU that may have faulted
            pytest.exit(f"case {cid}: {e}", returncode=3)
        yield out


def _cases(ids):
    return pytest.mark.parametrize("run", ids, indirect=True)


@pytest.mark.gpu
@_cases(ALL)
def test_predictions_stay_within_K_of_the_exact_solution(run):
    cid, c, pred, t = run["cid"], run["c"], run["pred"], run["t"]
    assert run["info"]["n_failed"] == 0 and run["pinfo"]["n_failed"] == 0
    assert pred.shape == (c["n"], c["n_ex"], FM.N_T, c["n_obs"])
    assert np.array_equal(np.isnan(pred), np.broadcast_to(np.isnan(t)[None, :, :, None], pred.shape))
    y = FM.reference(cid)["exact"]
    bound = FM.K[cid] * (c["tol"][1] + c["tol"][0] * np.abs(y))
    ok = ~np.isnan(y)
    ratio = np.max(np.abs(pred - y)[ok] / bound[ok])
    print(f"{cid}: worst |pred - y_exact| = {ratio * FM.K[cid]:.4f} tolerance units, K = {FM.K[cid]} ({ratio:.3f} of the bound)")
    assert ratio <= 1.0


@pytest.mark.gpu
@_cases(ALL)
def test_scipy_is_restated(run):
    """F1 (RK45): the outputs within 1e-9 max(1, |pred|) of SciPy's; F2, F3 (BDF): the population's step, LU and Jacobian totals
    within 1 %.  The RK45 bound presupposes test_scipy_rk45_does_not_depend_on_how_the_input_is_rounded."""
    cid, c, pred = run["cid"], run["c"], run["pred"]
    ref = FM.reference(cid)
    y = ref["scipy"]
    ok = ~np.isnan(y)
    dist = np.max(np.abs(pred - y)[ok] / np.maximum(1.0, np.abs(pred[ok])))
    print(f"{cid}: worst |pred - y_scipy| / max(1, |pred|) = {dist:.3g}")
    if c["method"] == "RK45":
        assert dist < 1e-9
        return
    steps, nlu, njev = (int(v) for v in ref["counts"].sum(axis=(0, 1)))
    ctr = run["ctr"]
    print(f"{cid}: device / SciPy steps {ctr['steps']} / {steps}, LU {ctr['lu_factorisations']} / {nlu}, Jacobians {ctr['jacobian_evals']} / {njev}")
    for got, want, what in ((ctr["steps"], steps, "steps"), (ctr["lu_factorisations"], nlu, "LU factorisations"),
                            (ctr["jacobian_evals"], njev, "Jacobian evaluations")):
        assert abs(got - want) <= 0.01 * want, f"{what}: device {got}, SciPy {want}"


def _formula(pkg, cid, pred, th):
    c = FM.CASES[cid]
    t, obs, _ = FM.make_data(cid)
    if c["noise"] is not None:
        return pkg.user_models.noise_loglik(pred, t, obs, th, c["noise"], None)
    return _np_loglik(np.nan_to_num(pred), obs, t, np.ones(c["n_obs"]), th[:, -1])


@pytest.mark.gpu
@_cases(ALL)
def test_likelihood_is_its_formula_on_the_engines_own_outputs(pkg, run):
    cid, th = run["cid"], run["th"]
    assert np.array_equal(run["lk"], run["lk_p"]) and run["info"]["rk_attempts"] == run["pinfo"]["rk_attempts"]
    assert np.all(np.isfinite(run["lk"]))
    ref = _formula(pkg, cid, run["pred"], th)
    err = np.max(np.abs(run["lk"] - ref) / np.maximum(1.0, np.abs(ref)))
    print(f"{cid}: worst |lk - formula(pred)| / max(1, |lk|) = {err:.3g}")
    assert err <= 1e-9


@pytest.mark.gpu
@_cases(ALL)
def test_metropolis_sweep_is_the_same_with_early_rejection(pkg, run):
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    step = np.diag(2e-3 * np.array([p["high"] for p in FM.priors(cid).values()]) / 3.0)
    out = []
    for on in (False, True):
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        eng.upload_lk(pkg.SMC_SET_FILT, run["lk"])
        eng.set_early_reject(on)
        mh = eng.mh_step_device_rng(0.5, 1.0, step, 7, 3)
        out.append((mh, eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT), eng.download_accept_flags()))
    eng.set_early_reject(True)
    (m0, p0, l0, a0), (m1, p1, l1, a1) = out
    print(f"{cid}: accepted {m0['accepted_now']} of {c['n']}; attempts {m0['rk_attempts']} without, {m1['rk_attempts']} with early rejection")
    assert m0["n_failed"] == 0 and m1["n_failed"] == 0
    assert m0["accepted_now"] == m1["accepted_now"] and np.array_equal(a0, a1) and np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert m1["rk_attempts"] <= m0["rk_attempts"]


@pytest.mark.gpu
@_cases(["F2"])
def test_predictive_summary_with_design_inputs(pkg, run):
    """An explicit design with inputs of its own: the summary equals that of predict_user_at of the downloaded set; the exact
    solution under the design's inputs holds too (the design's table, not the data's, was read)."""
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    rs = np.random.RandomState(5)
    t2 = np.array([[0.25, 1.0, 2.5, 4.0, 6.5], [0.0, 0.5, 3.0, np.nan, np.nan], [1.0, 2.0, 3.0, 5.0, 9.0]])
    cond2 = rs.uniform(0.2, 1.5, (3, c["n_cond"]))
    design = {"t": np.array([[0.0, 1.0, 3.0, 6.0], [0.5, 2.0, np.nan, np.nan], [2.0, np.nan, np.nan, np.nan]]),
              "u": rs.uniform(0.0, 3.0, (3, 4, c["n_in"]))}
    probs = (0.0, 0.025, 0.5, 1.0)
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    out = eng.predictive_summary(pkg.SMC_SET_PRED, probs=probs, t=t2, cond=cond2, inputs=design)
    pred, info = eng.predict_user_at(eng.download_particles(pkg.SMC_SET_PRED), t=t2, cond=cond2, inputs=design)
    assert out["n_failed"] == 0 and info["n_failed"] == 0 and out["rk_attempts"] == info["rk_attempts"]
    reached = _check_summary(pkg, out, pred, probs, c["n"])
    assert reached == int(np.sum(~np.isnan(t2))) * c["n_obs"]
    y = FM.exact_outputs(cid, th, t2, cond2, design)
    ok = ~np.isnan(y)
    assert np.max(np.abs(pred - y)[ok] / (FM.K[cid] * (c["tol"][1] + c["tol"][0] * np.abs(y[ok])))) <= 1.0
    with pytest.raises(pkg.SmcError, match="the model has inputs and the design has no matching design inputs"):
        eng.predictive_summary(pkg.SMC_SET_PRED, probs=probs, t=t2, cond=cond2)
    with pytest.raises(pkg.SmcError, match="the model has inputs and the design has no matching design inputs"):
        eng.predict_user_at(th, t=t2, cond=cond2)
    # the data's own design needs nothing
    again = eng.predict_user_at(th)[0]
    assert np.array_equal(again, run["pred"], equal_nan=True)


@pytest.mark.gpu
def test_no_inputs_is_the_existing_path_bit_for_bit(pkg):
    """inputs=None on a source without smc_input against the same model through smc_set_model_user5 with n_in = 0."""
    import linear_chain_model as LC
    L = pkg.lib()
    out = {}
    for cid in ("R3", "R4"):          # the sigma rule with obs_scale (smc_set_model_user3) and a noise model (smc_set_model_user4)
        c = LC.CASES[cid]
        t, obs, cond = (np.ascontiguousarray(a) for a in LC.make_data(cid))
        th = LC.population(cid)
        for how in ("engine", "user5"):
            with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
                eng.set_prior(LC.priors(cid))
                eng.set_model_user(LC.case_source(cid), c["ns"], t, obs, **LC.model_kwargs(cid))
                if how == "user5":
                    scale = None if c["scale"] is None else np.ascontiguousarray(c["scale"], dtype=np.float64)
                    ai = af = pi = pf = None
                    if c["noise"] is not None:
                        ai, af, pi, pf = pkg.user_models.noise_layout(c["noise"], c["n_obs"], c["dim"])
                    ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
                    fp = lambda a: None if a is None else _dp(a)
                    rc = L.smc_set_model_user5(eng.ctx, LC.case_source(cid).encode(), c["ns"], c["n_obs"], _dp(t), _dp(obs), _dp(cond),
                                               fp(scale), c["n_ex"], LC.N_T, 3, ip(ai), fp(af), ip(pi), fp(pf), c["rtol"], c["atol"],
                                               int(c["method"] == "BDF"), 1, 5.0, None, None, 0, 0)
                    assert rc == 0, L.smc_last_error(eng.ctx)
                eng.upload_particles(pkg.SMC_SET_PRED, th)
                info = eng.loglik(pkg.SMC_SET_PRED)
                out[cid, how] = (eng.download_lk(pkg.SMC_SET_PRED), info["rk_attempts"])
        assert np.array_equal(out[cid, "engine"][0], out[cid, "user5"][0]) and out[cid, "engine"][1] == out[cid, "user5"][1]
        assert np.all(np.isfinite(out[cid, "engine"][0]))


@pytest.mark.gpu
def test_a_short_run_smc_on_f1_finds_the_planted_parameters(pkg):
    c = FM.CASES["F1"]
    t, obs, _ = FM.make_data("F1")
    n = 1024
    with pkg.HipEngine(n, c["dim"], device=0) as eng:
        eng.set_prior(FM.priors("F1"))
        eng.set_model_user(c["source"], c["ns"], t, obs, **FM.model_kwargs("F1"))
        out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=FM.priors("F1")), rng="device", seed_device=3, verbose=False)
    assert out["gamma"] == 1.0 and np.isfinite(out["logZ"])
    mean, sd = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
    z = (np.array(FM.THETA_TRUE["F1"]) - mean) / sd
    print(f"F1 run_smc: mean {mean}, sd {sd}, planted {FM.THETA_TRUE['F1']}: {z} posterior standard deviations, logZ {out['logZ']:.3f}")
    assert np.all(np.abs(z) <= 4.0)
