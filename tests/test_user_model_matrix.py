"""The user-model kernel family (csrc/user_rk45_kernel.h, user_bdf_kernel.h, user_item_ops.h, user_obs_args.h, user_model.hip) over a covering set
of its instantiations - 1 .. 8 states, 1 .. 8 outputs, 3 .. 8 parameters with a noise parameter at index 7, three condition
numbers, analytic and numerical Jacobians, every likelihood - on a linear chain whose solution is known exactly
(tests/linear_chain_model.py, where the 14 cases, their data, the exact solutions, the bounds K and the swap counts live).

CPU part: the reference against itself (expm against the symmetrised eigen-decomposition, the right-hand side against A y, real
negative eigenvalues), the K table, SciPy's RK45 insensitive to the rounding of the right-hand side, the pivoting condition -
with gain = 1e4 every BDF solve of SciPy swaps rows in at least one LU factorisation, so the device's row exchange runs and
must agree between lu_factor and lu_solve (not: that pivoting is needed; linear_chain_model's text) - and that the sources
compile for gfx950.

GPU part, per case on one engine (compiled once): predictions within K (atol + rtol |y|) of the exact solution; SciPy's
solver as a restatement (RK45: the outputs to 1e-9; BDF: steps, LU factorisations and Jacobian evaluations, population totals
within 1 % - every BDF case uses the totals form); the likelihood as its formula on the engine's own outputs; a Metropolis
sweep bit for bit with and without early rejection; the predictive summary for the three eight-output cases.

Measured on an MI355X (tolerance units to the exact solution / K; distance to SciPy; BDF: steps, LU, Jacobians - the device has
SciPy's totals exactly in all seven cases):
    R1 2.818 / 5.636  3.2e-14      B1 2.739 / 5.478  1.3e-15   3485  1070 130
    R2 0.952 / 3.777  1.7e-13      B2 3.349 / 8.618  7.8e-14   5005  1592 126
    R3 0.173 / 2.338  1.9e-15      B3 1.580 / 16.036 4.4e-15  19889  4060 237
    R4 0.572 / 4.664  4.9e-14      B4 0.971 / 5.419  3.1e-15    253    71   4
    R5 0.247 / 2.286  6.8e-16      B5 1.406 / 7.232  4.1e-15  28152  7746 514
    R6 0.461 / 23.987 2.3e-14      B6 1.319 / 7.664  2.4e-15   7178  1963 128
    R7 0.121 / 1.857  1.2e-15      B7 1.479 / 76.219 1.9e-14  25610  4907 130
The likelihood lies within 8.2e-15 of its formula in every case.

Mutations of the kernels, each on a copy of the library: lu_factor without its row exchange (piv still recorded) fails
test_scipy_is_restated of B2, B4 and B7 (7.7e6 steps against 5005, 89311 against 253, 7.4e6 against 25610); m_ek read at
8 e + k - 1 fails R7's Metropolis sweep (41 accepted without, 40 with early rejection) and passes R4 and B2; an lu_factor that
never pivots (p = k, consistent with lu_solve) passes B2, B4 and B7 - see linear_chain_model's text."""
import ctypes

import numpy as np
import pytest

import linear_chain_model as LC
from test_user_model_multiobs import _np_loglik
from test_user_predictive import _check_summary

ALL = list(LC.CASES)
BDF_CASES = [c for c in ALL if LC.CASES[c]["method"] == "BDF"]
RK45_CASES = [c for c in ALL if LC.CASES[c]["method"] == "RK45"]
GAIN_BDF = [c for c in BDF_CASES if LC.CASES[c]["gain"] != 1.0]
CPU_COMPILE = ["R1", "R2", "R3", "R4", "B1", "B2", "B7"]      # the four cheapest RK45 cases and three BDF ones; the GPU part compiles all 14
EPS = np.finfo(float).eps


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_the_matrix_covers_every_state_and_output_count():
    cs = list(LC.CASES.values())
    assert len(ALL) == 14 and ALL[:3] == list(LC.SUMMARY_CASES)
    assert {c["ns"] for c in cs} == set(range(1, 9)) and {c["n_obs"] for c in cs} == set(range(1, 9))
    assert {c["dim"] for c in cs} >= {3, 4, 5, 6, 8}
    seven = ("param", 7)
    for method in ("RK45", "BDF"):
        noisy = [c for c in cs if c["method"] == method and c["noise"]]
        assert len({c["ns"] for c in cs if c["method"] == method}) == 7
        # dim = 8 with parameter 7 in the noise model, and a noise model next to eight states
        assert any(c["dim"] == 8 and seven in c["noise"]["additive"] + c["noise"].get("proportional", []) for c in noisy)
        assert any(c["ns"] == 8 for c in noisy)
        # the planted invalid particles go through the last output's parameters: in one additive and one proportional
        # specification at least, no other output reads that parameter (a validity check that stops early would pass otherwise)
        for part in ("additive", "proportional"):
            specs = [c["noise"][part] for c in noisy if part in c["noise"]]
            assert any(sp[-1][0] == "param" and sp[-1] not in sp[:-1] for sp in specs), (method, part)
    assert any(seven in c["noise"]["additive"] for c in cs if c["noise"])
    assert any(seven in c["noise"].get("proportional", []) for c in cs if c["noise"])
    assert all(make[2].shape == (c["n_ex"], 3) for c, make in ((LC.CASES[i], LC.make_data(i)) for i in ALL))      # n_cond = 3


@pytest.mark.parametrize("cid", ALL)
def test_the_two_exact_solutions_agree_and_the_model_is_its_matrix(cid):
    """expm against the eigen-decomposition, within 1e-3 of atol + rtol |y| at the tight pair (1e-9, 1e-6) whatever the case's
    own tolerances; the flux-by-flux right-hand side against A y; real negative eigenvalues."""
    c = LC.CASES[cid]
    t, obs, cond = LC.make_data(cid)
    a, b = LC.exact_states(cid), LC.exact_states(cid, LC.exact_eig)
    assert np.array_equal(np.isnan(a[..., 0]), np.broadcast_to(np.isnan(t), a.shape[:3])) and np.array_equal(np.isnan(a), np.isnan(b))
    worst = np.nanmax(np.abs(a - b) / (LC.TIGHT[1] + LC.TIGHT[0] * np.abs(a)))
    print(f"{cid}: expm against the eigen-decomposition, worst {worst:.3g} tolerance units")
    assert worst <= 1e-3
    rs = np.random.RandomState(3)
    for th in LC.population(cid)[:8]:
        A = LC.matrix(th[0], th[1], c["ns"], cond[0, 1], cond[0, 2])
        y = rs.uniform(0.0, 2.0, c["ns"])
        np.testing.assert_allclose(LC.rhs(0.0, y, th[0], th[1], cond[0, 1], cond[0, 2]), A @ y, rtol=0, atol=8 * EPS * np.abs(A).max() * 2.0)
        ev = np.linalg.eigvals(A)
        assert np.all(ev.imag == 0.0) and np.all(ev.real < 0.0)
    # the data: a pair of times 1e-6 apart, t[e][0] not always 0, a cut row and a single-time row where NaN is allowed
    assert abs((t[0, 5] - t[0, 4]) - 1e-6) < 1e-12 and (c["n_ex"] == 1 or t[1, 0] == 0.5)
    if not c["obs2d"] and c["n_ex"] >= 3:
        assert np.sum(~np.isnan(t[1])) == 7 and np.sum(~np.isnan(t[2])) == 1
        assert 0.0 < np.mean(np.isnan(obs[~np.isnan(t)])) < 0.3          # about 15 %, of as few as 42 values


@pytest.mark.parametrize("cid", ALL)
def test_scipy_stays_within_the_committed_K_of_the_exact_solution(cid):
    r = LC.reference(cid)["ratio"]
    print(f"{cid}: worst |y_scipy - y_exact| / (atol + rtol |y|) = {r:.4f}, K = {LC.K[cid]}")
    assert r <= LC.K[cid]


@pytest.mark.parametrize("cid", RK45_CASES)
def test_scipy_rk45_does_not_amplify_rounding(cid):
    """The restatement bound of the GPU part, 1e-9 max(1, |out|), is about the kernel only where SciPy's own result does not
    depend on how the right-hand side is rounded: its solves of the flux-by-flux and of the A y form must agree a hundred
    times closer than that.  (Past RK45's stability limit they do not: linear_chain_model's text on R7's times.)"""
    r = LC.reference(cid)["rounding"]
    print(f"{cid}: SciPy, flux-by-flux against A y: worst {r:.3g} max(1, |out|)")
    assert r <= 1e-11


@pytest.mark.parametrize("cid", GAIN_BDF)
def test_with_gain_every_scipy_bdf_solve_swaps_rows(cid):
    with_swap, solves, lu_swapped, lus = LC.swap_counts(cid)
    print(f"{cid}: {with_swap} of {solves} solves swap, {lu_swapped} of {lus} factorisations; committed {LC.SWAPS[cid]}")
    assert solves > 0 and with_swap == solves


def _compile(pkg, cid):
    c = LC.CASES[cid]
    L, src, m = pkg.lib(), LC.case_source(cid).encode(), int(c["method"] == "BDF")
    log = ctypes.create_string_buffer(16384)
    if c["noise"] is not None:
        rc = L.smc_user_model_check4(src, c["ns"], c["dim"], m, c["n_obs"], int("proportional" in c["noise"]), log, 16384)
    elif c["obs2d"]:
        rc = L.smc_user_model_check2(src, c["ns"], c["dim"], m, log, 16384)
    else:
        rc = L.smc_user_model_check3(src, c["ns"], c["dim"], m, c["n_obs"], log, 16384)
    return rc, log.value.decode(errors="replace")


@pytest.mark.parametrize("cid", CPU_COMPILE)
def test_case_sources_compile_for_gfx950(pkg, cid):
    rc, log = _compile(pkg, cid)
    assert rc == 0, log


def test_every_noise_specification_is_accepted(pkg):
    um = pkg.user_models
    for cid, c in LC.CASES.items():
        assert ("smc_user_jac" in LC.case_source(cid)) == bool(c["jac"]) and ("smc_user_obs_vec" in LC.case_source(cid)) != c["scalar"]
        if c["noise"] is None:
            continue
        ai, af, pi, pf = um.noise_layout(c["noise"], c["n_obs"], c["dim"])
        ip = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        fp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert pkg.lib().smc_user_noise_check(c["n_obs"], c["dim"], ip(ai), fp(af), ip(pi), fp(pf)) == 0, cid
        # not the degenerate specification that takes the smc_set_model_user3 path
        assert pi is not None or not (np.all(ai == c["dim"] - 1) or np.all(ai == -1)), cid


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _bar(lk, ref):
    return np.max(np.abs(lk - ref) / np.maximum(1.0, np.abs(ref)))


def _planted(cid, th):
    """th with particles whose likelihood is -inf, through the LAST output's parameters: a_k = 0, b_k < 0; sigma = 0 and < 0."""
    c = LC.CASES[cid]
    bad = th.copy()
    if c["noise"] is not None:
        kind, j = c["noise"]["additive"][-1]
        assert kind == "param"
        bad[0, j] = 0.0
        rows = [0]
        if "proportional" in c["noise"]:
            kind, j = c["noise"]["proportional"][-1]
            assert kind == "param"
            bad[1, j] = -1e-3
            rows.append(1)
        return bad, rows
    bad[0, -1], bad[1, -1] = 0.0, -0.01
    return bad, [0, 1]


def _formula(pkg, cid, pred, th):
    """The case's likelihood from model outputs pred (n, n_ex, n_t, n_obs)."""
    c = LC.CASES[cid]
    t, obs, _ = LC.make_data(cid)
    if c["noise"] is not None:
        return pkg.user_models.noise_loglik(pred, t, obs, th, c["noise"], c["scale"])
    sigma = th[:, -1] if c["sigma_fixed"] is None else np.full(th.shape[0], c["sigma_fixed"])
    if c["obs2d"]:        # the one-output formula (Micmem_likelihood.py): every experiment has n_t observations
        r2 = np.sum((obs[None] - pred[..., 0]) ** 2, axis=(1, 2))
        return c["n_ex"] * (-0.5 * LC.N_T) * np.log(2 * np.pi * sigma * sigma) - r2 / (2 * sigma * sigma)
    scale = np.ones(c["n_obs"]) if c["scale"] is None else np.asarray(c["scale"])
    return _np_loglik(np.nan_to_num(pred), obs, t, scale, sigma)


@pytest.fixture(scope="module")
def run(request, pkg):
    """One engine per case, compiled once; the clean population's predictions and sweep are shared by the tests of the case."""
    cid = request.param
    c = LC.CASES[cid]
    t, obs, _ = LC.make_data(cid)
    th = LC.population(cid)
    with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
        try:
            eng.set_prior(LC.priors(cid))
            eng.set_model_user(LC.case_source(cid), c["ns"], t, obs, **LC.model_kwargs(cid))
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
    assert pred.shape == (c["n"], c["n_ex"], LC.N_T, c["n_obs"])
    assert np.array_equal(np.isnan(pred), np.broadcast_to(np.isnan(t)[None, :, :, None], pred.shape))     # NaN exactly past a row's end
    W = LC.weights(c["n_obs"], c["ns"])
    y = LC.reference(cid)["exact"]
    ref = y @ W.T
    bound = LC.K[cid] * ((c["atol"] + c["rtol"] * np.abs(y)) @ np.abs(W).T)
    ok = ~np.isnan(ref)
    ratio = np.max(np.abs(pred - ref)[ok] / bound[ok])
    print(f"{cid}: worst |pred - W y_exact| = {ratio * LC.K[cid]:.4f} tolerance units, K = {LC.K[cid]} ({ratio:.3f} of the bound)")
    assert ratio <= 1.0
    for e in range(c["n_ex"]):
        if np.sum(~np.isnan(t[e])) == 1:       # nothing to integrate: the outputs of y0 = (A0, 0, ...), one rounding each
            assert np.all(np.abs(pred[:, e, 0, :] - LC.A0[e] * W[:, 0]) <= 2 * EPS * LC.A0[e] * W[:, 0])


@pytest.mark.gpu
@_cases(ALL)
def test_scipy_is_restated(run):
    """RK45: the outputs within 1e-9 max(1, |pred|) of SciPy's; BDF: the population's step, LU and Jacobian totals within 1 %.
    Every BDF case uses the totals form.  The RK45 bound presupposes test_scipy_rk45_does_not_amplify_rounding."""
    cid, c, pred = run["cid"], run["c"], run["pred"]
    ref = LC.reference(cid)
    W = LC.weights(c["n_obs"], c["ns"])
    y = ref["scipy"] @ W.T
    ok = ~np.isnan(y)
    dist = np.max(np.abs(pred - y)[ok] / np.maximum(1.0, np.abs(pred[ok])))
    print(f"{cid}: worst |pred - W y_scipy| / max(1, |pred|) = {dist:.3g}")
    if c["method"] == "RK45":
        assert dist < 1e-9
        return
    steps, nlu, njev = (int(v) for v in ref["counts"].sum(axis=(0, 1))[:3])
    ctr = run["ctr"]
    print(f"{cid}: device / SciPy steps {ctr['steps']} / {steps}, LU {ctr['lu_factorisations']} / {nlu}, Jacobians {ctr['jacobian_evals']} / {njev}")
    for got, want, what in ((ctr["steps"], steps, "steps"), (ctr["lu_factorisations"], nlu, "LU factorisations"),
                            (ctr["jacobian_evals"], njev, "Jacobian evaluations")):
        assert abs(got - want) <= 0.01 * want, f"{what}: device {got}, SciPy {want}"
    assert run["info"]["rk_attempts"] >= ctr["steps"] and ctr["newton_iters"] >= ctr["steps"]


@pytest.mark.gpu
@_cases(ALL)
def test_likelihood_is_its_formula_on_the_engines_own_outputs(pkg, run):
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    assert np.array_equal(run["lk"], run["lk_p"]) and run["info"]["rk_attempts"] == run["pinfo"]["rk_attempts"]
    assert np.all(np.isfinite(run["lk"]))
    err = _bar(run["lk"], _formula(pkg, cid, run["pred"], th))
    print(f"{cid}: worst |lk - formula(pred)| / max(1, |lk|) = {err:.3g}")
    assert err <= 1e-9
    if c["n"] == 1:
        return
    bad, rows = _planted(cid, th)
    eng.upload_particles(pkg.SMC_SET_PRED, bad)
    info = eng.loglik(pkg.SMC_SET_PRED)
    lk = eng.download_lk(pkg.SMC_SET_PRED)
    lk_p, pred, pinfo = eng.predict_user(bad)
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    assert np.array_equal(lk, lk_p) and info["rk_attempts"] == pinfo["rk_attempts"] and info["n_failed"] == 0
    assert np.isneginf(lk[rows]).all()
    rest = np.setdiff1d(np.arange(c["n"]), rows)
    assert np.isfinite(lk[rest]).all() and np.array_equal(lk[rest], run["lk"][rest])
    if c["noise"] is not None:
        assert np.isneginf(_formula(pkg, cid, pred, bad)[rows]).all()


@pytest.mark.gpu
@_cases(ALL)
def test_metropolis_sweep_is_the_same_with_early_rejection(pkg, run):
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    step = np.diag([{"k": 2e-3, "add": 1e-5, "prop": 1e-4, "free": 1e-3}[r] for r in LC.roles(cid)])
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
    if c["n"] >= 63:
        assert 0 < m0["accepted_now"] < c["n"]


@pytest.mark.gpu
@_cases(list(LC.SUMMARY_CASES))
def test_predictive_summary_of_eight_outputs(pkg, run):
    c, eng = run["c"], run["eng"]
    probs = (0.0, 0.025, 0.5, 1.0)
    cells = c["n_ex"] * LC.N_T * c["n_obs"]
    assert c["n_obs"] == 8 and cells % 32 != 0 and c["n"] % 64 != 0
    eng.upload_particles(pkg.SMC_SET_PRED, run["th"])
    out = eng.predictive_summary(pkg.SMC_SET_PRED, probs=probs)
    assert out["n_failed"] == 0 and out["rk_attempts"] == run["pinfo"]["rk_attempts"]
    reached = _check_summary(pkg, out, run["pred"], probs, c["n"])
    assert reached == int(np.sum(~np.isnan(run["t"]))) * 8
