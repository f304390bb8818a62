"""State-triggered events of a user model (include/smc_hip.h: STATE-TRIGGERED EVENTS; csrc/user_root.h and the SMC_USER_ROOTS
blocks of the kernel files; user_models.brentq, user_models.root_chain).  The models, data, exact solutions, the chained-SciPy
reference and the K table live in tests/triggered_model.py.

CPU part: user_models.brentq against scipy.optimize.brentq on the cases' own event functions along SciPy's dense outputs - the
root bit for bit, the same number of function calls; the SciPy chain within the committed K of the exact solution, T1's pinned
data time equal to the chain's fire time, before the jump there and after it at the next representable time; the sources
compile for gfx950, every refusal appears with its message, a source without the names dumps the files it has always dumped.

GPU part: T1 - T4 within K (atol + rtol |y|) of the exact solution and within 1e-9 of the SciPy chain (wherever that chain
determines its own tenth digit - triggered_model.CHAIN_BAR: everywhere but for 31 particles of T3 without smc_user_jac); T4's count output equal
to the chain's number of fires at every data time; BDF's step, LU and Jacobian totals equal to the chain's; the data time AT a
fire time; the likelihood as its formula; a Metropolis sweep bit for bit with and without early rejection; a cost hint that
sends particles through the list and the one-per-wave phase against the run without the hint, bit for bit; event functions
that never fire against the model without the names, bit for bit; an explicit design (predict_user_at); a short run_smc on T1;
the two inputs that trip the rules (a jump onto the firing surface, fire 257), each failing its own items only.

The data time at a fire time (T1's pinned pair is not measured: its observations are NaN, so it is predicted and does not
enter the likelihood).  Two correct solvers - SciPy and the device - agree to about 1e-13 along a trajectory, not bit
for bit (contraction, the inverse fifth root), and a root is located to 4 EPS: their fire times differ in the last places.  A
data time placed at the CHAIN's fire time therefore lies, on the device, an ulp or so before or after the device's own fire
time, and either side is right.  So T1's pinned pair (particle 0, row 0, indices 2 and 3) is left out of the comparisons of
the whole population, and the property itself is tested on the device's own fire time, which explicit designs find by
bisection (a design's data times do not move the steps): the largest data time that still sees the state before the jump lies
within 1e-9 of the chain's fire time, holds L there, and the next representable time holds L + D.

The one-rank against two-rank comparison of tests/test_user_sharded.py is not here: its helper is written for that file's
dim = 8 cases (it asserts the dimension and builds engines from linear_chain_model) and does not apply without change.

Measured on an MI355X (tolerance units to the exact solution / K; distance to the SciPy chain, bar 1e-9; BDF: device = SciPy
steps, LU, Jacobians; an explicit design: tolerance units, distance to the chain):
    T1   2.72 /   5.446   3.4e-14                               design 3.28, 1.8e-14
    T2 291.68 / 583.359   8.3e-13
    T3  10.59 /  21.182   4.7e-12    84640  33726  3555         design 9.38, 2.3e-14
    T3N 10.59 /  21.182   3.9e-11    84640  33726  3555         over the 289 particles whose chain is determined; 3.0e-8 over all
    T4   2.72 /   5.435   4.0e-14    fires per row 1218, 0, 1504 = the chain's
The device's fire time of T1's particle 0 is 0x1.86f36462ef26fp+0, the chain's 0x1.86f36462ef270p+0: one ulp apart.  The likelihood
lies within 1.5e-14 of its formula in every case; early rejection saves 257, 188, 265, 157 and 721 of 33904, 33420, 85223, 85223
and 30073 attempts of the sweep; 110 of the 320 particles trip each rule and fail alone; run_smc on T1 (1024 particles, seed 3)
ends with the planted (k, D, sigma) 0.6, 0.6 and 1.0 posterior standard deviations from the posterior mean, logZ = 12.64.
"""
import ctypes

import numpy as np
import pytest

import triggered_model as TM
from test_user_model_multiobs import _np_loglik

ALL = list(TM.CASES)
_SIG = "const double *theta, const double *cond"


# ---- CPU: brentq -------------------------------------------------------------------------------------------------------------

def _active_steps(cid, p, e, limit=6):
    """[(f, t_old, t_new)]: the case's event functions along SciPy's dense outputs, on the steps where solve_ivp would look for a
    root - every accepted step of the first segment on which an event function changes sign in its direction."""
    from scipy.integrate import BDF, RK45
    th, t = TM.population(cid)[p], TM.times(cid)[e]
    m = TM.py_model(cid, th, TM.COND[cid][e])
    cls = RK45 if TM.CASES[cid]["method"] == "RK45" else BDF
    s = cls(m["rhs"], t[0], m["y0"], np.nanmax(t), rtol=TM.tol(cid)[0], atol=TM.tol(cid)[1])
    g = np.array(m["root"](s.t, s.y), dtype=np.float64)
    out = []
    while s.status == "running" and len(out) < limit:
        s.step()
        g_new = np.array(m["root"](s.t, s.y), dtype=np.float64)
        sol = s.dense_output()
        for k, d in enumerate(m["dir"]):
            up, down = g[k] <= 0 <= g_new[k], g[k] >= 0 >= g_new[k]
            if (up and d > 0) or (down and d < 0) or ((up or down) and d == 0):
                out.append(((lambda k, sol: lambda x: float(m["root"](x, sol(x))[k]))(k, sol), s.t_old, s.t))
        g = g_new
        if out:
            break      # a terminal event: the segment ends here
    return out


@pytest.mark.parametrize("cid", ["T1", "T2", "T3", "T4"])
def test_brentq_is_scipys_bit_for_bit_with_the_same_number_of_calls(pkg, cid):
    from scipy.optimize import brentq
    eps4 = 4 * np.finfo(float).eps
    seen = 0
    for p in range(0, TM.N, 16):
        for e in range(3):
            for f, a, b in _active_steps(cid, p, e):
                want, r = brentq(f, a, b, xtol=eps4, rtol=eps4, full_output=True)
                got, calls, iters = pkg.user_models.brentq(f, a, b, full_output=True)
                assert got == want and calls == r.function_calls and iters == r.iterations, (cid, p, e, got, want, calls, r.function_calls)
                assert pkg.user_models.brentq(f, a, b) == want
                seen += 1
    assert seen >= 20
    # the two ends, a sign error, a NaN, and no convergence within the iterations
    assert pkg.user_models.brentq(lambda x: x, 0.0, 1.0, full_output=True) == (0.0, 2, 0)
    assert pkg.user_models.brentq(lambda x: x - 1.0, 0.0, 1.0, full_output=True) == (1.0, 2, 0)
    with pytest.raises(ValueError):
        pkg.user_models.brentq(lambda x: x * x + 1.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        pkg.user_models.brentq(lambda x: float("nan"), 0.0, 1.0)
    with pytest.raises(RuntimeError):
        pkg.user_models.brentq(lambda x: np.cos(x) - x, 0.0, 1.0, maxiter=2)
    for fn, a, b in ((lambda x: np.cos(x) - x, 0.0, 1.0), (lambda x: x ** 3 - 2 * x - 5, 2.0, 3.0), (lambda x: np.exp(-x) - 1e-8, 0.0, 40.0)):
        want, r = brentq(fn, a, b, xtol=eps4, rtol=eps4, full_output=True)
        assert pkg.user_models.brentq(fn, a, b, full_output=True) == (want, r.function_calls, r.iterations)


# ---- CPU: the references -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ALL)
def test_the_scipy_chain_stays_within_K_of_the_exact_solution(cid):
    r = TM.reference(cid)
    print(f"{cid}: chained SciPy lies {r['ratio']:.4f} tolerance units from the exact solution, K = {TM.K[cid]}; "
          f"{int(r['counts'][:, :, 3].sum())} fires, up to {int(r['counts'][:, :, 3].max())} per solve")
    assert r["ratio"] <= TM.K[cid]
    assert 2 * r["ratio"] >= 0.8 * TM.K[cid]      # K is 2 x the measured ratio, not a number chosen wide
    fires = r["counts"][:, :, 3]
    if cid == "T4":
        assert np.all(fires[:, 1] == 0) and np.all(fires[:, 0] >= 1)      # row 1's threshold is never reached
    else:
        assert np.all(fires >= 1) and fires.max() >= 4


def test_t1s_pinned_time_is_the_chains_fire_time_with_the_jump_behind_it():
    r = TM.reference("T1")
    th = TM.population("T1")[0]
    L, D = TM.COND["T1"][0, 1], th[1]
    assert r["first_fire"][0] == TM.TAU["T1"] == TM.times("T1")[0, TM.TAU_AT]
    tol = TM.K["T1"] * (TM.ATOL + TM.RTOL * (L + D))
    assert abs(r["scipy"][0, 0, TM.TAU_AT, 0] - L) <= tol and abs(r["scipy"][0, 0, TM.AFTER_AT, 0] - (L + D)) <= tol


def test_t3_without_jac_is_the_same_chain():
    a, b = TM.reference("T3"), TM.reference("T3N")
    assert np.array_equal(a["counts"][:, :, 3], b["counts"][:, :, 3])
    assert np.nanmax(np.abs(a["scipy"] - b["scipy"]) / (TM.tol("T3")[1] + TM.tol("T3")[0] * np.abs(a["scipy"]))) < 1.0


@pytest.mark.parametrize("cid", ALL)
def test_how_far_the_chain_determines_its_own_digits(cid):
    """The floor under the 1e-9 bar (triggered_model.chain_sensitivity), every sixteenth particle: the chains with a Jacobian, or
    without a Newton solve, are determined far beyond the ninth digit; T3N's, whose Jacobian SciPy forms by differences, is
    not everywhere, and the figure is printed."""
    w = np.array([TM.chain_sensitivity(cid, p) for p in range(1 if cid == "T1" else 0, TM.N, 16)])
    print(f"{cid}: the chain moves by at most {w.max():.3g} (median {np.median(w):.3g}) when y0 moves by 1e-15")
    if cid != "T3N":
        assert w.max() < 1e-11


def test_root_chain_states_its_two_rules(pkg):
    um = pkg.user_models
    rhs, y0, t = (lambda t, y: np.array([-0.6 * y[0]])), np.array([1.0]), np.array([0.0, 1.0, 9.0])
    root = lambda t, y: [y[0] - 0.4]
    with pytest.raises(RuntimeError, match="the start of its own segment"):
        um.root_chain(rhs, y0, t, root, [-1], lambda k, t, y: np.array([0.4]), rtol=TM.RTOL, atol=TM.ATOL)
    with pytest.raises(RuntimeError, match="more than 256 fires"):
        um.root_chain(rhs, y0, t, root, [-1], lambda k, t, y: y + 1e-3, rtol=TM.RTOL, atol=TM.ATOL)
    out = um.root_chain(rhs, y0, t, root, [+1], lambda k, t, y: y + 1.0, rtol=TM.RTOL, atol=TM.ATOL)      # the wrong direction
    assert out["fires"] == [] and abs(out["y"][2, 0] - np.exp(-5.4)) < 1e-6


# ---- CPU: compilation ------------------------------------------------------------------------------------------------------------

def _spec(pkg, cid, source=None):
    c = TM.CASES[cid]
    return pkg.binding.UserSourceSpec(source=(c["source"] if source is None else source).encode(), n_states=c["ns"], dim=c["dim"],
                                      method=int(c["method"] == "BDF"), n_obs=c["n_obs"], n_cond=c["n_cond"], n_ev=c["n_ev"],
                                      n_val=1 if c["n_ev"] else 0)


def _check(pkg, cid, source=None):
    log = ctypes.create_string_buffer(1 << 16)
    rc = pkg.lib().smc_user_model_check_spec(ctypes.byref(_spec(pkg, cid, source)), log, 1 << 16)
    return rc, log.value.decode()


@pytest.mark.parametrize("cid", ALL)
def test_sources_compile_for_gfx950(pkg, cid):
    rc, log = _check(pkg, cid)
    assert rc == 0, log
    rc, log = _check(pkg, cid, TM.PLAIN[cid])
    assert rc == 0, log
    # the names are used: a jump with another signature is no unused device function, it does not compile
    rc, log = _check(pkg, cid, TM.CASES[cid]["source"].replace("smc_user_root_event(int k, double t, double *y,", "smc_user_root_event(int k, double *y,"))
    assert rc == 1 and "smc_user_root_event" in log


def test_the_one_output_source_compiles_with_roots(pkg):
    log = ctypes.create_string_buffer(1 << 16)
    assert pkg.lib().smc_user_model_check2(TM.CASES["T1"]["source"].encode(), 1, 3, 0, log, 1 << 16) == 0, log.value.decode()
    assert pkg.lib().smc_user_model_check2(pkg.user_models.THRESHOLD_REDOSED.encode(), 1, 3, 1, log, 1 << 16) == 0, log.value.decode()


def test_every_refusal_appears_with_its_message(pkg):
    src = TM.CASES["T1"]["source"]
    plain = TM.PLAIN["T1"]
    root = f"__device__ void smc_user_root(double t, const double *y, {_SIG}, double *g) {{ g[0] = y[0] - cond[1]; }}\n"
    event = f"__device__ void smc_user_root_event(int k, double t, double *y, {_SIG}) {{ y[0] += theta[1]; }}\n"
    rc, log = _check(pkg, "T1", plain + root)
    assert rc == 1 and "defines smc_user_root_dir, the direction of every event function" in log and "defines smc_user_root_event, the jump at an event" in log
    rc, log = _check(pkg, "T1", plain + "__device__ const int smc_user_root_dir[] = {-1};\n" + root)
    assert rc == 1 and "defines smc_user_root_event, the jump at an event" in log and "smc_user_root_dir, the direction" not in log
    rc, log = _check(pkg, "T1", plain + root + event)
    assert rc == 1 and "defines smc_user_root_dir, the direction of every event function" in log
    rc, log = _check(pkg, "T1", src.replace("{-1}", "{2}"))
    assert rc == 1 and "smc_user_root_dir: direction 2 is none of -1 (falling), 0 (either), +1 (rising)" in log
    rc, log = _check(pkg, "T1", src.replace("{-1}", "{DOWN}"))
    assert rc == 1 and "smc_user_root_dir: the directions are written as a list of the integers" in log
    # a comment that names the array in front of the definition is passed over: the list behind "smc_user_root_dir[" is read
    rc, log = _check(pkg, "T1", "// smc_user_root_dir; { 7 } says which way each event function fires\n" + src)
    assert rc == 0, log
    five = src.replace("{-1}", "{-1, 0, 1, 0, -1}")
    rc, log = _check(pkg, "T1", five)
    assert rc == 1 and "1 .. 4 event functions (SMC_USER_MAX_ROOTS)" in log
    rc, log = _check(pkg, "T1", src.replace("{-1}", "{-1, 0, +1, 1}").replace("g[0] = y[0] - cond[1];", "g[0] = g[1] = g[2] = g[3] = y[0] - cond[1];"))
    assert rc == 0, log
    assert pkg.binding.SMC_USER_MAX_ROOTS == 4 and pkg.binding.SMC_USER_MAX_ROOT_FIRES == 256 and pkg.lib().smc_abi_version() == 3
    import re
    header = open(pkg.binding.__file__.replace("binding.py", "../include/smc_hip.h")).read()
    assert re.search(r"#define SMC_USER_MAX_ROOTS 4\b", header) and re.search(r"#define SMC_USER_MAX_ROOT_FIRES 256\b", header)


def test_a_source_without_the_names_dumps_the_files_it_has_always_dumped(pkg, tmp_path):
    L = pkg.lib()
    for cid in ("T1", "T3", "T4"):
        a, b = tmp_path / f"plain_{cid}", tmp_path / f"roots_{cid}"
        a.mkdir(), b.mkdir()
        assert L.smc_user_model_dump_source_spec(ctypes.byref(_spec(pkg, cid, TM.PLAIN[cid])), str(a).encode()) == 0
        assert L.smc_user_model_dump_source_spec(ctypes.byref(_spec(pkg, cid)), str(b).encode()) == 0
        plain, roots = sorted(p.name for p in a.iterdir()), sorted(p.name for p in b.iterdir())
        assert "user_root.h" not in plain and roots == sorted(plain + ["user_root.h"])
        for name in plain:
            assert b"SMC_USER_ROOTS" not in (a / name).read_bytes() and b"smc_root" not in (a / name).read_bytes(), name
        head = (b / "smc_user_model.hip").read_text()
        assert "#define SMC_USER_ROOTS 1\n" in head and ("#define SMC_USER_NO_SCHEDULE 1\n" in head) == (cid != "T4")
        assert b"SMC_USER_ROOTS" in (b / "user_item_ops.h").read_bytes()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _engine(pkg, cid, source=None, **over):
    c = TM.CASES[cid]
    t, obs, _ = TM.make_data(cid)
    eng = pkg.HipEngine(over.pop("n", c["n"]), c["dim"], device=0)
    eng.set_prior(TM.priors(cid))
    kw = TM.model_kwargs(cid)
    kw.update(over)
    eng.set_model_user(c["source"] if source is None else source, c["ns"], t, obs, **kw)      # 3-D obs: the rows are ragged
    return eng


def _sweep(pkg, eng, th):
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    return eng.download_lk(pkg.SMC_SET_PRED), info


@pytest.fixture(scope="module")
def run(request, pkg):
    """One engine per case, compiled once; the population's predictions and sweep are shared by the tests of the case."""
    cid = request.param
    c = TM.CASES[cid]
    t, obs, _ = TM.make_data(cid)
    th = TM.population(cid)
    try:
        eng = _engine(pkg, cid)
    except pkg.SmcError as e:
        pytest.exit(f"case {cid}: {e}", returncode=3)
    with eng:
        try:
            lk, info = _sweep(pkg, eng, th)
            out = {"cid": cid, "c": c, "eng": eng, "th": th, "t": t, "obs": obs, "info": info, "lk": lk,
                   "ctr": eng.user_sweep_counters() if c["method"] == "BDF" else None}
            out["lk_p"], out["pred"], out["pinfo"] = eng.predict_user(th)
        except pkg.SmcError as e:      # a device error: no further case is started on a GPU that may have faulted
            pytest.exit(f"case {cid}: {e}", returncode=3)
        yield out


def _cases(ids):
    return pytest.mark.parametrize("run", ids, indirect=True)


def _compared(cid, shape):
    """Everything but T1's pinned pair (see the top)."""
    ok = np.ones(shape, dtype=bool)
    if cid == "T1":
        ok[0, 0, TM.TAU_AT] = ok[0, 0, TM.AFTER_AT] = False
    return ok


@pytest.mark.gpu
@_cases(ALL)
def test_predictions_stay_within_K_of_the_exact_solution_and_1e9_of_the_chain(run):
    cid, c, pred, t = run["cid"], run["c"], run["pred"], run["t"]
    print(f"{cid}: n_failed {run['info']['n_failed']}, rk_attempts {run['info']['rk_attempts']}")
    assert run["info"]["n_failed"] == 0 and run["pinfo"]["n_failed"] == 0
    assert pred.shape == (c["n"], c["n_ex"], TM.N_T, c["n_obs"])
    assert np.array_equal(np.isnan(pred), np.broadcast_to(np.isnan(t)[None, :, :, None], pred.shape))
    ref = TM.reference(cid)
    y, s = ref["exact"], ref["scipy"]
    ok = ~np.isnan(y) & _compared(cid, y.shape)
    ratio = np.max(np.abs(pred - y)[ok] / (TM.K[cid] * (TM.tol(cid)[1] + TM.tol(cid)[0] * np.abs(y)))[ok])
    det = ref["determined"]      # where SciPy's chain determines its own tenth digit (triggered_model.CHAIN_BAR): all but T3N's
    print(f"{cid}: the chain is determined for {int(det.sum())} of {c['n']} particles")
    assert det.all() if cid != "T3N" else det.sum() >= 0.8 * c["n"]
    ok &= det[:, None, None, None]
    dist = np.max(np.abs(pred - s)[ok] / np.maximum(1.0, np.abs(s[ok])))
    print(f"{cid}: worst |pred - y_exact| = {ratio * TM.K[cid]:.4f} tolerance units, K = {TM.K[cid]}; worst |pred - y_scipy| / max(1, |y|) = {dist:.3g}")
    assert ratio <= 1.0
    assert dist < TM.CHAIN_BAR


@pytest.mark.gpu
@_cases(["T4"])
def test_fire_counts_are_the_chains(run):
    """The count output - the model's own counting state - at every data time against the chain's, and its last value against
    the chain's number of fires before the row's last time."""
    pred, ref = run["pred"], TM.reference("T4")
    ok = ~np.isnan(ref["scipy"][..., 1])
    assert np.array_equal(pred[..., 1][ok], ref["scipy"][..., 1][ok])
    last = np.array([[pred[p, e, np.flatnonzero(ok[p, e])[-1], 1] for e in range(3)] for p in range(TM.N)])
    fires = ref["counts"][:, :, 3]
    print(f"T4: fires per row {fires.sum(axis=0)}, device counts at the last time {last.sum(axis=0)}")
    assert np.all((last == fires) | (last == fires - 1))      # a fire exactly at the row's end is seen from before the jump
    assert np.array_equal(last[:, 1], np.zeros(TM.N)) and last[:, 0].min() >= 1


@pytest.mark.gpu
@_cases(["T3", "T3N"])
def test_bdf_work_is_the_chains(run):
    ref, ctr = TM.reference(run["cid"]), run["ctr"]
    steps, nlu, njev = (int(v) for v in ref["counts"][:, :, :3].sum(axis=(0, 1)))
    print(f"{run['cid']}: device / SciPy steps {ctr['steps']} / {steps}, LU {ctr['lu_factorisations']} / {nlu}, Jacobians {ctr['jacobian_evals']} / {njev}")
    assert (ctr["steps"], ctr["lu_factorisations"], ctr["jacobian_evals"]) == (steps, nlu, njev)


@pytest.mark.gpu
@_cases(["T1"])
def test_the_data_time_at_a_fire_time_sees_the_state_before_the_jump(run):
    """The device's own first fire time of particle 0 in row 0, found by bisection over explicit designs (see the top)."""
    eng, th = run["eng"], run["th"]
    L, D = TM.COND["T1"][0, 1], th[0, 1]
    tol = TM.K["T1"] * (TM.ATOL + TM.RTOL * (L + D))
    tau, t_end = TM.TAU["T1"], TM.times("T1")[0, -1]
    lo, hi = tau * (1 - 1e-9), tau * (1 + 1e-9)
    m = 32
    for _ in range(12):
        if np.nextafter(lo, np.inf) == hi:
            break
        mid = np.unique(np.clip(lo + (hi - lo) * np.arange(1, m + 1) / (m + 1), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf)))
        row = np.full(m + 4, np.nan)
        grid = np.concatenate([[0.0, lo], mid, [hi, t_end]])
        row[:grid.size] = grid
        pred, info = eng.predict_user_at(th, t=row[None, :], cond=TM.COND["T1"][:1])
        v = pred[0, 0, 1:grid.size - 1, 0]
        before = np.abs(v - L) <= tol
        after = np.abs(v - (L + D)) <= tol
        assert info["n_failed"] == 0 and np.all(before | after) and before[0] and after[-1], (lo, hi, v)
        assert np.all(before[:-1] >= before[1:])      # before ... before, after ... after
        i = int(np.sum(before))
        lo, hi = grid[i], grid[i + 1]
    assert np.nextafter(lo, np.inf) == hi
    print(f"T1: the device's fire time {lo!r} ({lo.hex()}), the chain's {tau!r} ({tau.hex()}): {abs(lo - tau) / tau:.3g} relative")
    assert abs(lo - tau) <= 1e-9 * tau
    # ... and in the data's own design the pinned pair holds one of the two states each, the later never the earlier one
    pair = run["pred"][0, 0, [TM.TAU_AT, TM.AFTER_AT], 0]
    assert np.all((np.abs(pair - L) <= tol) | (np.abs(pair - (L + D)) <= tol)) and pair[1] >= pair[0] - tol
    assert (abs(pair[0] - L) <= tol) == (tau <= lo) and (abs(pair[1] - L) <= tol) == (np.nextafter(tau, np.inf) <= lo)


@pytest.mark.gpu
@_cases(ALL)
def test_likelihood_is_its_formula_on_the_engines_own_outputs(run):
    cid, c, th = run["cid"], run["c"], run["th"]
    assert np.array_equal(run["lk"], run["lk_p"]) and run["info"]["rk_attempts"] == run["pinfo"]["rk_attempts"]
    assert np.all(np.isfinite(run["lk"]))
    ref = _np_loglik(np.nan_to_num(run["pred"]), run["obs"], run["t"], np.ones(c["n_obs"]), th[:, -1])
    err = np.max(np.abs(run["lk"] - ref) / np.maximum(1.0, np.abs(ref)))
    print(f"{cid}: worst |lk - formula(pred)| / max(1, |lk|) = {err:.3g}; rk_attempts {run['info']['rk_attempts']}")
    assert err <= 1e-9


@pytest.mark.gpu
@_cases(ALL)
def test_metropolis_sweep_is_the_same_with_early_rejection(pkg, run):
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    step = np.diag(2e-3 * np.array([p["high"] for p in TM.priors(cid).values()]) / 3.0)
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


def _hint(cid):
    """A cost hint that puts about one particle in eight on the list (> 220) and one in thirty on the solo list (> 3700)."""
    j = 1 if cid == "T1" else 2
    lo, hi = (1.39, 1.47) if cid == "T1" else (0.94, 0.985)
    return f"__device__ double smc_user_cost(const double *theta) {{ return theta[{j}] > {hi} ? 5000.0 : (theta[{j}] > {lo} ? 300.0 : 0.0); }}\n", j, lo, hi


@pytest.mark.gpu
@_cases(["T1", "T3"])
def test_a_cost_hint_changes_no_bit(pkg, run, tmp_path):
    """With the hint some particles go through the list and the one-per-wave phase (the pool's pack / unpack, the uniform tail's
    broadcast, with fired events); the numbers are those of the run without it."""
    cid, th = run["cid"], run["th"]
    hint, j, lo, hi = _hint(cid)
    assert np.sum(th[:, j] > lo) >= 20 and np.sum(th[:, j] > hi) >= 3
    # the hint's two values against the thresholds the kernel is compiled with (the head of the generated source): should the
    # scheduler's thresholds move, this fails instead of no longer reaching the list and the one-per-wave phase
    import re
    d = tmp_path / "hint"
    d.mkdir()
    assert pkg.lib().smc_user_model_dump_source_spec(ctypes.byref(_spec(pkg, cid, TM.CASES[cid]["source"] + hint)), str(d).encode()) == 0
    head = (d / "smc_user_model.hip").read_text()
    list_cost, solo_cost = (float(re.search(rf"#define SMC_USER_{k}_COST (\S+)", head).group(1)) for k in ("LIST", "SOLO"))
    assert 0 < list_cost < 300.0 < solo_cost < 5000.0
    with _engine(pkg, cid, source=TM.CASES[cid]["source"] + hint) as eng:
        lk, info = _sweep(pkg, eng, th)
        ctr = eng.user_sweep_counters() if run["ctr"] is not None else None
        lk_p, pred, pinfo = eng.predict_user(th)
    assert info["n_failed"] == 0
    assert np.array_equal(lk, run["lk"]) and info["rk_attempts"] == run["info"]["rk_attempts"] and ctr == run["ctr"]
    assert np.array_equal(pred, run["pred"], equal_nan=True) and np.array_equal(lk_p, run["lk_p"])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["T1", "T2", "T3"])
def test_event_functions_that_never_fire_change_no_bit(pkg, cid):
    """The root machinery compiled in with a threshold no state reaches, against the same model without the names."""
    c = TM.CASES[cid]
    never = (f"__device__ const int smc_user_root_dir[] = {{-1, 0}};\n"
             f"__device__ void smc_user_root(double t, const double *y, {_SIG}, double *g) {{ g[0] = y[0] + 1.0e3; g[1] = 2.0 - y[1] * 0.0; }}\n"
             f"__device__ void smc_user_root_event(int k, double t, double *y, {_SIG}) {{ y[0] = 0.0; }}\n")
    if c["ns"] == 1:
        never = never.replace("y[1] * 0.0", "y[0] * 0.0")
    th = TM.population(cid)
    got = []
    for source in (TM.PLAIN[cid] + never, TM.PLAIN[cid]):
        with _engine(pkg, cid, source=source) as eng:
            lk, info = _sweep(pkg, eng, th)
            ctr = eng.user_sweep_counters() if c["method"] == "BDF" else None
            lk_p, pred, pinfo = eng.predict_user(th)
            got.append((lk, info, ctr, lk_p, pred, pinfo))
    (lk0, i0, c0, lp0, p0, pi0), (lk1, i1, c1, lp1, p1, pi1) = got
    assert i0["n_failed"] == 0 and np.all(np.isfinite(lk0))
    assert np.array_equal(lk0, lk1) and i0["rk_attempts"] == i1["rk_attempts"] and c0 == c1
    assert np.array_equal(p0, p1, equal_nan=True) and np.array_equal(lp0, lp1) and pi0["rk_attempts"] == pi1["rk_attempts"]


@pytest.mark.gpu
@_cases(["T1", "T3"])
def test_an_explicit_design(run):
    """predict_user_at on another grid and other thresholds: the functions travel with the compiled kernel, nothing is set.  The
    first 64 particles: within 1e-9 of the chain under that design, and within K of the exact solution where no data time of the
    design lies between a fire's exact and numeric time (nobody drew the population for this design)."""
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    t2, cond2 = TM.design(cid)
    pred, info = eng.predict_user_at(th, t=t2, cond=cond2)
    assert info["n_failed"] == 0 and pred.shape == (c["n"], 2, t2.shape[1], c["n_obs"])
    m = 64
    chain, y = np.full((m,) + pred.shape[1:], np.nan), np.full((m,) + pred.shape[1:], np.nan)
    keep = np.ones(m, dtype=bool)
    for p in range(m):
        for e in range(2):
            seen = ~np.isnan(t2[e])
            r = TM.chain_row(cid, th[p], cond2[e], t2[e])
            chain[p, e, seen] = r["y"]
            y[p, e, seen], fires, _ = TM.exact_row(cid, th[p], cond2[e], t2[e])
            keep[p] &= [int(np.sum(t2[e][seen] < f)) for _, f in r["fires"]] == [int(np.sum(t2[e][seen] < f)) for f in fires]
    assert keep.sum() >= m // 2
    ok = ~np.isnan(y)
    assert np.array_equal(np.isnan(pred[:m]), ~ok)
    ratio = np.max((np.abs(pred[:m] - y) / (TM.K[cid] * (TM.tol(cid)[1] + TM.tol(cid)[0] * np.abs(y))))[keep][ok[keep]])
    dist = np.max(np.abs(pred[:m] - chain)[ok] / np.maximum(1.0, np.abs(chain[ok])))
    print(f"{cid}: an explicit design: {ratio * TM.K[cid]:.4f} tolerance units, K = {TM.K[cid]} ({int(keep.sum())} of {m} particles with no data "
          f"time between a fire's exact and numeric time); worst |pred - y_scipy| / max(1, |y|) = {dist:.3g}")
    assert ratio <= 1.0
    assert dist < TM.CHAIN_BAR
    again = eng.predict_user_at(th)[0]
    assert np.array_equal(again, run["pred"], equal_nan=True)


# ---- GPU: inputs that trip the rules -----------------------------------------------------------------------------------------------

def _tripped(pkg, run, event_body, what):
    """T1 with another jump for the particles with theta[1] > 1.2: their solves fail (info bit 30: n_failed, NaN from the stop on),
    every other item is T1's."""
    th = run["th"]
    bad = th[:, 1] > 1.2
    assert 20 <= bad.sum() <= TM.N - 20
    source = TM.PLAIN["T1"] + TM._ROOTS["T1"].replace("y[0] += theta[1];", event_body)
    assert source != TM.CASES["T1"]["source"]
    with _engine(pkg, "T1", source=source) as eng:
        lk, info = _sweep(pkg, eng, th)
        lk_p, pred, pinfo = eng.predict_user(th)
    print(f"{what}: {int(bad.sum())} particles of {TM.N} trip the rule; n_failed {info['n_failed']} (sweep), {pinfo['n_failed']} (prediction)")
    assert info["n_failed"] == pinfo["n_failed"] == int(bad.sum())      # counted per particle
    finite = ~np.isnan(run["t"])
    for e in range(3):
        assert np.all(np.isnan(pred[bad][:, e, -1 if e < 2 else 7, 0])), (what, e)      # NaN from the stop on
        assert np.all(np.isfinite(pred[bad][:, e, 0, 0]))                               # the outputs before it are there
    assert np.all(np.isfinite(pred[~bad][:, finite]))
    ref = TM.reference("T1")["exact"][~bad]
    assert not bad[0]
    ok = ~np.isnan(ref) & _compared("T1", ref.shape)      # particle 0 leads the particles that do not trip the rule
    assert np.max(np.abs(pred[~bad] - ref)[ok] / (TM.K["T1"] * (TM.ATOL + TM.RTOL * np.abs(ref[ok])))) <= 1.0
    assert np.all(np.isfinite(lk[~bad]))
    return pred[bad]


@pytest.mark.gpu
@_cases(["T1"])
def test_a_jump_that_leaves_the_state_on_the_firing_surface_fails_the_solve(pkg, run):
    """y = L after the jump: g == 0 and falling, the root of the next step is the start of its own segment."""
    pred = _tripped(pkg, run, "y[0] = (theta[1] > 1.2) ? cond[1] : y[0] + theta[1];", "a jump onto the firing surface")
    L = TM.COND["T1"][:, 1]
    seen = ~np.isnan(pred[..., 0])
    assert np.all(pred[..., 0][seen] >= np.broadcast_to(L[None, :, None], seen.shape)[seen] * (1 - 1e-5))      # it stopped at the first fire


@pytest.mark.gpu
@_cases(["T1"])
def test_fire_257_fails_the_solve(pkg, run):
    """A dose of 1e-3: a fire every 1e-3 / (L k) or so, several hundred before the first row ends."""
    _tripped(pkg, run, "y[0] += (theta[1] > 1.2) ? 1.0e-3 : theta[1];", "fire 257")


@pytest.mark.gpu
def test_a_short_run_smc_on_t1_finds_the_planted_dose(pkg):
    n = 1024
    with _engine(pkg, "T1", n=n) as eng:
        out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=TM.priors("T1")), rng="device", seed_device=3, verbose=False)
    assert out["gamma"] == 1.0 and np.isfinite(out["logZ"])
    mean, sd = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
    z = (np.array(TM.THETA_TRUE["T1"]) - mean) / sd
    print(f"T1 run_smc: mean {mean}, sd {sd}, planted {TM.THETA_TRUE['T1']}: {z} posterior standard deviations, logZ {out['logZ']:.3f}")
    assert np.all(np.abs(z) < 3.0)
    assert abs(mean[1] - TM.THETA_TRUE["T1"][1]) < 0.1      # the dose, which no scheduled event could have estimated
