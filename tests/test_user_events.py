"""Scheduled events of a user model (include/smc_hip.h: smc_set_model_user6, smc_user_event; csrc/user_event.h and the
SMC_USER_EVENTS blocks of the kernel files; user_models.event_layout; HipEngine.set_model_user(events=)).  The models, data,
exact solutions, the chained-SciPy reference and the K table live in tests/dosed_model.py.

CPU part: every refusal of the row rules, in NumPy and through smc_user_event_check, in the same words, and a row without events
accepted; the exact solutions against the closed forms; the SciPy chain within the committed K, with the value before the event
at t == tau and the value after it at nextafter(tau); the sources compile for gfx950, the event names without events and
events without smc_user_event are refused with the stated messages; dump_source6 without events writes dump_source5's files.

GPU part: E1 - E4 within K (atol + rtol |y|) of the exact solution; the outputs at tau and nextafter(tau) by name; SciPy
restated; the likelihood as its formula; a Metropolis sweep bit for bit with and without early rejection; events=None against
smc_set_model_user6 with n_ev = 0; the machinery compiled in with every row empty against the model without events; E1 without
its events at or beyond a row's end; a design with events of its own (predict_user_at, the summary); a reset without values
(n_val = 0); a short run_smc on E1.

Measured on an MI355X (tolerance units to the exact solution / K; distance to the SciPy chain; BDF: device / SciPy steps, LU,
Jacobians; the design with events of its own, tolerance units):
    E1  3.08 /  6.168   3.3e-13   design 2.86
    E2  2.95 /  5.898   7.5e-14
    E3  6.05 / 12.101   8.3e-14   91435 / 91435   33318 / 33318   2976 / 2976   design 4.70
    E4 38.70 / 77.408   6.8e-12
The likelihood lies within 1.8e-14 of its formula in every case; early rejection saves 305, 2157, 160 and 94 of 11670, 105956,
93419 and 11252 attempts of the sweep; run_smc on E1 (1024 particles, seed 3) ends with the planted parameters 0.52 and 0.55
posterior standard deviations from the posterior mean, logZ = 30.49."""
import ctypes

import numpy as np
import pytest

import dosed_model as DM
from test_user_model_multiobs import _np_loglik
from test_user_predictive import _check_summary

ALL = list(DM.CASES)
_dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
TAU_AT, AFTER_AT = 2, 3      # row 0: the data time equal to the event time DM.TAU, and the next representable time


# ---- CPU: the row rules ------------------------------------------------------------------------------------------------

def _good(n_ex=2, n_ev=4, n_val=2):
    t = np.tile(np.arange(6, dtype=np.float64), (n_ex, 1))
    return t, np.tile(0.5 + np.arange(n_ev, dtype=np.float64), (n_ex, 1)), np.ones((n_ex, n_ev, n_val))


def _refusals():
    out = []
    t, et, ev = _good(); et[1, 1] = np.nan
    out.append((t, et, ev, "row 1 of ev_t has a NaN event time before a number at event 2"))
    t, et, ev = _good(); et[1, 2] = et[1, 1]
    out.append((t, et, ev, "row 1 of ev_t is not strictly increasing at event 2"))
    t, et, ev = _good(); et[0, 3] = np.inf
    out.append((t, et, ev, "row 0 of ev_t holds an infinite event time at event 3"))
    t, et, ev = _good(); et[1, 0] = t[1, 0]
    out.append((t, et, ev, "row 1 of ev_t is not later than the row's first time t[e][0] at event 0"))
    t, et, ev = _good(); t[0] += 1.0
    out.append((t, et, ev, "row 0 of ev_t is not later than the row's first time t[e][0] at event 0"))
    t, et, ev = _good(); ev[1, 2, 1] = np.nan
    out.append((t, et, ev, "row 1 of ev_v is not finite at event 2, value 1"))
    t, et, ev = _good(); ev[0, 0, 0] = -np.inf
    out.append((t, et, ev, "row 0 of ev_v is not finite at event 0, value 0"))
    t, et, ev = _good(n_ev=257)
    out.append((t, et, ev, "n_ev = 257 above the event capacity 256 (SMC_USER_MAX_EVENTS)"))
    t, et, ev = _good(n_val=9)
    out.append((t, et, ev, "n_val = 9 outside 0 .. 8 (SMC_USER_MAX_EVENT_VALUES)"))
    return out


def _c_check(L, t, et, ev):
    t, et = np.ascontiguousarray(t), np.ascontiguousarray(et)
    ev = None if ev is None or ev.shape[2] == 0 else np.ascontiguousarray(ev)
    return L.smc_user_event_check(_dp(t), _dp(et), _dp(ev), et.shape[0], t.shape[1], et.shape[1], 0 if ev is None else ev.shape[2])


@pytest.mark.parametrize("k", range(len(_refusals())))
def test_a_refused_row_is_refused_in_the_same_words_by_numpy_and_the_library(pkg, k):
    t, et, ev, why = _refusals()[k]
    with pytest.raises(ValueError) as e:
        pkg.user_models.event_layout(t, et, ev)
    assert str(e.value).startswith("event_layout: " + why), str(e.value)
    L = pkg.lib()
    assert _c_check(L, t, et, ev) != 0
    msg = L.smc_last_error(None).decode()
    assert msg.startswith("smc_user_event_check: " + why), msg


def test_accepted_rows_and_a_row_with_no_event(pkg):
    L = pkg.lib()
    t, et, ev = _good()
    et[1, :] = np.nan           # no event at all
    et[0, 3] = np.nan           # a shortened row
    ev[1] = np.nan              # ignored past a row's events
    ev[0, 3] = np.inf
    assert list(pkg.user_models.event_layout(t, et, ev)) == [3, 0]
    assert _c_check(L, t, et, ev) == 0
    assert list(pkg.user_models.event_layout(t, et, None)) == [3, 0] and _c_check(L, t, et, None) == 0      # n_val = 0
    for cid in ALL:
        ev_c = DM.events(cid)
        assert list(pkg.user_models.event_layout(DM.TIMES, ev_c["t"], ev_c["values"])) == [5, 0, 3]
        assert _c_check(L, DM.TIMES, ev_c["t"], ev_c["values"]) == 0
    assert pkg.binding.SMC_USER_MAX_EVENTS == 256 and pkg.binding.SMC_USER_MAX_EVENT_VALUES == 8 and L.smc_abi_version() == 3


# ---- CPU: the references ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ALL)
def test_exact_solution_against_the_closed_forms(cid):
    th = DM.population(cid)[::8]
    for t, cond, ev_t, ev_v in ((DM.TIMES, DM.COND, DM.EV_T, DM.EV_V), DM.design()):
        if cid == "E4" and t is not DM.TIMES:
            continue            # the design is for models without inputs
        a = DM.exact_outputs(cid, th, t, cond, ev_t, ev_v, DM.inputs(cid))
        b = DM.closed_outputs(cid, th, t, cond, ev_t, ev_v, DM.inputs(cid))
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a[0, :, :, 0]), np.isnan(t))
        # two evaluations of the same solution: expm of a system whose rates reach 3e4, and sums of exponentials
        assert np.nanmax(np.abs(a - b) / (1e-12 + np.abs(b))) < 1e-9


def test_events_that_cannot_be_observed_do_not_enter_the_exact_solution():
    ev_t, ev_v = DM.events_inside()
    th = DM.population("E2")[:5]
    assert np.array_equal(DM.exact_outputs("E2", th, DM.TIMES, DM.COND, DM.EV_T, DM.EV_V),
                          DM.exact_outputs("E2", th, DM.TIMES, DM.COND, ev_t, ev_v), equal_nan=True)


@pytest.mark.parametrize("cid", ALL)
def test_the_scipy_chain_stays_within_K_and_sees_the_event_between_tau_and_its_neighbour(cid):
    r = DM.reference(cid)
    print(f"{cid}: chained SciPy lies {r['ratio']:.4f} tolerance units from the exact solution, K = {DM.K[cid]}")
    assert r["ratio"] <= DM.K[cid]
    _check_the_jump(cid, r["scipy"], DM.population(cid), "SciPy chain")


def _check_the_jump(cid, y, th, what):
    """y (n, n_ex, n_t, ns): at t == tau row 0 holds the state before the event, at nextafter(tau) the state after it."""
    exact = DM.reference(cid)["exact"]
    bound = DM.K[cid] * (DM.ATOL + DM.RTOL * np.abs(exact))
    for at in (TAU_AT, AFTER_AT):
        assert np.all(np.abs(y[:, 0, at] - exact[:, 0, at]) <= bound[:, 0, at]), f"{what}: index {at}"
    # the jump itself: what smc_user_event adds, within the tolerance of the two values
    amount = DM.EV_V[0, 0, 0] * (th[:, 2] if cid in ("E2", "E3") else 1.0)
    jump = y[:, 0, AFTER_AT, 0] - y[:, 0, TAU_AT, 0]
    assert np.all(np.abs(jump - amount) <= bound[:, 0, TAU_AT, 0] + bound[:, 0, AFTER_AT, 0]), what
    assert np.all(jump > 0.25)


# ---- CPU: compilation -----------------------------------------------------------------------------------------------------

def _check6(pkg, source, c, n_ev, n_val, n_in=None):
    log = ctypes.create_string_buffer(16384)
    n_in = c["n_in"] if n_in is None else n_in
    rc = pkg.lib().smc_user_model_check6(source.encode(), c["ns"], c["dim"], int(c["method"] == "BDF"), c["n_obs"], 0, c["n_cond"], n_in,
                                         5 if n_in else 0, n_ev, n_val, log, 16384)
    return rc, log.value.decode()


@pytest.mark.parametrize("cid", ALL)
def test_sources_compile_for_gfx950(pkg, cid):
    c = DM.CASES[cid]
    rc, log = _check6(pkg, c["source"], c, c["n_ev"], c["n_val"])
    assert rc == 0, log
    rc, log = _check6(pkg, DM.PLAIN[cid], c, 0, 0)
    assert rc == 0, log


@pytest.mark.parametrize("cid", ["E1", "E3"])
def test_an_event_without_values_compiles(pkg, cid):
    """n_val = 0: a reset needs no number (ev_v is then NULL and smc_event_value is not called)."""
    c = DM.CASES[cid]
    reset = DM.PLAIN[cid] + "__device__ void smc_user_event(int j, double t, double *y, const double *theta, const double *cond) { y[0] = 0.0; }\n"
    rc, log = _check6(pkg, reset, c, 256, 0)
    assert rc == 0, log


def test_event_names_and_event_geometry_must_go_together(pkg):
    c = DM.CASES["E1"]
    rc, log = _check6(pkg, c["source"], c, 0, 0)
    assert rc == 1 and "smc_user_event: this model has no events" in log
    rc, log = _check6(pkg, DM.PLAIN["E1"] + "__device__ double g(const double *c) { return smc_event_value(c, 0, 0); }\n", c, 0, 0)
    assert rc == 1 and "smc_user_event: this model has no events" in log
    rc, log = _check6(pkg, DM.PLAIN["E1"], c, 3, 1)
    assert rc == 1 and "this model has events and its source does not define smc_user_event" in log
    for n_ev, n_val in ((257, 1), (-1, 0), (3, 9), (3, -1)):
        assert _check6(pkg, c["source"], c, n_ev, n_val)[0] == 2


def test_dump_source6_without_events_writes_dump_source5s_files(pkg, tmp_path):
    L = pkg.lib()
    src = pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode()
    for k, (n_in, n_knot) in enumerate(((0, 0), (2, 9))):
        a, b = tmp_path / f"a{k}", tmp_path / f"b{k}"
        a.mkdir(), b.mkdir()
        assert L.smc_user_model_dump_source5(src, 2, 4, 0, 2, 2, 3, n_in, n_knot, str(a).encode()) == 0
        assert L.smc_user_model_dump_source6(src, 2, 4, 0, 2, 2, 3, n_in, n_knot, 0, 0, str(b).encode()) == 0
        names = sorted(p.name for p in a.iterdir())
        assert names == sorted(p.name for p in b.iterdir()) and "user_event.h" not in names
        for name in names:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
            assert b"SMC_USER_EVENTS" not in (a / name).read_bytes(), name
    w = tmp_path / "w"
    w.mkdir()
    c = DM.CASES["E2"]
    assert L.smc_user_model_dump_source6(c["source"].encode(), 2, 4, 0, 2, 0, 1, 0, 0, 5, 2, str(w).encode()) == 0
    assert "user_event.h" in [p.name for p in w.iterdir()]
    head = (w / "smc_user_model.hip").read_text()
    assert "#define SMC_USER_EVENTS 1\n#define SMC_USER_EVAT 1\n#define SMC_USER_NEV 5\n#define SMC_USER_NVAL 2\n" in head


# ---- GPU: E1 - E4 -----------------------------------------------------------------------------------------------------------

def _engine(pkg, cid, source=None, ev=None, **over):
    c = DM.CASES[cid]
    t, obs, _ = DM.make_data(cid)
    eng = pkg.HipEngine(over.pop("n", c["n"]), c["dim"], device=0)
    eng.set_prior(DM.priors(cid))
    kw = DM.model_kwargs(cid, ev)
    kw.update(over)
    eng.set_model_user(c["source"] if source is None else source, c["ns"], t, obs, **kw)
    return eng


def _sweep(pkg, eng, th):
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    return eng.download_lk(pkg.SMC_SET_PRED), info


@pytest.fixture(scope="module")
def run(request, pkg):
    """One engine per case, compiled once; the population's predictions and sweep are shared by the tests of the case."""
    cid = request.param
    c = DM.CASES[cid]
    t, obs, _ = DM.make_data(cid)
    th = DM.population(cid)
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


@pytest.mark.gpu
@_cases(ALL)
def test_predictions_stay_within_K_of_the_exact_solution(run):
    cid, c, pred, t = run["cid"], run["c"], run["pred"], run["t"]
    assert run["info"]["n_failed"] == 0 and run["pinfo"]["n_failed"] == 0
    assert pred.shape == (c["n"], c["n_ex"], DM.N_T, c["n_obs"])
    assert np.array_equal(np.isnan(pred), np.broadcast_to(np.isnan(t)[None, :, :, None], pred.shape))
    y = DM.reference(cid)["exact"]
    bound = DM.K[cid] * (DM.ATOL + DM.RTOL * np.abs(y))
    ok = ~np.isnan(y)
    ratio = np.max(np.abs(pred - y)[ok] / bound[ok])
    print(f"{cid}: worst |pred - y_exact| = {ratio * DM.K[cid]:.4f} tolerance units, K = {DM.K[cid]} ({ratio:.3f} of the bound)")
    assert ratio <= 1.0
    if cid == "E2":      # the population reaches the list and the solo phase
        hint = DM.cost_hint(run["th"])
        assert np.sum(hint > 220.0) >= 20 and np.sum(hint > 3700.0) >= 3


@pytest.mark.gpu
@_cases(ALL)
def test_the_output_at_tau_is_before_the_event_and_its_neighbour_after(run):
    _check_the_jump(run["cid"], run["pred"], run["th"], "device")


@pytest.mark.gpu
@_cases(ALL)
def test_scipy_is_restated(run):
    """RK45: the outputs within 1e-9 max(1, |pred|) of the chained solve_ivp's; BDF: the population's step, LU and Jacobian totals
    within 1 % of the chain's."""
    cid, c, pred = run["cid"], run["c"], run["pred"]
    ref = DM.reference(cid)
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
    step = np.diag(2e-3 * np.array([p["high"] for p in DM.priors(cid).values()]) / 3.0)
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
@_cases(["E1"])
def test_events_at_or_beyond_the_rows_end_change_no_bit(pkg, run):
    ev_t, ev_v = DM.events_inside()
    with _engine(pkg, "E1", ev=DM.events("E1", ev_t, ev_v)) as eng:
        lk, info = _sweep(pkg, eng, run["th"])
        lk_p, pred, pinfo = eng.predict_user(run["th"])
    assert np.array_equal(lk, run["lk"]) and info["rk_attempts"] == run["info"]["rk_attempts"]
    assert np.array_equal(pred, run["pred"], equal_nan=True) and np.array_equal(lk_p, run["lk_p"])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["E2", "E3"])
def test_empty_rows_do_not_perturb_the_integrator(pkg, cid):
    """The event machinery compiled in, every row empty, against the same model without events: RK45 (with a cost hint: lists
    and the solo phase) and BDF."""
    c = DM.CASES[cid]
    th = DM.population(cid)
    none = {"t": np.full((c["n_ex"], 2), np.nan), "values": np.zeros((c["n_ex"], 2, c["n_val"]))}
    got = []
    for source, ev in ((c["source"], none), (DM.PLAIN[cid], None)):
        kw = {} if ev is not None else {"events": None}
        with _engine(pkg, cid, source=source, ev=ev, **kw) as eng:
            lk, info = _sweep(pkg, eng, th)
            ctr = eng.user_sweep_counters() if c["method"] == "BDF" else None
            lk_p, pred, pinfo = eng.predict_user(th)
            got.append((lk, info, ctr, lk_p, pred, pinfo))
    (lk0, i0, c0, lp0, p0, pi0), (lk1, i1, c1, lp1, p1, pi1) = got
    assert i0["n_failed"] == 0 and np.all(np.isfinite(lk0))
    assert np.array_equal(lk0, lk1) and i0["rk_attempts"] == i1["rk_attempts"] and c0 == c1
    assert np.array_equal(p0, p1, equal_nan=True) and np.array_equal(lp0, lp1) and pi0["rk_attempts"] == pi1["rk_attempts"]


@pytest.mark.gpu
def test_no_events_is_the_existing_path_bit_for_bit(pkg):
    """events=None against the same model through smc_set_model_user6 with n_ev = 0 (with inputs: forced_linear_model's F1)."""
    import forced_linear_model as FM
    L = pkg.lib()
    c = FM.CASES["F1"]
    t, obs, cond = (np.ascontiguousarray(a) for a in FM.make_data("F1"))
    inp = FM.make_inputs("F1")
    in_t, in_u = np.ascontiguousarray(inp["t"]), np.ascontiguousarray(inp["u"])
    th = FM.population("F1")
    out = {}
    for how in ("engine", "user6"):
        with pkg.HipEngine(c["n"], c["dim"], device=0) as eng:
            eng.set_prior(FM.priors("F1"))
            eng.set_model_user(c["source"], c["ns"], t, obs, **FM.model_kwargs("F1"))
            if how == "user6":
                rc = L.smc_set_model_user6(eng.ctx, c["source"].encode(), c["ns"], c["n_obs"], _dp(t), _dp(obs), _dp(cond), None, c["n_ex"],
                                           FM.N_T, c["n_cond"], None, None, None, None, c["tol"][0], c["tol"][1], 0, 1, 5.0, _dp(in_t),
                                           _dp(in_u), c["n_in"], c["n_knot"], None, None, 0, 0)
                assert rc == 0, L.smc_last_error(eng.ctx)
                assert L.smc_set_model_user6(eng.ctx, c["source"].encode(), c["ns"], c["n_obs"], _dp(t), _dp(obs), _dp(cond), None, c["n_ex"],
                                             FM.N_T, c["n_cond"], None, None, None, None, c["tol"][0], c["tol"][1], 0, 1, 5.0, _dp(in_t),
                                             _dp(in_u), c["n_in"], c["n_knot"], _dp(in_t), None, 0, 0) != 0      # n_ev = 0 with ev_t
            lk, info = _sweep(pkg, eng, th)
            out[how] = (lk, info["rk_attempts"], eng.predict_user(th)[1])
    assert np.array_equal(out["engine"][0], out["user6"][0]) and out["engine"][1] == out["user6"][1]
    assert np.array_equal(out["engine"][2], out["user6"][2], equal_nan=True) and np.all(np.isfinite(out["engine"][0]))


@pytest.mark.gpu
@_cases(["E1", "E3"])
def test_a_regimen_that_was_never_run(pkg, run):
    """predict_user_at on a longer horizon with events of its own, fewer per row than the model was compiled for: within K of the
    exact solution under THAT regimen; without design events an explicit design is refused; the data's own design needs none."""
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    t2, cond2, ev_t2, ev_v2 = DM.design()
    ev2 = DM.events(cid, ev_t2, ev_v2)
    pred, info = eng.predict_user_at(th, t=t2, cond=cond2, events=ev2)
    assert info["n_failed"] == 0 and pred.shape == (c["n"], 2, t2.shape[1], c["n_obs"])
    y = DM.exact_outputs(cid, th, t2, cond2, ev_t2, ev_v2)
    ok = ~np.isnan(y)
    assert np.array_equal(np.isnan(pred), np.isnan(y))
    ratio = np.max(np.abs(pred - y)[ok] / (DM.K[cid] * (DM.ATOL + DM.RTOL * np.abs(y[ok]))))
    print(f"{cid}: design with its own events: {ratio * DM.K[cid]:.4f} tolerance units, K = {DM.K[cid]}")
    assert ratio <= 1.0
    with pytest.raises(pkg.SmcError, match="the model has events and the design has no matching design events"):
        eng.predict_user_at(th, t=t2, cond=cond2)
    wide = {"t": np.full((2, c["n_ev"] + 1), np.nan), "values": np.zeros((2, c["n_ev"] + 1, c["n_val"]))}
    with pytest.raises(ValueError, match="the model was compiled for 5 events per row"):
        eng.predict_user_at(th, t=t2, cond=cond2, events=wide)
    L = pkg.lib()
    assert L.smc_user_set_design_events(eng.ctx, _dp(wide["t"]), _dp(wide["values"]), 2, c["n_ev"] + 1) != 0
    assert "above the event capacity 5" in L.smc_last_error(eng.ctx).decode()
    again = eng.predict_user_at(th)[0]
    assert np.array_equal(again, run["pred"], equal_nan=True)


@pytest.mark.gpu
@_cases(["E2"])
def test_predictive_summary_with_design_events(pkg, run):
    cid, c, eng, th = run["cid"], run["c"], run["eng"], run["th"]
    t2, cond2, ev_t2, ev_v2 = DM.design()
    ev2 = DM.events(cid, ev_t2, ev_v2)
    probs = (0.0, 0.025, 0.5, 1.0)
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    out = eng.predictive_summary(pkg.SMC_SET_PRED, probs=probs, t=t2, cond=cond2, events=ev2)
    pred, info = eng.predict_user_at(eng.download_particles(pkg.SMC_SET_PRED), t=t2, cond=cond2, events=ev2)
    assert out["n_failed"] == 0 and info["n_failed"] == 0 and out["rk_attempts"] == info["rk_attempts"]
    reached = _check_summary(pkg, out, pred, probs, c["n"])
    assert reached == int(np.sum(~np.isnan(t2))) * c["n_obs"]
    y = DM.exact_outputs(cid, th, t2, cond2, ev_t2, ev_v2)
    ok = ~np.isnan(y)
    assert np.max(np.abs(pred - y)[ok] / (DM.K[cid] * (DM.ATOL + DM.RTOL * np.abs(y[ok])))) <= 1.0
    with pytest.raises(pkg.SmcError, match="the model has events and the design has no matching design events"):
        eng.predictive_summary(pkg.SMC_SET_PRED, probs=probs, t=t2, cond=cond2)


@pytest.mark.gpu
def test_a_reset_without_values_empties_the_compartment(pkg):
    """n_val = 0 (events=..."values": None): y[0] = 0 at row 0's event AT a data time; that time still holds the decaying state,
    every later one exactly 0 (y' = -k y keeps a zero), and the rows without a firing event are E1's without events."""
    c = DM.CASES["E1"]
    t, obs, _ = DM.make_data("E1")
    th = DM.population("E1")[:65]
    reset = DM.PLAIN["E1"] + "__device__ void smc_user_event(int j, double t, double *y, const double *theta, const double *cond) { y[0] = 0.0; }\n"
    ev_t = np.full((3, 2), np.nan)
    ev_t[0, 0] = DM.TAU
    ev_t[2, 0] = 6.0            # row 2's end: never fires
    with pkg.HipEngine(65, c["dim"], device=0) as eng:
        eng.set_prior(DM.priors("E1"))
        eng.set_model_user(reset, 1, t, obs, cond=DM.COND, events={"t": ev_t, "values": None})
        lk, pred, info = eng.predict_user(th)
    assert info["n_failed"] == 0 and np.all(np.isfinite(lk))
    y = DM.COND[None, :, :, None] * np.exp(-th[:, 0, None, None, None] * DM.TIMES[None, :, :, None])      # no event: t0 = 0 in every row
    y[:, 0, AFTER_AT:] = 0.0
    assert np.all(pred[:, 0, AFTER_AT:, 0] == 0.0) and np.all(pred[:, 0, TAU_AT, 0] > 0.05)
    ok = ~np.isnan(y)
    assert np.array_equal(np.isnan(pred), np.isnan(y))
    assert np.max(np.abs(pred - y)[ok] / (DM.K["E1"] * (DM.ATOL + DM.RTOL * np.abs(y[ok])))) <= 1.0


@pytest.mark.gpu
def test_a_short_run_smc_on_e1_finds_the_planted_parameters(pkg):
    n = 1024
    with _engine(pkg, "E1", n=n) as eng:
        out = pkg.run_smc(eng, pkg.SMCSettings(n_particle=n, priors=DM.priors("E1")), rng="device", seed_device=3, verbose=False)
    assert out["gamma"] == 1.0 and np.isfinite(out["logZ"])
    mean, sd = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
    z = (np.array(DM.THETA_TRUE["E1"]) - mean) / sd
    print(f"E1 run_smc: mean {mean}, sd {sd}, planted {DM.THETA_TRUE['E1']}: {z} posterior standard deviations, logZ {out['logZ']:.3f}")
    assert np.all(np.abs(z) < 3.0)
