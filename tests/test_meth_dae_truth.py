"""K8 (the methanation DAE kernel) and the CPU checker against a METHOD-INDEPENDENT solution of the DAE that the reference's residual
defines: backward Euler on nested grids with Richardson extrapolation, built on the pinned residual alone (tests/meth_dae_truth.py,
fixture tests/golden/meth_dae_truth.npz) - 12 runs sampled at t = 0.5, 5 (the transient) and 75.  The bounds K are measured on the
CPU and committed there; nothing here is fitted to a device result.  What stays unpinned: IDA's own step sequence and its
make_consistent start (no SUNDIALS)."""
import os

import numpy as np
import pytest

import meth_dae_truth as T

TOLS = T.TOLS
S_AREA, P_STP, GAS_R = np.pi * (0.01 / 2) ** 2, 1.013 * 10 ** 5, 8.3144589       # methanation_set_conditon.py:81, 89, 78


@pytest.fixture(scope="module")
def fx():
    return {k: v for k, v in T.load().items()}


@pytest.fixture(scope="module")
def M():
    import __graft_entry__ as g
    g.load_oracle()
    from oracle import methanation
    methanation.lib()
    return methanation


def bar_at(fx):
    return fx["bar"].max(axis=0)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_fixture_meets_its_error_bar_and_holds_what_the_issue_lists(fx):
    assert fx["states"].shape == (12, 3, T.NS) and fx["p0"].shape == (12, 18) and fx["y0"].shape == (12, T.NS)
    assert list(fx["times"]) == list(T.TIMES) and list(fx["experiment"]) == list(T.EXPERIMENTS) * 3
    assert fx["bar"].max() <= T.BAR_MAX and len(fx["grid_steps"]) >= 4 and np.all(np.isfinite(fx["states"]))
    assert os.path.getsize(T.FIXTURE) < 400 * 1024


def test_fixture_against_its_generator(fx, M):
    """Experiment 0, BASEPARAMS, t = 0.5 from scratch with four levels from the same coarsest grid: within the sum of the two bars."""
    cs = T.cases(M)
    assert np.array_equal(np.array([c[2] for c in cs]), fx["p0"]) and np.array_equal(np.array([c[3] for c in cs]), fx["y0"])
    y, bar, table = T.solve_truth(fx["y0"][0], fx["p0"][0], T.N0, 4, times=(0.5,), M=M)
    d = T.units(y[0], fx["states"][0, 0]).max()
    print(f"recomputed against stored: {d:.3g} units; bars {bar.max():.3g} + {fx['bar'][0, 0]:.3g}")
    assert d <= bar.max() + fx["bar"][0, 0]
    assert bar.max() <= T.BAR_MAX


def test_fixture_against_the_dae_without_the_generator(fx, M):
    """Extrapolation preserves linear constraints: the linear algebraic rows of the pinned residual (u[0] - u_in, the seven outlet
    conditions) vanish at every stored state to rounding - each is a difference of two stored values, allowed 4 ulp of them - and the
    inlet node's six differential values (X' = 0 there) are the start values, bit for bit."""
    for c in range(12):
        for it in range(3):
            X = fx["states"][c, it]
            r = M.reaction(X, np.zeros(T.NS), fx["p0"][c])
            assert np.all(np.abs(r[T.LINEAR_ROWS]) <= 4 * np.finfo(float).eps * np.abs(X[T.LINEAR_ROWS])), (c, it)
            assert np.array_equal(X[T.INLET_DIFF], fx["y0"][c][T.INLET_DIFF]), (c, it)


@pytest.fixture(scope="module")
def cpu_runs(fx, M):
    return {kind: T.checker_runs(kind, fx) for kind in ("policy", "default", "ida")}


def test_the_checker_is_pinned_to_the_independent_solution(fx, cpu_runs):
    """dae_solve, dae_solve_policy(k8_policy()) and dae_solve_ida (run to each sample time: it delivers at its last communication point)
    within their measured bounds at 1e-6, the policy run at every tolerance and within 2000 attempts at 1e-8; no run left out."""
    for kind, K in (("policy", T.K_POLICY), ("default", T.K_DEFAULT), ("ida", T.K_IDA)):
        d, att = cpu_runs[kind]
        for it, tf in enumerate(T.TIMES):
            for itol, tol in enumerate(TOLS):
                if tol in K[tf]:
                    print(f"{kind} tf = {tf} tol = {tol:g}: worst {d[:, it, itol].max():.4f} units, K = {K[tf][tol]}")
                    assert np.all(d[:, it, itol] <= K[tf][tol]), (kind, tf, tol, d[:, it, itol])
    assert cpu_runs["policy"][1][:, :, 2].max() <= T.MAX_ATTEMPTS_CPU


def test_the_checker_converges_towards_the_independent_solution(fx, cpu_runs):
    """dae_solve at 1e-8 is below 0.1 of its distance at 1e-6, or below the error bar: the distance measured as everywhere else (the
    worst of the 12 runs, per sample time).  Per run the ratio is 0.004 .. 0.15 (meth_dae_truth's docstring says why one is above 0.1)."""
    d, _ = cpu_runs["default"]
    for it, tf in enumerate(T.TIMES):
        d6, d8 = d[:, it, 0].max(), d[:, it, 2].max()
        print(f"tf = {tf}: {d6:.4f} -> {d8:.4f} units")
        assert d8 < 0.1 * d6 or d8 < bar_at(fx)[it]


def test_the_bar_has_teeth(fx):
    """Planted errors the bound must see, every run: a kinetic parameter off by 1e-4 (the activation energy p0[11] at all three times;
    the rate constant p0[10] at t = 5 and 75, and at t = 0.5 from K[0.5][1e-7] on - at 1e-6 its 7 .. 10 units in the third vector's runs
    are what K[0.5][1e-6] = 6.9 allows, so there the 1e-6 bar cannot tell it from integration error), a final time off by 1e-3 in
    the transient (t = 0.5 and 5; at t = 75 the reactor stands still and no test of the final state can see it)."""
    for kind in ("default", "policy"):
        d, _ = T.checker_runs(kind, fx, tols=(1e-6,), scale_p=T.planted_p(11))
        for it, tf in enumerate(T.TIMES):
            assert np.all(d[:, it, 0] > T.K[tf][1e-6]), (kind, tf, d[:, it, 0])
        d, _ = T.checker_runs(kind, fx, tols=(1e-6,), scale_p=T.planted_p(10))
        assert np.all(d[:, 0, 0] > T.K[0.5][1e-7]) and np.all(d[:, 1, 0] > T.K[5.0][1e-6]) and np.all(d[:, 2, 0] > T.K[75.0][1e-6])
        d, _ = T.checker_runs(kind, fx, tols=(1e-6,), times=(0.5, 5.0), scale_tf=1 + 1e-3)
        assert np.all(d[:, 0, 0] > T.K[0.5][1e-6]) and np.all(d[:, 1, 0] > T.K[5.0][1e-6]), (kind, d[:, :, 0])


# ---- GPU: 9 launches of 12 solves (and one of 13), shared by the tests ------------------------------------------------------------------
def outlet_mapping(y, p0):
    """my_model's outlet mapping (methanation_set_likelihood.py:204-208) in NumPy, operation by operation in the reference's order."""
    y, p0 = np.atleast_2d(y), np.atleast_2d(p0)
    u, Tt = y[:, 356], y[:, 305]
    P_total = (p0[:, 0] + p0[:, 1] + p0[:, 2] + p0[:, 3] + p0[:, 4]) * GAS_R * p0[:, 5]
    return np.stack([y[:, 50 + 51 * f] * S_AREA * u * 60 * GAS_R * Tt / P_total * 1e6 * P_total / P_STP * 298 / Tt for f in range(5)], axis=1)


@pytest.fixture(scope="module")
def k8_runs(pkg, fx):
    out = {}
    for tf in T.TIMES:
        for tol in TOLS:
            out[tf, tol] = pkg.methanation.dae_solve_batch(fx["p0"], fx["y0"], tf=tf, rtol=tol, atol=tol, want_states=True)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("tf", T.TIMES)
def test_k8_status(k8_runs, tf, tol):
    flows, status, states, info = k8_runs[tf, tol]
    assert np.all(status == 0), status


@pytest.mark.gpu
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("tf", T.TIMES)
def test_k8_states_within_K_of_the_independent_solution(k8_runs, fx, tf, tol):
    """All 357 states, differential and algebraic, of all 12 solves."""
    flows, status, states, info = k8_runs[tf, tol]
    it = T.TIMES.index(tf)
    d = T.units(states, fx["states"][:, it]).max(axis=1)
    print(f"K8 tf = {tf} tol = {tol:g}: worst {d.max():.4f} units (run {d.argmax()}), K = {T.K[tf][tol]}, ratio {d.max() / T.K[tf][tol]:.3f}")
    assert np.all(d <= T.K[tf][tol]), d


@pytest.mark.gpu
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("tf", T.TIMES)
def test_k8_flows_are_the_outlet_mapping_of_its_own_state(k8_runs, fx, tf, tol):
    """The kernel and NumPy evaluate the same product in the same order with correctly rounded IEEE operations (nothing to contract in
    a chain of products and quotients), so no difference is expected; allowed is one rounding, 2^-53 relative, for each of the mapping's
    nine multiplications and divisions (its /P_total*P_total and *T/T cancel)."""
    flows, status, states, info = k8_runs[tf, tol]
    ref = outlet_mapping(states, fx["p0"])
    rel = np.abs(flows - ref) / np.abs(ref)
    print(f"flows against the mapping of the kernel's own outlet state: worst {rel.max():.3g} relative")
    assert np.all(np.abs(flows - ref) <= 9 * 2.0 ** -53 * np.abs(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("tf", T.TIMES)
def test_k8_flows_against_the_mapping_of_the_independent_solution(k8_runs, fx, tf, tol):
    """F = g C u (T cancels): with |dC| <= K (1e-6 + 1e-6 |C|) and |du| <= K (1e-6 + 1e-6 |u|), |dF| <= g (|u| dC + |C| du + dC du) - the
    two relative bounds add - plus the mapping's rounding."""
    flows, status, states, info = k8_runs[tf, tol]
    X = fx["states"][:, T.TIMES.index(tf)]
    ref = outlet_mapping(X, fx["p0"])
    C, u = np.abs(X[:, [50, 101, 152, 203, 254]]), np.abs(X[:, [356]])
    g = S_AREA * 60 * GAS_R * 1e6 / P_STP * 298
    k = T.K[tf][tol]
    dC, du = k * (1e-6 + 1e-6 * C), k * (1e-6 + 1e-6 * u)
    allowed = g * (u * dC + C * du + dC * du) * (1 + 1e-12) + 18 * 2.0 ** -53 * np.abs(ref)
    ratio = np.abs(flows - ref) / allowed
    print(f"flows tf = {tf} tol = {tol:g}: worst {ratio.max():.3f} of the propagated bound")
    assert np.all(np.abs(flows - ref) <= allowed)


@pytest.mark.gpu
def test_k8_failure_sentinel_leaves_its_neighbours_alone(pkg, k8_runs, fx):
    """A solve with a NaN kinetic parameter in the middle of the batch: status != 0 and the -10000 flows for it, the 12 good solves
    bit for bit what the batch without it returned."""
    at = 5
    p0 = np.insert(fx["p0"], at, fx["p0"][at], axis=0)
    y0 = np.insert(fx["y0"], at, fx["y0"][at], axis=0)
    p0[at, 10] = np.nan
    flows, status, states, info = pkg.methanation.dae_solve_batch(p0, y0, tf=0.5, rtol=1e-6, atol=1e-6, want_states=True)
    assert status[at] != 0 and np.all(flows[at] == -10000.0)
    good = np.arange(13) != at
    f0, s0, y0_, _ = k8_runs[0.5, 1e-6]
    assert np.array_equal(status[good], s0) and np.array_equal(flows[good], f0) and np.array_equal(states[good], y0_)
