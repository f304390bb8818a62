"""CPU tests of the oracle's DAE time integration (oracle/meth_dae_oracle.c).  PARITY UNPINNED against the
reference's IDA (absent); what is checked: the integrator core against SciPy's BDF on an ODE, tolerance
refinement, the steady state it reaches, plausibility of my_model's outputs."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def M():
    import __graft_entry__ as g
    g.load_oracle()
    from oracle import methanation
    return methanation


@pytest.fixture(scope="module")
def setup(M):
    cond = M.load_conditions(os.path.join(GOLD, "methanation_information.csv"))
    return cond, M.initial_guess(cond)


def test_bdf_core_against_scipy_on_stiff_ode(M):
    from scipy.integrate import solve_ivp
    k = [0.04, 1e4, 3e7]   # Robertson
    f = lambda t, y: [-k[0] * y[0] + k[1] * y[1] * y[2], k[0] * y[0] - k[1] * y[1] * y[2] - k[2] * y[1] ** 2, k[2] * y[1] ** 2]
    ref = solve_ivp(f, (0, 40), [1, 0, 0], method="BDF", rtol=1e-11, atol=1e-14).y[:, -1]
    y6, rc6, st6 = M.bdf_test_ode([1, 0, 0], k, 40.0, 1e-6, 1e-10)
    y9, rc9, st9 = M.bdf_test_ode([1, 0, 0], k, 40.0, 1e-9, 1e-13)
    assert rc6 == 0 and rc9 == 0
    assert np.max(np.abs(y6 - ref) / np.abs(ref)) < 2e-5
    assert np.max(np.abs(y9 - ref) / np.abs(ref)) < 1e-7
    assert st9["steps"] > st6["steps"] and max(np.nonzero(st6["order_hist"])[0]) >= 3


@pytest.mark.parametrize("i", [0, 7, 19, 29])
def test_tolerance_refinement_and_steady_state(M, setup, i):
    cond, guess = setup
    p = M.p0_tuple(cond, i, M.BASEPARAMS)
    y, rc, st = M.dae_solve(guess[i], p)
    assert rc == 0 and st["newton_fail"] == 0 and 150 < st["steps"] < 1000
    yt, rc2, st2 = M.dae_solve(guess[i], p, rtol=1e-9, atol=1e-9)
    outlet = [50, 101, 152, 203, 254, 305, 356]
    assert rc2 == 0 and np.max(np.abs(yt - y)[outlet] / np.abs(yt[outlet])) < 5e-6
    # t = 75 s is close to the steady state: integrating on to t = 2000 changes the outlet little and the
    # residual with X' = 0 vanishes there
    ys, rc3, _ = M.dae_solve(guess[i], p, tf=2000.0)
    assert rc3 == 0 and np.max(np.abs(ys - y)[outlet] / np.abs(ys[outlet])) < 5e-3
    r = M.reaction(ys, np.zeros(357), p)
    assert np.abs(r[1:50]).max() < 1e-3 * np.abs(M.reaction(guess[i], np.zeros(357), p)).max()


@pytest.mark.parametrize("i", [0, 7, 19, 29])
def test_k8_control_policy_against_the_checker(M, setup, i):
    """Round 5: K8 follows IDA's policy for the iteration matrix and the Newton iteration (csrc/meth_dae_elem.h, dae_integrate_with;
    stated on the CPU by dae_policy {2, 1, 0, 0.33, 0.15}).  Same equations, same tolerances, same step-size control: the outlet
    state stays within a few tolerance units of the checker's default policy (matrix at every attempt, SciPy's Newton test) and of
    a 1e-9 run, with a fraction of the factorisations and fewer than two Newton iterations per attempt."""
    cond, guess = setup
    outlet = [50, 101, 152, 203, 254, 305, 356]
    for pr in (M.BASEPARAMS, M.BASEPARAMS * np.array([3.0, 1.0, 0.3, 1.0, 1, 1, 1, 1])):
        p = M.p0_tuple(cond, i, pr)
        y_chk, rc0, st0 = M.dae_solve_policy(guess[i], p, None)
        y_k8, rc1, st1 = M.dae_solve_policy(guess[i], p, M.k8_policy())
        y_ref, rc2, _ = M.dae_solve_policy(guess[i], p, None, rtol=1e-9, atol=1e-9)
        assert rc0 == rc1 == rc2 == 0
        units = lambda a, b: np.max(np.abs(a - b)[outlet] / (1e-6 + 1e-6 * np.abs(b[outlet])))
        assert units(y_k8, y_chk) < 5.0 and units(y_k8, y_ref) < 5.0 and units(y_chk, y_ref) < 5.0
        assert st0["nlu"] == st0["steps"] + st0["rejects"] + st0["newton_fail"]          # the checker: a matrix per attempt
        assert st1["nlu"] < 0.35 * st1["steps"] and st1["newton_iters"] < 2.0 * (st1["steps"] + st1["rejects"])   # (SciPy's test: >= 2 per attempt)
        assert 0.8 * st0["steps"] < st1["steps"] < 1.25 * st0["steps"]


def test_ida_algorithm_restated_agrees_with_the_bdf_formulation(M, setup):
    """Round 5 cross-check.  K8 and the checker integrate with SciPy's quasi-constant-step formulation of the BDF family under
    IDA's control policy; the reference integrates with IDA itself.  dae_ida_integrate restates IDA's OWN algorithm (divided
    differences phi[j], fixed leading coefficient, its order / step rules, interpolation at the 10 output points) from its published
    description.  Without SUNDIALS it cannot be validated either (parity stays unpinned), but two independent formulations that agree
    at the outlet to a fraction of a tolerance unit bound what the choice of formulation can cost."""
    from scipy.integrate import solve_ivp
    k = [0.04, 1e4, 3e7]   # Robertson, as in the test of the BDF core
    f = lambda t, y: [-k[0] * y[0] + k[1] * y[1] * y[2], k[0] * y[0] - k[1] * y[1] * y[2] - k[2] * y[1] ** 2, k[2] * y[1] ** 2]
    ref = solve_ivp(f, (0, 40), [1, 0, 0], method="BDF", rtol=1e-11, atol=1e-14).y[:, -1]
    y6, rc6, st6 = M.ida_test_ode([1, 0, 0], k, 40.0, 1e-6, 1e-10)
    assert rc6 == 0 and np.max(np.abs(y6 - ref) / np.abs(ref)) < 2e-5 and max(np.nonzero(st6["order_hist"])[0]) >= 3
    cond, guess = setup
    outlet = [50, 101, 152, 203, 254, 305, 356]
    units = lambda a, b: np.max(np.abs(a - b)[outlet] / (1e-6 + 1e-6 * np.abs(b[outlet])))
    for i in (0, 7, 19, 29):
        for pr in (M.BASEPARAMS, M.BASEPARAMS * np.array([3.0, 1.0, 0.3, 1.0, 1, 1, 1, 1])):
            p = M.p0_tuple(cond, i, pr)
            y_ida, rc, st = M.dae_solve_ida(guess[i], p)
            y_k8, rc1, st1 = M.dae_solve_policy(guess[i], p, M.k8_policy())
            y_ref, rc2, _ = M.dae_solve_policy(guess[i], p, None, rtol=1e-9, atol=1e-9)
            assert rc == rc1 == rc2 == 0
            assert units(y_ida, y_k8) < 2.0 and units(y_ida, y_ref) < 2.0
            assert st["nlu"] < 0.2 * st["steps"] and st["newton_iters"] < 2.0 * st["steps"]      # IDA's economy: a matrix per ~12 steps
            assert max(np.nonzero(st["order_hist"])[0]) == 5


def test_my_model_outputs(M, setup):
    cond, guess = setup
    flows, states, stats = M.my_model(M.BASEPARAMS, cond, guess)
    assert flows.shape == (5, 30) and np.all(flows > 0) and np.all(np.isfinite(flows))
    # carbon balance at the outlet: CO2 + CH4 flow equals the CO2 fed (standard-state sccm, +-1 %)
    info = np.loadtxt(os.path.join(GOLD, "methanation_information.csv"), delimiter=",", skiprows=1)[:30]
    assert np.allclose(flows[1] + flows[2], info[:, 11], rtol=2e-2)
    assert np.allclose(flows[4], info[:, 15], rtol=2e-2)          # argon is inert
    assert all(s["status"] == 0 for s in stats)
