"""The two forms of the per-lane step attempt of the Michaelis-Menten solve kernels (csrc/mm_rk45.h: mm_item_attempt_lane, the
form with the fewest vector instructions, and mm_item_attempt, selected by SMC_BULK_ATTEMPT=0 when the context is created)
must give the same bits: sums of squared residuals, info words (attempt counts, failed bit), logL and predictions, in the four
default-mode solve kernels (replicate sharing on and off, predictions on and off), with the lone-chain block on and off, for
populations of 64 (one full wave: the bulk loop runs while at least 41 lanes are live), 65 (a second block of one item) and
130 particles (two blocks and a remainder).

Every particle is non-stiff (Vmax <= 60 Km: off the stiff list), so every attempt is a per-lane one - in the bulk loop, and,
once the queue is empty and 2..40 lanes are live, in the lane tail (solve_sched.h).  Kinds alternate by lane % 8, so that
neighbouring lanes diverge; per wave eight long solves (kind 0) sit among 56 shorter ones and are what the lane tail runs.
Checked on the CPU with oracle.rk45_solve (SciPy's step sequence), S0 = 0.1 / 2.0:

  kind  Vmax    Km     attempts   accepted   what it reaches
  0     2.9     0.05   209 / 187  182 / 173  long, with rejections: the first accepted step after one clamps at factor 1; more
                                             steps than data times: a step crosses one data time or none; lane tail
  1     1.0     0.05   72 / 71    68 / 59    the same, a third as long
  2     0.05    1.0    3 / 3      3 / 3      three steps serve 40 data times: a step that crosses many; factor clamped at 10
  3     1e-30   1.0    8 / 8      8 / 8      error norm < 2^-64 in every attempt (bound below): the window's way out
  4     0       1.0    8 / 8      8 / 8      error norm 0, the power is inf, the factor 10
  5     1e308   1e307  40 / 1     39 / 0     S0 = 2: Vmax * S overflows, f and the error norm are not finite, the IEEE re-run
                                             follows and is not finite either, the rejection's factor is 0.2 (the power is NaN),
                                             h_abs < min_step: failed, NaN sum.  S0 = 0.1: finite, an ordinary solve
  6     0.2     1.0    5 / 3      4 / 3      one rejection in five attempts
  7     1e-3    1.0    3 / 3      3 / 3      as kind 2
Every solve's last step is clipped at t_bound."""
import numpy as np
import pytest

T = np.linspace(0.0, 10.0, 40)
S0 = np.array([0.1, 2.0, 0.1])                       # experiment 2 replicates experiment 0: two solves per particle when shared
KINDS = np.array([[2.9, 0.05, 1.0], [1.0, 0.05, 1.0], [0.05, 1.0, 1.0], [1e-30, 1.0, 1.0], [0.0, 1.0, 1.0], [1e308, 1e307, 1.0],
                  [0.2, 1.0, 1.0], [1e-3, 1.0, 1.0]])
ABS_E = sum(abs(e) for e in (-71 / 57600, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40))
ATTEMPTS = (1 << 29) - 1                             # info word: attempts | cancelled << 29 | failed << 30
FAILED = 1 << 30


@pytest.fixture(scope="module")
def reference(O):
    """(kind, S0) -> stats of the CPU restatement; computed once."""
    with np.errstate(all="ignore"):
        return {(k, s): O.rk45_solve(KINDS[k, 0], KINDS[k, 1], s, T)[1] for k in range(len(KINDS)) for s in (0.1, 2.0)}


def test_parameters_reach_the_paths(reference):
    r = reference
    assert np.all(KINDS[:, 0] <= 60.0 * KINDS[:, 1])                    # off the stiff list: per-lane attempts only
    for s in (0.1, 2.0):
        for k in (0, 1):                                                # rejections, and fewer than one data time per step
            assert r[k, s]["n_attempts"] > r[k, s]["n_accepted"] > 40
        for k in (2, 7):                                                # many data times per step, no rejection
            assert r[k, s]["n_attempts"] == r[k, s]["n_accepted"] == 3
        for k in (3, 4):
            assert r[k, s]["n_attempts"] == r[k, s]["n_accepted"] == 8
    assert r[0, 0.1]["n_attempts"] > 2 * r[1, 0.1]["n_attempts"] and r[1, 0.1]["n_attempts"] > 5 * r[5, 0.1]["n_attempts"] / 4   # the lane tail's solves
    assert r[6, 0.1]["n_attempts"] == r[6, 0.1]["n_accepted"] + 1
    # |k_j| <= Vmax, so the error estimate is at most Vmax * sum|e_j| * (t_bound - t0), over a scale of at least atol
    assert KINDS[3, 0] * ABS_E * (T[-1] - T[0]) / 1e-6 < 2.0 ** -64
    assert KINDS[5, 0] > np.finfo(np.float64).max / S0[1]                # Vmax * S0 overflows
    assert r[5, 2.0]["status"] == -1 and r[5, 2.0]["n_accepted"] == 0 and r[5, 2.0]["n_out"] == 0
    assert all(v["n_out"] == 40 and v["status"] == 0 for key, v in r.items() if key != (5, 2.0))


def _sweeps(pkg, n, th, P_obs):
    """every kernel and both settings of the lone-chain block, on a fresh engine"""
    out = {}
    t = np.tile(T, (3, 1))
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(t, P_obs, S0)
        for share in (True, False):
            eng.set_share_replicates(share)
            assert eng.share_info()["n_solve"] == (2 if share else 3)
            for want_pred in (False, True):
                for fast in (True, False):
                    eng.set_fast_tail(fast)
                    lk, pred, info = eng.loglik_host(th, want_pred=want_pred)
                    out[share, want_pred, fast] = {"lk": lk, "pred": pred if want_pred else 0, "rk_attempts": info["rk_attempts"],
                                                   "n_failed": info["n_failed"], "sum_r2": eng.download_item_sums(n),
                                                   "info": eng.download_item_info(n)}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 130])
def test_both_forms_give_the_same_bits(pkg, reference, monkeypatch, n):
    rs = np.random.RandomState(n)
    P_obs = rs.uniform(0.0, 2.0, size=(3, len(T)))
    kind = np.arange(n) % len(KINDS)
    th = KINDS[kind]
    monkeypatch.delenv("SMC_BULK_ATTEMPT", raising=False)
    new = _sweeps(pkg, n, th, P_obs)
    monkeypatch.setenv("SMC_BULK_ATTEMPT", "0")          # read when the context is created
    old = _sweeps(pkg, n, th, P_obs)
    monkeypatch.delenv("SMC_BULK_ATTEMPT")
    for key in new:
        a, b = new[key], old[key]
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (key, k)
        # the paths were taken: the failing kind fails on the S0 = 2 experiment alone, everything else finishes
        fails = (a["info"] & FAILED) != 0
        want_fail = np.zeros((3, n), dtype=bool)
        want_fail[1, kind == 5] = True
        assert np.array_equal(fails, want_fail), key
        assert np.all(np.isnan(a["sum_r2"][want_fail])) and np.all(np.isfinite(a["sum_r2"][~want_fail]))
        assert a["n_failed"] == int(np.sum(kind == 5))
        att = a["info"] & ATTEMPTS
        for e in range(3):
            for k in range(len(KINDS)):
                got = att[e, kind == k]
                assert np.all(got == got[0])
                want = reference[k, float(S0[e])]["n_attempts"]
                if key == (True, False, True):
                    print(f"n={n} experiment {e} kind {k}: {got[0]} attempts, CPU {want}")
                if (k, e) != (5, 1):      # the device's fast inverse fifth root may move an accept / reject decision of a long solve
                    assert abs(int(got[0]) - want) <= max(1, int(0.02 * want)), (key, e, k, got[0], want)
