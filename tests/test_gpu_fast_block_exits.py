"""GPU tests (-m gpu) of every way out of the hand-written lone-chain block (csrc/mm_rk45.h: mm_fast_uniform_attempts): with
the block on (smc_set_fast_tail(1)) a sweep must produce, bit for bit, what the compiled step function produces with it off -
sums of squared residuals, info words (attempt counts), logL -, in all four default-mode solve kernels (with and without
predictions, with and without replicate sharing) and for populations of 1, 64 and 65 particles.

Every particle has Vmax = 1800 Km, so each of its solves is a solo solve: alone in its wave and in the block from its first
attempt (solve_sched.h).  The items and the ways out they take, checked on the CPU with oracle.rk45_solve (SciPy's step
sequence; the device's default-mode controller may differ from it by its fast inverse fifth root, hence the 1e-3 on counts):

  kind   Vmax    S0    attempts  accepted   ways out of the block
  stiff  10      0.1   6319      5445       an output due (40 data times), the budget used up (> 1024 attempts: more than two
                                            refills), a rejection (874) and the first accepted step after it, the clip at
                                            t_bound (the last step, also an output)
  stiff  10      2.0   5         5          outputs due from the second attempt on: every step crosses data times
  stiff  4       0.1   6760      5432       as the first
  tiny   1e-30   any   8         8          error norm < 2^-64 at every attempt: |k_j| <= Vmax, so the error estimate is at
                                            most Vmax * sum|e_j| * (t_bound - t0) / atol = 1.6e-24 < 2^-64 = 5.4e-20
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = np.linspace(0.0, 10.0, 40)
S0 = np.array([0.1, 2.0, 0.1])                       # experiment 2 replicates experiment 0: two solves per particle when shared
KINDS = np.array([[10.0, 10.0 / 1800, 1.0], [1e-30, 1e-30 / 1800, 1.0], [4.0, 4.0 / 1800, 1.0]])
ABS_E = sum(abs(e) for e in (-71 / 57600, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40))
ATTEMPTS = (1 << 29) - 1                             # info word: attempts | cancelled << 29 | failed << 30


@pytest.fixture(scope="module")
def reference(O):
    """(kind, S0) -> stats of the CPU restatement; computed once."""
    ref = {(k, s): O.rk45_solve(KINDS[k, 0], KINDS[k, 1], s, T)[1] for k in range(3) for s in (0.1, 2.0)}
    return ref


def test_parameters_reach_the_ways_out(reference):
    r = reference
    assert (r[0, 0.1]["n_attempts"], r[0, 0.1]["n_accepted"]) == (6319, 5445)
    assert (r[0, 2.0]["n_attempts"], r[0, 2.0]["n_accepted"]) == (5, 5)
    assert (r[2, 0.1]["n_attempts"], r[2, 0.1]["n_accepted"]) == (6760, 5432)
    assert (r[1, 0.1]["n_attempts"], r[1, 0.1]["n_accepted"]) == (8, 8) == (r[1, 2.0]["n_attempts"], r[1, 2.0]["n_accepted"])
    assert all(v["n_out"] == 40 and v["status"] == 0 for v in r.values())
    assert r[0, 0.1]["n_attempts"] > 1024 and r[0, 0.1]["n_attempts"] > r[0, 0.1]["n_accepted"]
    assert KINDS[1, 0] * ABS_E * (T[-1] - T[0]) / 1e-6 < 2.0 ** -64
    assert np.all(KINDS[:, 0] > 1000 * KINDS[:, 1])                     # solo solves


@pytest.mark.parametrize("n", [1, 64, 65])
def test_block_on_and_off_give_the_same_bits(pkg, reference, n):
    rs = np.random.RandomState(n)
    t = np.tile(T, (3, 1))
    P_obs = rs.uniform(0.0, 2.0, size=t.shape)
    kind = np.arange(n) % 3
    th = KINDS[kind]
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(t, P_obs, S0)
        for share in (True, False):
            eng.set_share_replicates(share)
            assert eng.share_info()["n_solve"] == (2 if share else 3)
            for want_pred in (False, True):
                res = {}
                for fast in (True, False):
                    eng.set_fast_tail(fast)
                    lk, pred, info = eng.loglik_host(th, want_pred=want_pred)
                    res[fast] = {"lk": lk, "pred": pred if want_pred else 0, "rk_attempts": info["rk_attempts"],
                                 "n_failed": info["n_failed"], "sum_r2": eng.download_item_sums(n), "info": eng.download_item_info(n)}
                a, b = res[True], res[False]
                for k in a:
                    assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (share, want_pred, k)
                assert a["n_failed"] == 0 and np.all(np.isfinite(a["lk"]))
                att = a["info"] & ATTEMPTS
                for e in range(3):
                    for k in range(min(n, 3)):
                        want = reference[k, float(S0[e])]["n_attempts"]
                        got = att[e, kind == k]
                        assert np.all(got == got[0])
                        print(f"n={n} share={share} pred={want_pred} experiment {e} kind {k}: {got[0]} attempts, CPU {want}")
                        assert abs(int(got[0]) - want) <= int(1e-3 * want), (share, want_pred, e, k, got[0], want)
