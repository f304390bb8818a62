"""GPU tests (-m gpu) of the shared solves of replicate Michaelis-Menten experiments (smc_set_share_replicates): a sweep that
integrates once per pair of replicates must produce, bit for bit, what the sweep that integrates every experiment produces.
Every comparison is switch on against switch off in the same process, with numpy.array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANCELLED, FAILED, ATTEMPTS = 1 << 29, 1 << 30, (1 << 29) - 1


def _condition(name, n_t):
    """(S0, time row) of condition a, b or c; n_t == 1: a row with t0 == t_bound, nothing to integrate."""
    S0, t_end, t0 = {"a": (2.0, 10.0, 0.0), "b": (0.25, 7.0, 0.0), "c": (1.0, 13.0, 0.5)}[name]
    return S0, (np.array([t_end]) if n_t == 1 else np.linspace(t0, t_end, n_t))


def _layout(names, n_t, seed):
    rs = np.random.RandomState(seed)
    t = np.array([_condition(k, n_t)[1] for k in names])
    S0 = np.array([_condition(k, n_t)[0] for k in names])
    P_obs = rs.uniform(0.0, 2.0, size=t.shape)            # replicates differ in their observations only
    return t, P_obs, S0


def _particles(n, seed):
    """Prior-like and posterior-like particles, a stiff one, one with sigma <= 0 (no solve: -inf), the rest in random order."""
    rs = np.random.RandomState(seed)
    th = rs.uniform(0.05, 10.0, size=(n, 3))
    th[::2] = np.array([1.2254, 0.5218, 0.02048]) + rs.standard_normal((len(th[::2]), 3)) * np.array([0.025, 0.0295, 0.00094])
    if n > 3:
        th[3] = (9.0, 0.02, 1.0)                           # Vmax / Km = 450: on the stiff list
    if n > 5:
        th[5, 2] = 0.0
    return th


def _sweep(eng, th, want_pred=True):
    lk, pred, info = eng.loglik_host(th, want_pred=want_pred)
    n = len(th)
    return {"lk": lk, "pred": pred, "rk_attempts": info["rk_attempts"], "n_failed": info["n_failed"],
            "sums": eng.download_item_sums(n), "info": eng.download_item_info(n)}


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


@pytest.mark.parametrize("n_t", [1, 2, 40])
@pytest.mark.parametrize("names", ["aba", "aa", "aaa", "ababccc"])
def test_likelihood_sweep_with_predictions(pkg, names, n_t):
    """Host-batch likelihood sweeps with predictions (the WRITE_PRED kernels) for particle counts around the 64-lane group:
    logL, the (n_ex, n) sums, the info records, the predictions and the attempt count.  n_ex = 2, 3, 7 (NEX up to 8 in the
    accept kernel); 1 and 2 solve groups: the chunk's group of two "experiments" is padded, resp. full; n_t = 1: t0 == t_bound,
    both sums come from the start of the item."""
    t, P_obs, S0 = _layout(names, n_t, seed=len(names) * 100 + n_t)
    n_max = 130
    th_all = _particles(n_max, seed=n_t)
    with pkg.HipEngine(n_max, 3, device=0) as eng:
        eng.set_model_mm(t, P_obs, S0)
        assert eng.share_info()["n_solve"] == {"aba": 2, "aa": 1, "aaa": 2, "ababccc": 4}[names]
        for n in (1, 63, 64, 65, 130):
            th = th_all[:n]
            res = {}
            for on in (True, False):
                eng.set_share_replicates(on)
                res[on] = _sweep(eng, th)
            _assert_same(res[True], res[False], (names, n_t, n))
            assert res[True]["n_failed"] == 0
            finite = np.isfinite(res[True]["lk"])
            assert finite.sum() >= n - 1 and (n_t == 1 or n < 4 or res[True]["rk_attempts"] > 0)
        eng.set_share_replicates(False)
        assert eng.share_info()["n_solve"] == len(names)


@pytest.mark.parametrize("exact", [False, True])
def test_stiff_band(pkg, O, data, exact):
    """300 particles with Vmax / Km between 60 and 5000 on the golden data (experiment 5 replicates experiment 0): the stiff
    list, the solo phase, the uniform tail and - in default mode - the hand-written lone-chain loop all run on shared items.
    Parity mode must also walk the checker's step sequence: equal attempt counts."""
    n = 300
    rs = np.random.RandomState(11)
    th = rs.uniform(0.05, 10.0, size=(n, 3))
    th[:, 1] = th[:, 0] / 10.0 ** rs.uniform(np.log10(60.0), np.log10(5000.0), n)
    res, res_set = {}, {}
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(data.t, data.P_obs, data.S0)
        eng.set_exact_pow(exact)
        assert eng.share_info()["n_solve"] == 5
        for on in (True, False):
            eng.set_share_replicates(on)
            res[on] = _sweep(eng, th)
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            info = eng.loglik(pkg.SMC_SET_PRED)
            res_set[on] = {"lk": eng.download_lk(pkg.SMC_SET_PRED), "rk_attempts": info["rk_attempts"],
                           "sums": eng.download_item_sums(n), "info": eng.download_item_info(n)}
    _assert_same(res[True], res[False], "host batch")
    _assert_same(res_set[True], res_set[False], "particle set")
    assert res[True]["n_failed"] == 0 and np.array_equal(res[True]["lk"], res_set[True]["lk"])
    assert np.array_equal(res[True]["info"][0], res[True]["info"][5])            # the partner's record repeats its primary's
    if exact:
        _, _, oinfo = O.mm_loglik_batch(th, data)
        print(f"parity mode, stiff band: device attempts {res[True]['rk_attempts']}, checker {oinfo['n_attempts']}")
        assert res[True]["rk_attempts"] == oinfo["n_attempts"]


def test_metropolis_sweep_with_early_rejection(pkg, data):
    """One host-RNG Metropolis sweep over a prior-like population of 4096 with early rejection on: accept flags, selected
    particles, their logL and the accept count are equal; a cancelled proposal carries the cancelled mark in both slots of the
    pair.  (Which solves get cancelled, hence rk_attempts, depends on timing - with and without sharing.)"""
    n = 4096
    rs = np.random.RandomState(5)
    th = rs.uniform(0.0, 10.0, size=(n, 3))
    noise = rs.standard_normal((n, 3)) * np.array([0.5, 0.5, 0.5])
    rr = rs.uniform(0, 1, n)
    res = {}
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(data.t, data.P_obs, data.S0)
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_early_reject(True)
        for on in (True, False):
            eng.set_share_replicates(on)
            eng.reset_accept_flags()
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            eng.loglik(pkg.SMC_SET_PRED)
            lk0 = eng.download_lk(pkg.SMC_SET_PRED)
            eng.upload_lk(pkg.SMC_SET_FILT, lk0)
            out = eng.mh_step_host_rng(0.05, 1.0, noise, rr)
            res[on] = {"lk0": lk0, "accepted_now": out["accepted_now"], "n_failed": out["n_failed"],
                       "flags": eng.download_accept_flags(), "filt": eng.download_particles(pkg.SMC_SET_FILT),
                       "lk": eng.download_lk(pkg.SMC_SET_FILT)}
            if on:
                info, sums = eng.download_item_info(n), eng.download_item_sums(n)
    _assert_same(res[True], res[False], "Metropolis sweep")
    assert 0 < res[True]["accepted_now"] < n
    c0, c5 = (info[0] & CANCELLED) != 0, (info[5] & CANCELLED) != 0
    print(f"cancelled solves of the shared pair: {int(c0.sum())} of {n}")
    assert c0.sum() > 0, "the population should hold proposals whose rejection is certain early"
    assert np.array_equal(c0, c5)
    assert np.array_equal(sums[0] == -1.0, c0) and np.array_equal(sums[5] == -1.0, c5)
    assert np.array_equal(info[0] & ATTEMPTS, info[5] & ATTEMPTS)


@pytest.mark.parametrize("mh_batch", ["auto", 0])
def test_complete_run(pkg, data, mh_batch):
    """A complete device-RNG run at N = 20 000 on the golden data: tempering schedule, accept counts, Metropolis loop lengths,
    particles, logL and logZ are bit-identical with sharing on and off."""
    n = 20000
    runs = {}
    for on in (True, False):
        with pkg.HipEngine(n, 3, device=0) as eng:
            eng.set_model_mm(data.t, data.P_obs, data.S0)
            s = pkg.SMCSettings(n_particle=n, share_replicates=on, mh_batch=mh_batch)
            eng.set_prior(s.priors)
            runs[on] = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=41)
    a, b = runs[True], runs[False]
    for key in ("gamma_new", "n_accept", "last_j"):
        assert [r_[key] for r_ in a["records"]] == [r_[key] for r_ in b["records"]], key
    assert np.array_equal(a["p_pred"], b["p_pred"]) and np.array_equal(a["lk"], b["lk"]) and a["logZ"] == b["logZ"]
    assert a["gamma"] == b["gamma"] == 1.0
    assert a["stats"]["rk_attempts_shared"] > 0 and b["stats"]["rk_attempts_shared"] == 0
    assert a["stats"]["rk_attempts_shared"] < a["stats"]["rk_attempts"] / 3        # one experiment of six, the most expensive one


def test_accounting(pkg, data):
    """rk_attempts_shared, counted on the device, is the sum of the attempt records of experiment 5, the golden data's partner."""
    n = 1000
    th = _particles(n, seed=2)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(data.t, data.P_obs, data.S0)
        eng.timing_reset()
        assert eng.share_info() == {"n_solve": 5, "rk_attempts_shared": 0}
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        info = eng.loglik(pkg.SMC_SET_PRED)
        rec = eng.download_item_info(n) & ATTEMPTS
        assert info["rk_attempts"] == int(rec.sum())
        assert eng.share_info()["rk_attempts_shared"] == int(rec[5].sum()) > 0
        eng.loglik(pkg.SMC_SET_PRED)                                   # a running total since timing_reset()
        assert eng.share_info()["rk_attempts_shared"] == 2 * int(rec[5].sum())
        eng.timing_reset()
        eng.set_share_replicates(False)
        eng.loglik(pkg.SMC_SET_PRED)
        assert eng.share_info() == {"n_solve": 6, "rk_attempts_shared": 0}
