"""GPU tests (-m gpu) of the rejection at start of Michaelis-Menten Metropolis sweeps (smc_set_start_reject): an item of a later
pass of the solve queue whose finished siblings already reach the proposal's rejection threshold (tests/test_reject_threshold.py)
is cancelled before its first attempt.  Nothing observable may change: every comparison is switch on against switch off in the
same process, with numpy.array_equal.  Only the attempt counters and the solved / cancelled split depend on the switch (and on
timing)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANCELLED, FAILED, ATTEMPTS = 1 << 29, 1 << 30, (1 << 29) - 1
GAMMA = 0.01


def _population(n, seed=5):
    """Prior-like: uniform over the default prior's box; proposals a good fraction of the box away."""
    rs = np.random.RandomState(seed)
    th = rs.uniform(0.0, 10.0, size=(n, 3))
    noise = rs.standard_normal((n, 3)) * 0.5
    rr = rs.uniform(0, 1, n)
    return th, noise, rr


def _one_sweep(pkg, eng, th, lk0, noise, rr, rng, on):
    """One Metropolis sweep at GAMMA from (th, lk0) with the switch `on`; everything a caller can observe afterwards."""
    n = len(th)
    eng.set_start_reject(on)
    eng.reset_accept_flags()
    eng.upload_particles(pkg.SMC_SET_FILT, th)
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    eng.upload_lk(pkg.SMC_SET_FILT, lk0)
    eng.upload_lk(pkg.SMC_SET_PRED, lk0)
    before = eng.start_reject_info()["solves_not_started"]
    if rng == "host":
        out = eng.mh_step_host_rng(GAMMA, 1.0, noise, rr)
    else:
        out = eng.mh_step_device_rng(GAMMA, 1.0, np.diag([0.5, 0.5, 0.5]), 1234, 7)
    res = {"accepted_now": out["accepted_now"], "accepted_ever": out["accepted_ever"], "n_failed": out["n_failed"],
           "flags": eng.download_accept_flags(), "filt": eng.download_particles(pkg.SMC_SET_FILT),
           "lk": eng.download_lk(pkg.SMC_SET_FILT), "proposals": eng.download_particles(pkg.SMC_SET_PRED)}
    items = {"info": eng.download_item_info(n), "sums": eng.download_item_sums(n),
             "not_started": eng.start_reject_info()["solves_not_started"] - before}
    return res, items


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


def _check_items(items, flags_off, n, n_ex, what):
    """Every item was finished or cancelled exactly once, a particle that holds a cancelled item is one the full computation
    rejects, and the device's count of items that never started is the number of records `0 attempts | cancelled`."""
    info, sums = items["info"], items["sums"]
    cancelled = (info & CANCELLED) != 0
    assert np.array_equal(sums == -1.0, cancelled), what
    completed = (sums >= 0.0) & ~cancelled
    assert int(completed.sum()) + int(cancelled.sum()) == n_ex * n, what          # completed + cancelled == expected
    assert not np.any(flags_off[cancelled.any(axis=0)]), what
    never = info == CANCELLED
    assert items["not_started"] == int(never.sum()), what
    return never


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("rng", ["host", "device"])
@pytest.mark.parametrize("n", [257, 4099, 16384])
def test_ragged_small_populations(pkg, data, n, rng, share):
    """Partial last group of 64, more than one block, and the smallest cost-ordered sweep.  Everything starts at once at these
    sizes, so the look may never fire: shapes, and the off path."""
    th, noise, rr = _population(n)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(data.t, data.P_obs, data.S0)
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_early_reject(True)
        eng.set_share_replicates(share)
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        assert eng.loglik(pkg.SMC_SET_PRED)["n_failed"] == 0
        lk0 = eng.download_lk(pkg.SMC_SET_PRED)
        res, items = {}, {}
        for on in (True, False):
            res[on], items[on] = _one_sweep(pkg, eng, th, lk0, noise, rr, rng, on)
    _assert_same(res[True], res[False], (n, rng, share))
    assert res[True]["n_failed"] == 0 and 0 < res[True]["accepted_now"] < n
    for on in (True, False):
        never = _check_items(items[on], res[False]["flags"], n, len(data.S0), (n, rng, share, on))
        print(f"n={n} rng={rng} share={share} start_reject={on}: {int(never.sum())} items never started")


@pytest.mark.parametrize("rng", ["host", "device"])
def test_look_fires_when_the_first_pass_takes_several_rounds(pkg, data, rng):
    """2^19 particles: a shared sweep has 5 x 2^19 items for a grid of 262 144 lanes, so the first pass of the queue is over long
    before the later ones begin, and the prior-like population holds thousands of proposals whose first experiments alone decide the
    rejection.  How many items never start is timing: printed, not asserted."""
    n = 1 << 19
    th, noise, rr = _population(n)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_model_mm(data.t, data.P_obs, data.S0)
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_early_reject(True)
        assert eng.share_info()["n_solve"] == 5
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        assert eng.loglik(pkg.SMC_SET_PRED)["n_failed"] == 0
        lk0 = eng.download_lk(pkg.SMC_SET_PRED)
        res, items = {}, {}
        for on in (True, False):
            res[on], items[on] = _one_sweep(pkg, eng, th, lk0, noise, rr, rng, on)
    _assert_same(res[True], res[False], rng)
    assert res[True]["n_failed"] == 0 and 0 < res[True]["accepted_now"] < n
    never = {on: _check_items(items[on], res[False]["flags"], n, len(data.S0), (rng, on)) for on in (True, False)}
    att = {on: int((items[on]["info"] & ATTEMPTS).sum()) for on in (True, False)}
    print(f"rng={rng}: items never started: {int(never[True].sum())} with the look, {int(never[False].sum())} without "
          f"(of {n * len(data.S0)}); attempts {att[True]} against {att[False]}")
    assert int(never[True].sum()) > 0
    # the experiments of the first pass (0 and its replicate 5, and 1) never look
    assert int(never[True][[2, 3, 4]].sum()) > int(never[False][[2, 3, 4]].sum())


def test_complete_run(pkg, data):
    """A complete device-RNG run at N = 2^17: tempering schedule, accept counts, Metropolis loop lengths, particles, logL and logZ are
    bit-identical with the switch on and off."""
    n = 1 << 17
    runs = {}
    for on in (True, False):
        with pkg.HipEngine(n, 3, device=0) as eng:
            eng.set_model_mm(data.t, data.P_obs, data.S0)
            s = pkg.SMCSettings(n_particle=n, start_reject=on)
            eng.set_prior(s.priors)
            runs[on] = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=41)
    a, b = runs[True], runs[False]
    for key in ("gamma_new", "n_accept", "last_j"):
        assert [r_[key] for r_ in a["records"]] == [r_[key] for r_ in b["records"]], key
    assert np.array_equal(a["p_pred"], b["p_pred"]) and np.array_equal(a["lk"], b["lk"]) and a["logZ"] == b["logZ"]
    assert a["gamma"] == b["gamma"] == 1.0
    print(f"solves never started: {a['stats']['solves_not_started']} with the look, {b['stats']['solves_not_started']} without; "
          f"attempts {a['stats']['rk_attempts']} against {b['stats']['rk_attempts']}")
    assert a["stats"]["n_failed"] == b["stats"]["n_failed"] == 0
