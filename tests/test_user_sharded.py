"""A user model over W ranks: the world > 1 branches of run_smc's user-model path (smc_mh_iteration_device_rng: two_pass_factor
with its all-reduces of d and d (d + 1) / 2 words, then one all-reduce of the counts; smc_resample_global with the exchange of
[component][count] blocks of d + 1 rows) with a run-time compiled kernel, d = 8 and a BDF model - on ONE GPU, W rank threads
with the collectives among local peers inside the engines (tests/test_gpu_peer_collectives.py, whose helpers are reused).
Two cases of tests/linear_chain_model.py at n = 768, rng = "device":
    R2  RK45, 3 states, 8 outputs, dim 8, NaN gaps, ragged rows, a noise model;
    B3  BDF, 4 states, 8 outputs, dim 8.
Bars (the project's own for the sharded Michaelis-Menten run): schedule, loop lengths, accept and offspring counts and the ESS
search's iteration counts equal the one-rank run exactly; particles within 1e-9 max(1, |p|), logZ within 1e-9 relative
(cross-rank moment sums round differently from one block's tree: DESIGN.md 5); two runs of the same W bit for bit.

Measured on an MI355X (worst |p - p_one_rank| / max(1, |p|), |logZ - logZ_one_rank| / |logZ_one_rank|):
    R2  W = 2: 2.2e-14, 5.4e-14   W = 3: 3.4e-14, 2.2e-14   (16 tempering steps)
    B3  W = 2: 2.7e-14, 1.5e-14   W = 3: 8.4e-15, 4.7e-15   (17 tempering steps)
    R2  host-driven, W = 2 against its own one-rank run: 8.2e-14, 2.7e-14 (lk: 4.6e-13)
Every count agreed in every case.

A finding of the host-driven rehearsal: at d = 8 its two-rank run left its own one-rank run in tempering step 12 (601 accepted
against 579).  The two cov_m agreed to 1.1e-14, but LAPACK returned rows 1 and 2 of NumPy's SVD factor with the other sign for
one of them, which turns every proposal z @ factor into another one.  driver.run_smc now gives the host-side factor the device
factor's sign convention (driver.fix_row_signs; tests/test_driver_host_logic.py holds it on that pair of matrices).

The predictive summary under ranks: run_smc hands the rank's block start to predictive_summary as global_offset, so the noise
draw is keyed by the GLOBAL particle number; before, every rank drew the noise of particles 0 .. n_local - 1 and the ranks'
bands were correlated copies (test_predictive_bands_under_ranks_use_global_particle_numbers fails without that line).

Mutations, each on a copy of the library or the driver, and the tests that fail:
    peer_reduce_kernel leaves the last rank out from word 5 on          test_sharded_user_model_run_follows_the_one_rank_run, all four
    (the sums of columns 5 .. 7 and most centred sums lack a rank)      cases (the tempering ends after 8 or 10 steps instead of 17 / 16);
                                                                        tests/test_gpu_any_dimension.py passes (it reduces nothing)
    smc_resample_phase3 packs lk into row d - 1 of the send block       the same four cases and the host-driven rehearsal
    run_smc without "global_offset": lo (the parent commit)             test_predictive_bands_under_ranks_use_global_particle_numbers
    run_smc without fix_row_signs                                       test_host_driven_rehearsal_follows_its_own_one_rank_run
"""
import numpy as np
import pytest

import linear_chain_model as LC
from test_gpu_peer_collectives import _run_ranks, _same_counts, _same_run

pytestmark = pytest.mark.gpu

N, SEED = 768, 41
CASES = ("R2", "B3")
WORLDS = {"R2": (2, 3), "B3": (2, 3)}


def _maker(pkg, cid, n_local, n_global):
    c = LC.CASES[cid]
    t, obs, _ = LC.make_data(cid)

    def make(r):
        e = pkg.HipEngine(n_local, c["dim"], device=0, n_global=n_global)
        e.set_prior(LC.priors(cid))
        e.set_model_user(LC.case_source(cid), c["ns"], t, obs, **LC.model_kwargs(cid))
        return e
    return make


def _settings(pkg, cid, n=N):
    return pkg.SMCSettings(n_particle=n, priors=LC.priors(cid))


_RUNS = {}


def _run(pkg, cid, world):
    """The run of case cid over `world` ranks with the collectives inside the engines (world = 1: the plain one-rank run), once
    per module; the results are shared and not to be changed."""
    if (cid, world) not in _RUNS:
        assert LC.CASES[cid]["dim"] == 8 and N % world == 0
        _RUNS[cid, world] = _run_ranks(_maker(pkg, cid, N // world, N), _settings(pkg, cid), world, SEED, pkg.run_smc)
    return _RUNS[cid, world]


def _distance(outs, ref):
    p = np.concatenate([o["p_pred"] for o in outs])
    dp = float((np.abs(p - ref["p_pred"]) / np.maximum(1.0, np.abs(ref["p_pred"]))).max())
    dz = max(abs(o["logZ"] - ref["logZ"]) / abs(ref["logZ"]) for o in outs)
    return dp, dz


@pytest.mark.parametrize("cid,world", [(c, w) for c in CASES for w in WORLDS[c]])
def test_sharded_user_model_run_follows_the_one_rank_run(pkg, cid, world):
    ref = _run(pkg, cid, 1)[0]
    outs = _run(pkg, cid, world)
    assert ref["gamma"] == 1.0 and ref["step"] >= 3 and ref["stats"]["n_failed"] == 0
    assert all(r["n_offspring"] == N for r in ref["records"])
    _same_counts(outs, ref)
    assert all(o["p_pred"].shape == (N // world, 8) for o in outs)
    dp, dz = _distance(outs, ref)
    print(f"{cid}, W = {world}: {ref['step']} steps; worst |p - p_1| / max(1, |p|) = {dp:.3g}, |logZ - logZ_1| / |logZ_1| = {dz:.3g}")
    assert dp < 1e-9 and dz < 1e-9
    for o in outs[1:]:               # every rank logs the same schedule and evidence, bit for bit
        assert o["logZ"] == outs[0]["logZ"]
        assert [r["gamma_new"] for r in o["records"]] == [r["gamma_new"] for r in outs[0]["records"]]


@pytest.mark.parametrize("cid", CASES)
def test_two_sharded_runs_of_the_same_seed_are_bit_identical(pkg, cid):
    """A race in the peer collectives or a stale staging buffer shows here first."""
    world = 2
    again = _run_ranks(_maker(pkg, cid, N // world, N), _settings(pkg, cid), world, SEED, pkg.run_smc)
    _same_run(again, _run(pkg, cid, world))


def test_host_driven_rehearsal_follows_its_own_one_rank_run(pkg):
    """R2 through the *_local calls with Python reductions (ThreadComm) and NumPy's SVD factor: its proposals legitimately
    differ from the fused path's (the device's Jacobi factor, equal to rounding only), so it is compared with its own one-rank
    run, as test_multi_rank_loopback_equals_single_rank does."""
    from _thread_comm import ThreadWorld
    cid, world = "R2", 2

    def one_rank_host(eng, s, comm=None, **kw):
        return pkg.run_smc(eng, s, comm=ThreadWorld(1).comm(0), **kw)
    ref = _run_ranks(_maker(pkg, cid, N, N), _settings(pkg, cid), 1, SEED, one_rank_host)[0]
    outs = _run_ranks(_maker(pkg, cid, N // world, N), _settings(pkg, cid), world, SEED, pkg.run_smc, peer=False)
    assert ref["gamma"] == 1.0
    for o in outs:
        assert o["gamma"] == 1.0 and o["step"] == ref["step"]
        for k in ("gamma_new", "n_accept", "last_j"):
            assert [r[k] for r in o["records"]] == [r[k] for r in ref["records"]], k
        assert all(r["n_offspring"] == N for r in o["records"])
    dp, dz = _distance(outs, ref)
    lk = np.concatenate([o["lk"] for o in outs])
    dl = float((np.abs(lk - ref["lk"]) / np.maximum(1.0, np.abs(ref["lk"]))).max())
    print(f"{cid}, host-driven, W = {world}: worst |p - p_1| / max(1, |p|) = {dp:.3g}, logZ {dz:.3g}, lk {dl:.3g}")
    assert dp < 1e-9 and dz < 1e-9 and dl < 1e-9


def _same_summary(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("mean", "sd", "lower", "upper", "n_finite"))


def test_predictive_bands_under_ranks_use_global_particle_numbers(pkg):
    """run_smc(predictive={"noise": True, ...}) over two ranks: rank r's summary is the summary of its final block with the
    noise keyed by (seed, r n_local + particle, cell) - what a fresh one-rank engine holding that block gives with
    global_offset = r n_local, bit for bit - and not the one keyed from 0.  An explicit global_offset in the dict wins."""
    cid, world = "R2", 2
    nl = N // world
    probs = (0.025, 0.5, 0.975)
    predictive = {"noise": True, "seed": 5, "probs": probs}

    def with_bands(eng, s, **kw):
        return pkg.run_smc(eng, s, predictive=dict(predictive), **kw)
    outs = _run_ranks(_maker(pkg, cid, nl, N), _settings(pkg, cid), world, SEED, with_bands)
    _same_run(outs, _run(pkg, cid, world))                     # the summary changes nothing of the run
    cells = int(np.sum(~np.isnan(LC.make_data(cid)[0]))) * 8
    with _maker(pkg, cid, nl, nl)(0) as eng:
        got = {}
        for r in range(world):
            eng.upload_particles(pkg.SMC_SET_PRED, np.ascontiguousarray(outs[r]["p_pred"]))
            for off in {0, r * nl}:
                got[r, off] = eng.predictive_summary(which=pkg.SMC_SET_PRED, probs=probs, noise=True, seed=5, global_offset=off)
        for r in range(world):
            want = got[r, r * nl]
            assert want["n_failed"] == 0 and int(np.sum(want["n_finite"] == nl)) == cells
            assert _same_summary(outs[r]["predictive"], want), f"rank {r}"
        assert not _same_summary(got[1, nl], got[1, 0])           # the offset matters: other noise, other bands
        assert not np.array_equal(got[1, nl]["mean"], got[1, 0]["mean"], equal_nan=True)
        # an explicit global_offset wins: one rank (block start 0) told to number its particles from nl
        s1 = _settings(pkg, cid, nl)
        base = {"rng": "device", "verbose": False, "seed_device": SEED}
        one = pkg.run_smc(eng, s1, predictive=dict(predictive, global_offset=nl), **base)
        eng.upload_particles(pkg.SMC_SET_PRED, np.ascontiguousarray(one["p_pred"]))
        moved = eng.predictive_summary(which=pkg.SMC_SET_PRED, probs=probs, noise=True, seed=5, global_offset=nl)
        plain = eng.predictive_summary(which=pkg.SMC_SET_PRED, probs=probs, noise=True, seed=5, global_offset=0)
        assert _same_summary(one["predictive"], moved) and not _same_summary(moved, plain)


def test_dump_and_resume_at_eight_parameters(pkg, tmp_path):
    """test_resume_from_dump_is_bit_identical at d = 8 with a user model: the continuation from pred/2_p_pred.csv ends in the
    uninterrupted run's particles, lk, evidence and records, bit for bit; the dumps carry eight columns and the prior's names."""
    cid, n, k = "R2", 257, 2
    s = _settings(pkg, cid, n)
    base = {"rng": "device", "verbose": False, "seed_device": SEED}
    with _maker(pkg, cid, n, n)(0) as eng:
        full = pkg.run_smc(eng, s, dump_dir=str(tmp_path), **base)
    assert full["gamma"] == 1.0 and full["step"] > k + 1
    with _maker(pkg, cid, n, n)(0) as eng:
        cont = pkg.run_smc(eng, s, resume_from=(str(tmp_path), k), **base)
    tail = dict(full, records=full["records"][k:])
    assert len(cont["records"]) == len(tail["records"])
    _same_run([cont], [tail])
    names = list(LC.priors(cid))
    assert names == [f"p{j}" for j in range(8)]
    with open(tmp_path / "Posterior_Distribution.csv") as fh:
        assert fh.readline().strip().split(",") == names
    post = np.loadtxt(tmp_path / "Posterior_Distribution.csv", delimiter=",", skiprows=1, ndmin=2)
    assert post.shape == (n, 8) and np.array_equal(post, full["p_pred"])
    for name in ("first_p_pred", f"{k}_p_pred", "last_p_pred"):
        assert np.loadtxt(tmp_path / "pred" / f"{name}.csv", delimiter=",", ndmin=2).shape == (n, 8)
    assert np.array_equal(np.loadtxt(tmp_path / "pred" / "last_p_pred.csv", delimiter=",", ndmin=2), full["p_pred"])
