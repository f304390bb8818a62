"""The fused forms of the batch path against the stage-by-stage ones (GPU).

On one rank the accept kernel's last block takes the loop's decision and forms the next proposal factor (no launch of
mh_control_kernel between two iterations), the scatter kernel of a cost-ordered sweep derives its own offsets, and a batch
ends with one copy to the host.  None of that may move a result:

  * whole runs with the Metropolis loop on the host (mh_batch = 0: one smc_mh_iteration_device_rng per iteration, row
    reduction in moments_reduce_kernel, factor in mh_transform_kernel), in fixed batches of 3 and in "auto" batches are
    compared BIT FOR BIT - integer counts are order-independent and every floating-point sum keeps its order, so there is
    no tolerance to choose;
  * the moments a batch carries are checked against np.cov of the population they describe, with the tolerance
    test_fused_mh_iterations_carry_their_moments uses (1e-11 of the largest entry: summation order of ~5e4 float64 terms).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make_engine(pkg, data, n):
    eng = pkg.HipEngine(n, 3, device=0)
    eng.set_model_mm(data.t, data.P_obs, data.S0)
    eng.set_prior(pkg.SMCSettings().priors)
    return eng


def run(pkg, data, n, mh_batch):
    s = pkg.SMCSettings(n_particle=n, mh_batch=mh_batch)
    with make_engine(pkg, data, n) as eng:
        out = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=4242)
    rec = out["records"]
    return {"p_pred": np.array(out["p_pred"], copy=True), "lk": np.array(out["lk"], copy=True), "logZ": np.array([out["logZ"]]),
            "gamma": np.array([r["gamma_new"] for r in rec]), "n_accept": np.array([r["n_accept"] for r in rec]),
            "last_j": np.array([r["last_j"] for r in rec]),
            "cov_m": np.array([m["cov_m"] for r in rec for m in r["mh"]]),
            "accepted_now": np.array([m["accepted_now"] for r in rec for m in r["mh"]]),
            "mhstep_ratio": np.array([m["mhstep_ratio"] for r in rec for m in r["mh"]])}


@pytest.mark.parametrize("n", [16384, 300000])
def test_whole_run_is_bit_identical_for_every_batching(pkg, data, n):
    ref = run(pkg, data, n, 0)
    assert ref["gamma"][-1] == 1.0 and len(ref["cov_m"]) > len(ref["gamma"])
    for mh_batch in (3, "auto"):
        got = run(pkg, data, n, mh_batch)
        for k, v in ref.items():
            assert got[k].shape == v.shape and np.array_equal(got[k], v), (n, mh_batch, k)


def test_batch_carries_its_moments(pkg, data):
    """cov_m of every iteration of a batch - formed by the accept kernel's last block from the moments that kernel has just
    accumulated - is np.cov(p_filt.T, bias=True) * w_cov of the population the iteration starts from, and so is the cov_m of
    a stage-by-stage iteration that follows the batch (it starts from the moments the batch left)."""
    n = 50000
    s = pkg.SMCSettings(n_particle=n)
    w_cov = s.w_cov()
    rs = np.random.RandomState(21)
    th = np.array([1.2254, 0.5218, 0.02048]) + rs.standard_normal((n, 3)) * np.array([0.025, 0.0295, 0.00094])

    def start(eng):
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        eng.loglik(pkg.SMC_SET_PRED)
        eng.upload_particles(pkg.SMC_SET_FILT, th)
        eng.upload_lk(pkg.SMC_SET_FILT, eng.download_lk(pkg.SMC_SET_PRED))
        eng.reset_accept_flags()

    def close(cov, pop):
        ref = np.cov(pop.T, bias=True) * w_cov
        return np.abs(cov - ref).max() <= 1e-11 * np.abs(ref).max()

    never = 2.0 * n          # accepted_ever cannot exceed n: the loop does not break, and nothing is halved below 0
    pops = [th]
    for k in (1, 2, 3):      # the population after k iterations: a batch of k on a fresh engine (same seeds, deterministic)
        with make_engine(pkg, data, n) as eng:
            start(eng)
            out = eng.mh_sweeps_device_rng(1.0, 1.0, w_cov, 5, 9 << 16, k, never, 0.0)
            assert out["n_done"] == k and not out["stopped"]
            pops.append(eng.download_particles(pkg.SMC_SET_FILT))
            if k == 3:
                for i, it in enumerate(out["iterations"]):
                    assert close(it["cov_m"], pops[i]), i
                    assert it["accepted_now"] == np.any(pops[i + 1] != pops[i], axis=1).sum() > 0.2 * n
                nxt = eng.mh_iteration_device_rng(1.0, 1.0, w_cov, 5, (9 << 16) | 3, 0)
                assert close(nxt["cov_m"], pops[3])
