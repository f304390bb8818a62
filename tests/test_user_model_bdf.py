"""User models under method="BDF" (include/smc_hip.h: SMC_USER_METHOD_BDF): the run-time compiled restatement of SciPy's
bdf.py for stiff models.  CPU part: the sources compile for gfx950, the ABI's new entry points keep the RK45 path as it
was, and the kernel is under the control-flow and scratch checks of the other kernels.  GPU part: Robertson's kinetics
(with and without smc_user_jac) and an eight-state chain against SciPy's BDF, failure, early rejection and a full run.

Every tolerance is fixed in advance: the per-output bound delta = k (atol + rtol |y|) with k from
tests/robertson_bdf_bound.py (SciPy BDF against Radau at rtol 1e-10 on this population, worst ratio doubled)."""
import ctypes
import multiprocessing
import os
import re
import shutil
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import robertson_bdf_bound as RB
from test_k8_uniform_control import _innermost_loop
from test_user_model import CHAIN8, DIVERGING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
OPT = "/opt/rocm/lib/llvm/bin/opt"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=on", "-fno-fast-math"]   # csrc/Makefile
BDF = 1


def _check(pkg, src, ns, dim, method=BDF):
    log = ctypes.create_string_buffer(16384)
    rc = pkg.lib().smc_user_model_check2(src.encode(), ns, dim, method, log, 16384)
    return rc, log.value.decode(errors="replace")


def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_bdf_sources_compile_for_gfx950(pkg):
    assert pkg.binding.SMC_USER_METHOD_BDF == BDF and pkg.binding.SMC_USER_METHOD_RK45 == 0
    for src, ns in ((pkg.user_models.ROBERTSON, 3), (pkg.user_models.ROBERTSON_NUMJAC, 3), (CHAIN8, 8),
                    (pkg.user_models.MICHAELIS_MENTEN, 1)):
        rc, log = _check(pkg, src, ns, 3)
        assert rc == 0, log
    assert "smc_user_jac" in pkg.user_models.ROBERTSON and "smc_user_jac" not in pkg.user_models.ROBERTSON_NUMJAC


def test_a_named_but_undefined_jacobian_fails_with_the_compiler_log(pkg):
    rc, log = _check(pkg, pkg.user_models.ROBERTSON_NUMJAC + "// smc_user_jac: later\n", 3, 3)
    assert rc == 1 and "smc_user_jac" in log


def test_unknown_method_and_too_many_states_are_refused(pkg):
    assert _check(pkg, pkg.user_models.ROBERTSON, 3, 3, method=2)[0] == 2
    assert _check(pkg, pkg.user_models.ROBERTSON, 9, 3)[0] == 2
    assert pkg.lib().smc_user_model_dump_source2(pkg.user_models.ROBERTSON.encode(), 3, 3, 2, b"/nonexistent") == 2


def test_rk45_dump_is_unchanged_by_the_method_argument(pkg, tmp_path):
    for src, ns in ((pkg.user_models.MICHAELIS_MENTEN, 1), (pkg.user_models.CONSECUTIVE_REACTIONS, 2), (CHAIN8, 8)):
        a, b = tmp_path / f"a{ns}", tmp_path / f"b{ns}"
        a.mkdir()
        b.mkdir()
        assert pkg.lib().smc_user_model_dump_source(src.encode(), ns, 3, str(a).encode()) == 0
        assert pkg.lib().smc_user_model_dump_source2(src.encode(), ns, 3, 0, str(b).encode()) == 0
        assert sorted(os.listdir(a)) == sorted(os.listdir(b))
        for f in os.listdir(a):
            assert (a / f).read_bytes() == (b / f).read_bytes(), f


def _bdf_dump(pkg, tmp_path, src, ns):
    d = str(tmp_path)
    assert pkg.lib().smc_user_model_dump_source2(src.encode(), ns, 3, BDF, d.encode()) == 0
    assert sorted(os.listdir(d)) == ["philox.h", "reject_bound.h", "rk45_math.h", "smc_user_model.hip", "solve_sched.h", "sweep_args.h",
                                     "user_item_ops.h"]
    return d


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(OPT)), reason="needs hipcc and LLVM opt from ROCm")
@pytest.mark.parametrize("model", ["ROBERTSON", "ROBERTSON_NUMJAC"])
def test_bdf_kernel_is_under_the_same_control_flow_checks(pkg, tmp_path, model):
    """tests/test_k8_uniform_control.py's checks of the RK45 user kernel, on the BDF kernel: no cross-lane operation inside a
    cycle that lanes leave one by one, such cycles small, one memory atomic (the chunk dequeue), and no exec-mask control
    flow in the uniform attempt loop."""
    d = _bdf_dump(pkg, tmp_path, getattr(pkg.user_models, model), 3)
    U = _load_tool("uniformity_report")
    ll, uni = U.compile_ir(os.path.join(d, "smc_user_model.hip"), d, extra=("-I", d))
    name, cycles, n_div = U.kernel_cycles(ll, uni, "smc_user_solve_kernel")
    assert n_div > 0
    bad = [(c["depth"], len(c["blocks"]), c["cross_lane"][:3]) for c in cycles if c["cross_lane"]]
    assert not bad, f"{name}: cross-lane operations inside a cycle with a divergent exit: {bad}"
    assert all(len(c["blocks"]) <= 8 for c in cycles), f"{name}: a large cycle has a divergent exit: " \
        f"{[(c['depth'], len(c['blocks'])) for c in cycles]}"
    asm = os.path.join(d, "u.s")
    subprocess.run([HIPCC, *FLAGS, "-I", d, "-DSMC_ISA_MARKS", "-S", "--cuda-device-only", "-o", asm, os.path.join(d, "smc_user_model.hip")],
                   check=True, stderr=subprocess.DEVNULL, timeout=900)
    lines = open(asm).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("smc_user_solve_kernel:"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [l.strip() for l in lines[start:end]]
    atomics = [l for l in body if re.match(r"(global|flat|buffer)_atomic", l)]
    assert len(atomics) == 1 and re.match(r"global_atomic_add_x2 v\[\d+:\d+\], ", atomics[0]), atomics
    marks = [i for i, l in enumerate(body) if "MARK uniform_tail_attempt" in l]
    assert marks
    for mk in marks:
        lab, back = _innermost_loop(body, mk)
        loop = [l for l in body[lab:back + 1] if l and not l.startswith(";")]
        assert not [l for l in loop if re.match(r"s_\w+_saveexec", l)], f"{model}: exec-mask control flow in the uniform attempt loop"
    shutil.rmtree(tmp_path, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc from ROCm")
def test_three_state_bdf_kernel_has_no_scratch_stores(pkg, tmp_path):
    """NS <= 3: the item (D, J, LU, ...) and the attempt's temporaries stay in registers - no scratch store in the solve
    kernel, so none in its attempt loops (register budget)."""
    for model in ("ROBERTSON", "ROBERTSON_NUMJAC"):
        (tmp_path / model).mkdir()
        d = _bdf_dump(pkg, tmp_path / model, getattr(pkg.user_models, model), 3)
        asm = os.path.join(d, "u.s")
        subprocess.run([HIPCC, *FLAGS, "-I", d, "-S", "--cuda-device-only", "-o", asm, os.path.join(d, "smc_user_model.hip")],
                       check=True, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().split("\n")
        start = next(i for i, l in enumerate(lines) if l.startswith("smc_user_solve_kernel:"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        stores = [l.strip() for l in lines[start:end] if l.strip().startswith("scratch_store")]
        assert not stores, (model, stores[:4])


# ---- GPU -----------------------------------------------------------------------------------------------------------

def _scipy_population(th, analytic):
    """SciPy BDF on every (particle, experiment), in fresh processes (16 CPUs on the GPU box)."""
    n_proc = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4)
    with ProcessPoolExecutor(max_workers=n_proc, mp_context=multiprocessing.get_context("spawn")) as ex:
        rows = list(ex.map(RB.scipy_row, [(a, b, analytic) for a, b, _ in th], chunksize=8))
    y = np.array([r[0] for r in rows])                       # (n, n_ex, n_t)
    return y, sum(r[1] for r in rows), sum(r[2] for r in rows), sum(r[3] for r in rows)


ROB_PRIORS = {"k1": {"dist": "uniform", "low": 0, "high": 0.2}, "k3": {"dist": "uniform", "low": 0, "high": 5e4},
              "sigma": {"dist": "uniform", "low": 0, "high": 0.1}}


def _robertson_against_scipy(pkg, source, analytic):
    th, obs = RB.population()
    y_ref, steps, nlu, njev = _scipy_population(th, analytic)
    r = obs[None] - y_ref
    ref = RB.loglik(np.sum(r * r, axis=(1, 2)), th[:, 2])
    delta = RB.K_BOUND * (RB.ATOL + RB.RTOL * np.abs(y_ref))
    bound = np.sum(2 * np.abs(r) * delta + delta * delta, axis=(1, 2)) / (2 * th[:, 2] ** 2)
    n = th.shape[0]
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(ROB_PRIORS)
        eng.set_model_user(source, 3, RB.T, obs, cond=RB.A0[:, None], rtol=RB.RTOL, atol=RB.ATOL, method="BDF")
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        info = eng.loglik(pkg.SMC_SET_PRED)
        lk = eng.download_lk(pkg.SMC_SET_PRED)
        ctr = eng.user_sweep_counters()
    assert info["n_failed"] == 0
    err = np.abs(lk - ref)
    assert np.all(err <= bound), f"{int(np.sum(err > bound))} particles outside the bound; worst ratio {np.max(err / bound):.3g}"
    close = err <= 1e-8 * np.maximum(1.0, np.abs(ref))             # rounding level
    assert np.mean(close) >= 0.9, f"only {np.mean(close):.2%} of the particles agree to rounding level"
    for got, want, what in ((ctr["steps"], steps, "steps"), (ctr["lu_factorisations"], nlu, "LU factorisations"),
                            (ctr["jacobian_evals"], njev, "Jacobian evaluations")):
        assert abs(got - want) <= 0.01 * want, f"{what}: device {got}, SciPy {want}"
    assert info["rk_attempts"] >= ctr["steps"] and ctr["newton_iters"] >= ctr["steps"]


@pytest.mark.gpu
def test_robertson_with_jacobian_follows_scipy_bdf(pkg):
    _robertson_against_scipy(pkg, pkg.user_models.ROBERTSON, True)


@pytest.mark.gpu
def test_robertson_with_numerical_jacobian_follows_scipy_bdf(pkg):
    _robertson_against_scipy(pkg, pkg.user_models.ROBERTSON_NUMJAC, False)


@pytest.mark.gpu
def test_eight_state_chain_under_bdf_follows_scipy(pkg):
    """SMC_USER_MAX_STATES = 8 states under BDF (numerical Jacobian) against solve_ivp(method="BDF")."""
    from scipy.integrate import solve_ivp
    rs = np.random.RandomState(1)
    n_ex, n_t, n = 2, 25, 64
    t = np.tile(np.linspace(0.0, 20.0, n_t), (n_ex, 1))
    A0 = np.array([1.0, 3.0])
    obs = rs.uniform(0, 1, (n_ex, n_t))
    th = np.column_stack([rs.uniform(0.2, 2, n), rs.uniform(0.2, 2, n), rs.uniform(0.05, 0.5, n)])

    def rhs(_t, y, ka, kb):
        d = np.zeros(8)
        for i in range(8):
            k_in, k_out = (kb, ka) if i % 2 == 0 else (ka, kb)
            d[i] = (k_in * y[i - 1] if i > 0 else 0.0) - (k_out * y[i] if i < 7 else 0.0)
        return d
    ref = np.empty(n)
    for i, (ka, kb, sg) in enumerate(th):
        r2 = 0.0
        for e in range(n_ex):
            y0 = np.zeros(8)
            y0[0] = A0[e]
            sol = solve_ivp(rhs, [t[e, 0], t[e, -1]], y0, method="BDF", t_eval=t[e], rtol=1e-3, atol=1e-6, args=(ka, kb))
            r2 += np.sum((obs[e] - sol.y[7]) ** 2)
        ref[i] = n_ex * (-0.5 * n_t) * np.log(2 * np.pi * sg * sg) - r2 / (2 * sg * sg)
    priors = {"ka": {"dist": "uniform", "low": 0, "high": 3}, "kb": {"dist": "uniform", "low": 0, "high": 3},
              "sigma": {"dist": "uniform", "low": 0, "high": 1}}
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(priors)
        eng.set_model_user(CHAIN8, 8, t, obs, cond=A0[:, None], method="BDF")
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        info = eng.loglik(pkg.SMC_SET_PRED)
        lk = eng.download_lk(pkg.SMC_SET_PRED)
    assert info["n_failed"] == 0
    assert np.max(np.abs(lk - ref) / np.maximum(1.0, np.abs(ref))) < 1e-6


@pytest.mark.gpu
def test_bdf_failure_is_counted_and_the_kernel_returns(pkg):
    n = 256
    t = np.linspace(0.0, 2.0, 10)[None, :]
    th = np.column_stack([np.full(n, 0.5), np.full(n, 1.0), np.full(n, 0.1)])
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(pkg.SMCSettings().priors)
        eng.set_model_user(DIVERGING, 1, t, np.zeros_like(t), method="BDF")
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        info = eng.loglik(pkg.SMC_SET_PRED)
    assert info["n_failed"] == n


@pytest.mark.gpu
def test_bdf_metropolis_sweep_is_the_same_with_early_rejection(pkg):
    """Exact early rejection stops solves whose proposal is certain to be rejected: accept flags, particles and logL of a
    Metropolis sweep must be bit-identical with it on and off."""
    th0, obs = RB.population(n=4096, seed=5)
    rs = np.random.RandomState(3)
    n = th0.shape[0]
    th = np.column_stack([RB.K_TRUE[0] * (1 + 0.1 * rs.standard_normal(n)), RB.K_TRUE[1] * (1 + 0.1 * rs.standard_normal(n)),
                          rs.uniform(0.005, 0.03, n)])
    out = []
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(ROB_PRIORS)
        eng.set_model_user(pkg.user_models.ROBERTSON, 3, RB.T, obs, cond=RB.A0[:, None], rtol=RB.RTOL, atol=RB.ATOL, method="BDF")
        eng.upload_particles(pkg.SMC_SET_PRED, th)
        info = eng.loglik(pkg.SMC_SET_PRED)
        lk = eng.download_lk(pkg.SMC_SET_PRED)
        assert info["n_failed"] == 0
        for on in (False, True):
            eng.upload_particles(pkg.SMC_SET_FILT, th)
            eng.upload_lk(pkg.SMC_SET_FILT, lk)
            eng.set_early_reject(on)
            mh = eng.mh_step_device_rng(0.5, 1.0, np.diag([0.004, 1000.0, 0.002]), 7, 3)
            out.append((mh, eng.download_particles(pkg.SMC_SET_FILT), eng.download_lk(pkg.SMC_SET_FILT),
                        eng.user_sweep_counters()))
    (m0, p0, l0, c0), (m1, p1, l1, c1) = out
    assert m0["n_failed"] == 0 and 0 < m0["accepted_now"] < n
    assert m0["accepted_now"] == m1["accepted_now"] and np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert m1["rk_attempts"] <= m0["rk_attempts"] and c1["steps"] <= c0["steps"]


@pytest.mark.gpu
def test_stiff_model_full_run_recovers_the_generating_constants(pkg):
    _, obs = RB.population(n=1)
    n = 8192
    s = pkg.SMCSettings(n_particle=n, priors=ROB_PRIORS, rtol=RB.RTOL, atol=RB.ATOL)
    with pkg.HipEngine(n, 3, device=0) as eng:
        eng.set_prior(ROB_PRIORS)
        eng.set_model_user(pkg.user_models.ROBERTSON, 3, RB.T, obs, cond=RB.A0[:, None], rtol=RB.RTOL, atol=RB.ATOL, method="BDF")
        out = pkg.run_smc(eng, s, rng="device", verbose=False, seed_device=3)
    assert out["gamma"] == 1.0
    m, sd = out["p_pred"].mean(axis=0), out["p_pred"].std(axis=0)
    k_true = np.array(RB.K_TRUE)
    assert np.all(np.abs(m[:2] - k_true) < 5 * sd[:2] + 0.02 * k_true), (m, sd)
    assert abs(m[2] - RB.SIGMA_TRUE) < 0.004, (m, sd)


@pytest.mark.gpu
def test_unknown_method_raises_and_rk45_has_no_bdf_counters(pkg):
    t = np.linspace(0.0, 1.0, 5)[None, :]
    with pkg.HipEngine(64, 3, device=0) as eng:
        with pytest.raises(ValueError, match="method"):
            eng.set_model_user(pkg.user_models.ROBERTSON, 3, t, np.zeros_like(t), cond=[[1.0]], method="Radau")
        eng.set_model_user(pkg.user_models.CONSECUTIVE_REACTIONS, 2, t, np.zeros_like(t), cond=[[1.0]])
        with pytest.raises(pkg.SmcError, match="BDF"):
            eng.user_sweep_counters()
