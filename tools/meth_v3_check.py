"""Two builds / kernels of K8 on the same solves, compared EXACTLY: flows, status and the five counters.
    tools/meth_v3_check.py [n_particles=16] [a=two-wave] [b=one-wave]
A variant is `one-wave` or `two-wave` (SMC_K8_SPLIT=0 / 1), optionally followed by `@<path of a libsmc_hip.so>` (handed to the
binding through SMC_HIP_LIB; without it the in-tree library), e.g.
    tools/meth_v3_check.py 16 two-wave two-wave@build/ab/parent/libsmc_hip.so
The solves are n_particles prior-box parameter vectors x 30 experiments, the vectors of
tests/test_gpu_methanation.py::test_two_wave_kernel_equals_the_one_wave_kernel_bit_for_bit (RandomState(11)): at 16 particles some
of them fail and run their whole attempt budget.  Each variant runs in a child process of its own (the library is chosen when
the binding is imported).  Exit status 1 when anything differs."""
import os, sys, subprocess, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

COUNTERS = ("steps", "rejects", "newton_fail", "newton_iters", "factorisations")


def run(n_part):
    import __graft_entry__ as g
    pkg = g.load_package()
    g.load_oracle()
    from oracle import methanation as M      # the test's parameter vectors are built with the checker's settings layer
    cond = M.load_conditions(os.path.join(g.ROOT, "tests", "golden", "methanation_information.csv"))
    guess = M.initial_guess(cond)
    lo, hi, pos = M.prior_box()
    rs = np.random.RandomState(11)
    prs = np.tile(M.BASEPARAMS, (n_part, 1))
    prs[:, :4] = (lo[pos] + (hi[pos] - lo[pos]) * rs.uniform(0, 1, (n_part, 5)))[:, :4]
    p0 = np.array([M.p0_tuple(cond, i, pr) for pr in prs for i in range(30)])
    y0 = np.array([guess[i] for pr in prs for i in range(30)])
    flows, status, _, info = pkg.methanation.dae_solve_batch(p0, y0)
    return flows, status, info


def variant_env(tag):
    kernel, _, lib = tag.partition("@")
    env = {"SMC_K8_SPLIT": {"one-wave": "0", "two-wave": "1"}[kernel]}
    if lib:
        env["SMC_HIP_LIB"] = os.path.abspath(lib)
    return env


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    if os.environ.get("SMC_CHILD"):
        f, s, info = run(n)
        np.savez(os.environ["SMC_CHILD"], flows=f, status=s, info=json.dumps({k: int(info[k]) for k in COUNTERS}))
        sys.exit(0)
    tags = [sys.argv[2] if len(sys.argv) > 2 else "two-wave", sys.argv[3] if len(sys.argv) > 3 else "one-wave"]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, tag in enumerate(tags):
            path = os.path.join(tmp, f"variant{i}.npz")
            e = {k: v for k, v in os.environ.items() if k != "SMC_HIP_LIB"}
            e.update(SMC_CHILD=path, **variant_env(tag))
            subprocess.run([sys.executable, os.path.abspath(__file__), str(n)], env=e, check=True, timeout=300)
            with np.load(path) as z:
                out.append((z["flows"], z["status"], json.loads(str(z["info"]))))
            print(f"{tag}: {out[-1][2]}, failed solves {int((out[-1][1] != 0).sum())}", flush=True)
    (fa, sa, ia), (fb, sb, ib) = out
    same = {"flows": np.array_equal(fa, fb, equal_nan=True), "status": np.array_equal(sa, sb)}
    same.update({k: ia[k] == ib[k] for k in COUNTERS})
    print(f"{tags[0]} against {tags[1]}, {len(sa)} solves, {int((sa != 0).sum())} failed: " +
          ", ".join(f"{k} {'equal' if v else 'DIFFERENT'}" for k, v in same.items()))
    sys.exit(0 if all(same.values()) else 1)
