"""Cost of count observations (include/smc_hip.h: COUNT OBSERVATIONS; csrc/user_count.h) in the RK45 solve kernel of the
A -> B -> C model of tests/count_chain.py (A Gaussian, V B counted) on its 4 x 30 data set.

    python tools/user_count_bench.py --census          registers, spills, private segment and the scratch instructions inside the
                                                        bulk attempt loop of the sweep kernel: the counts Poisson and negative
                                                        binomial, beside the same source with noise = 2 plus censoring (no GPU: the
                                                        sources are dumped and compiled off line with hiprtc's flags and
                                                        -DSMC_ISA_MARKS)
    python tools/user_count_bench.py [n] [rounds]      SMC_T_SOLVE (HIP events) of a likelihood sweep over n (default 100 000)
                                                        posterior-like particles, one engine per variant, after a warm-up sweep each,
                                                        ALTERNATING, `rounds` (default 9) times:
                                                          (a) the counts declared Gaussian with a proportional part (the parent's path)
                                                          (b) the count output Poisson
                                                          (c) the count output negative binomial
                                                        then a Metropolis sweep of (a) and (b) with and without early rejection: the
                                                        attempts it saves

One JSON line per variant, then the ratios of the medians."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import __graft_entry__ as g
import count_chain as CC

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-fno-fast-math"]      # user_model.hip: compile_user
pkg = g.load_package()
B = pkg.binding


def _innermost_loop(body, mk):
    """(index of the loop's first label, index of the last branch back to it) for the innermost loop around line mk"""
    for lab in range(mk, -1, -1):
        if not re.match(r"^\.LBB\d+_\d+:", body[lab]):
            continue
        label = body[lab].split(":")[0]
        back = [i for i in range(mk, len(body)) if re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", body[i])]
        if back:
            return lab, back[-1]
    raise AssertionError("no loop around the mark")


def census():
    import ctypes
    L = pkg.lib()
    for name, fam, noise, censor in (("gaussian, noise = 2 + censoring", None, 2, 1), ("gaussian, noise = 2", None, 2, 0),
                                     ("poisson, noise = 1", (0, 1), 1, 0), ("negative binomial, noise = 2", (0, 2), 2, 0),
                                     ("negative binomial, noise = 2 + censoring", (0, 2), 2, 1)):
        with tempfile.TemporaryDirectory() as d:
            spec = B.UserSourceSpec(source=CC.source(fam).encode(), n_states=2, dim=4, method=0, n_obs=2, noise=noise, n_cond=2, censor=censor)
            assert L.smc_user_model_dump_source_spec(ctypes.byref(spec), d.encode()) == 0
            s = os.path.join(d, "listing.s")
            subprocess.run([HIPCC, *FLAGS, "-I", d, "-DSMC_ISA_MARKS", "-S", "--cuda-device-only", "-o", s,
                            os.path.join(d, "smc_user_model.hip")], check=True, stderr=subprocess.DEVNULL, timeout=900)
            meta = open(s).read()
        lines = meta.split("\n")
        start = next(i for i, ln in enumerate(lines) if ln.startswith("smc_user_solve_kernel:"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [ln.strip() for ln in lines[start:end]]
        mark = next(i for i, ln in enumerate(body) if "MARK bulk_attempt" in ln)
        lab, back = _innermost_loop(body, mark)
        out = {"kernel": name,
               "bulk_attempt_loop_scratch_instructions": sum(1 for x in body[lab:back + 1] if x.startswith("scratch_")),
               "solve_kernel_scratch_instructions": sum(1 for x in body if x.startswith("scratch_")),
               "solve_kernel_calls": sum(1 for x in body if x.startswith("s_swappc"))}
        for fn in ("smc_user_solve_kernel", "smc_user_predict_kernel"):
            k = meta.index(f".name:           {fn}\n")
            blk = meta[meta.rindex("  - .agpr_count", 0, k):]
            blk = blk[:blk.index("  - .agpr_count", 10) if "  - .agpr_count" in blk[10:] else len(blk)]
            out[fn] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                       for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}
        print(json.dumps(out), flush=True)


def bench(n, rounds):
    rs = np.random.RandomState(0)
    mean, sd = np.array([0.7965, 0.3063, 0.0111, 0.5118]), np.array([0.0036, 0.0131, 0.0008, 0.0391])
    th = mean + sd * rs.standard_normal((n, 4))
    gauss_prop = {"additive": [("param", 2), ("fixed", 1.0)], "proportional": [("fixed", 0.0), ("param", 3)]}
    variants = [("(a) counts declared Gaussian with a proportional part", None, gauss_prop, CC.make_data(0)),
                ("(b) Poisson", (0, 1), CC.NOISE_POISSON, CC.make_data(0)),
                ("(c) negative binomial", (0, 2), CC.NOISE_NB, CC.make_data(0))]
    engines = []
    priors = {nm: {"dist": "uniform", "low": 0, "high": float(h)} for nm, h in zip(CC.NAMES, CC.PRIOR_HIGH)}
    try:
        for name, fam, noise, (t, obs) in variants:
            eng = pkg.HipEngine(n, 4, device=0)
            engines.append(eng)
            eng.set_prior(priors)
            eng.set_model_user(CC.source(fam), 2, t, obs, cond=CC.COND, noise=noise)
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            eng.loglik(pkg.SMC_SET_PRED)                      # warm-up
            eng.timing_enable(True)
        ms = [[] for _ in variants]
        info = [None] * len(variants)
        for _ in range(rounds):
            for j, eng in enumerate(engines):
                eng.timing_reset()
                info[j] = eng.loglik(pkg.SMC_SET_PRED)
                eng.synchronize()
                ms[j].append(eng.timing_get()["solve"]["ms"])
        med = [float(np.median(m)) for m in ms]
        for (name, _, _, _), m, i in zip(variants, ms, info):
            print(json.dumps({"variant": name, "particles": n, "solve_ms_median": round(float(np.median(m)), 4), "solve_ms_min": round(min(m), 4),
                              "solve_ms_max": round(max(m), 4), "solve_ms_all": [round(x, 4) for x in m], "rk_attempts": i["rk_attempts"],
                              "n_failed": i["n_failed"]}), flush=True)
        print(json.dumps({"ratio_poisson_to_gaussian": round(med[1] / med[0], 4), "ratio_negbin_to_gaussian": round(med[2] / med[0], 4)}), flush=True)
        # attempts saved by early rejection: one Metropolis sweep from the same particles and the same draws
        for j in (0, 1):
            eng = engines[j]
            lk = eng.download_lk(pkg.SMC_SET_PRED)
            att = {}
            for on in (False, True):
                eng.upload_particles(pkg.SMC_SET_FILT, th)
                eng.upload_lk(pkg.SMC_SET_FILT, lk)
                eng.set_early_reject(on)
                mh = eng.mh_step_device_rng(0.5, 1.0, np.diag([0.004, 0.004, 2e-5, 1e-3]), 7, 3)      # the proposal of tests/test_user_counts.py
                att[on] = (mh["rk_attempts"], mh["accepted_now"])
            print(json.dumps({"variant": variants[j][0], "metropolis_attempts_without_early_rejection": att[False][0],
                              "with": att[True][0], "saved_share": round(1.0 - att[True][0] / att[False][0], 5), "accepted": att[True][1]}), flush=True)
    finally:
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    if "--census" in sys.argv:
        census()
    else:
        args = [x for x in sys.argv[1:] if not x.startswith("-")]
        bench(int(args[0]) if args else 100_000, int(args[1]) if len(args) > 1 else 9)
