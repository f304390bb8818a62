"""Cost of censored observations (include/smc_hip.h: smc_set_model_user7; csrc/user_censor.h) in the RK45 solve kernel of
CONSECUTIVE_REACTIONS_AB on the data of tests/noise_model_chain.py.

    python tools/user_censor_bench.py --census          registers, spills, private segment and the scratch instructions inside the
                                                         bulk attempt loop of the sweep kernel, additive-only and combined, without
                                                         and with SMC_USER_CENSOR (no GPU: the sources are dumped and compiled off
                                                         line with hiprtc's flags and -DSMC_ISA_MARKS)
    python tools/user_censor_bench.py [n] [rounds]      SMC_T_SOLVE (HIP events) of a likelihood sweep over n (default 65 536)
                                                         posterior-like particles under the combined noise model, one engine per
                                                         variant, after a warm-up sweep each, ALTERNATING, `rounds` (default 9) times:
                                                           (a) the noise model without censoring
                                                           (b) the same data with a third of the values censored (both outputs at
                                                               their 1/3 quantile, from the left)
    ... --only-a                                         variant (a) alone: what a build of the parent revision (SMC_HIP_LIB) can run

One JSON line per variant, then the ratio of the medians with the spread of the rounds."""
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
import noise_model_chain as NC

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-fno-fast-math"]      # user_model.hip: compile_user
pkg = g.load_package()
SRC = pkg.user_models.CONSECUTIVE_REACTIONS_AB


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
    L = pkg.lib()
    for noise, dim, name in ((1, 4, "additive-only"), (2, 5, "combined")):
        for censor in (0, 1):
            with tempfile.TemporaryDirectory() as d:
                assert L.smc_user_model_dump_source7(SRC.encode(), 2, dim, 0, 2, noise, 1, 0, 0, 0, 0, censor, d.encode()) == 0
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
            out = {"kernel": name, "SMC_USER_CENSOR": censor,
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


def bench(n, rounds, only_a):
    t, values = NC.make_data(0)
    values = np.where(np.isnan(t)[:, :, None], np.nan, values)
    obs_c, censor = pkg.user_models.censor_data(values, lower=np.nanquantile(values, 1.0 / 3.0, axis=(0, 1)))
    rs = np.random.RandomState(0)
    mean, sd = np.array([0.7923, 0.2975, 0.0114, 0.0203, 0.0778]), np.array([0.0062, 0.0017, 0.0011, 0.0015, 0.0129])
    th = mean + sd * rs.standard_normal((n, 5))
    variants = [("(a) noise model", values, None)] + ([] if only_a else [("(b) a third censored", obs_c, censor)])
    engines = []
    try:
        for name, obs, c in variants:
            eng = pkg.HipEngine(n, 5, device=0)
            engines.append(eng)
            eng.set_prior({f"p{j}": {"dist": "uniform", "low": 0, "high": 10} for j in range(5)})
            eng.set_model_user(SRC, 2, t, obs, cond=NC.A0[:, None], noise=NC.NOISE, **({} if c is None else {"censor": c}))
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
        for (name, _, c), m, i in zip(variants, ms, info):
            print(json.dumps({"variant": name, "library": os.environ.get("SMC_HIP_LIB", "in-tree"), "particles": n,
                              "censored_share": 0.0 if c is None else round(float((c != 0).sum() / np.isfinite(values).sum()), 3),
                              "solve_ms_median": round(float(np.median(m)), 4), "solve_ms_min": round(min(m), 4),
                              "solve_ms_max": round(max(m), 4), "solve_ms_all": [round(x, 4) for x in m], "rk_attempts": i["rk_attempts"],
                              "n_failed": i["n_failed"]}), flush=True)
        if not only_a:
            print(json.dumps({"ratio_b_to_a": round(med[1] / med[0], 4),
                              "spread_max_over_min": {name: round(max(ms[j]) / min(ms[j]), 4) for j, (name, _, _) in enumerate(variants)}}),
                  flush=True)
    finally:
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    if "--census" in sys.argv:
        census()
    else:
        args = [x for x in sys.argv[1:] if not x.startswith("-")]
        bench(int(args[0]) if args else 65_536, int(args[1]) if len(args) > 1 else 9, "--only-a" in sys.argv)
