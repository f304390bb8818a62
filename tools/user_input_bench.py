"""Cost of the input lookup (include/smc_hip.h: smc_set_model_user5, smc_input; csrc/user_input.h) in the RK45 solve kernel: the
same one-state model, y' = -th0 y + th1 u(t) with u a ramp from u_a at t = 0 to u_b at t = 10, written four ways:

    (a) closed form    u = cond[1] + cond[2] * t                  two cond numbers, no table
    (b) 2 knots        smc_input(cond, 0, t), the ramp's two ends
    (c) 64 knots       the same ramp sampled at 64 knots
    (c) 256 knots      ... and at 256

    python tools/user_input_bench.py --census         registers, scratch and LDS of the four sweep kernels (no GPU: the sources
                                                       are dumped and compiled off line with hiprtc's flags)
    python tools/user_input_bench.py [n] [rounds]     SMC_T_SOLVE (HIP events) of a likelihood sweep over n (default 65 536)
                                                       posterior-like particles at the default tolerances, one engine per
                                                       variant, after a warm-up sweep each, ALTERNATING, `rounds` (default 9)
                                                       times each

All four integrate the same function, so their attempt counts agree up to rounding (a sampled ramp is the ramp to an ulp of
u); they are reported.  One JSON line per variant, then the ratios to (a) of the medians with the spread of the rounds."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import __graft_entry__ as g

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-fno-fast-math"]      # user_model.hip: compile_user
pkg = g.load_package()
_SIG = "const double *theta, const double *cond"
SRC = f"""
__device__ void smc_user_y0({_SIG}, double *y) {{ y[0] = cond[0]; }}
__device__ void smc_user_rhs(double t, const double *y, {_SIG}, double *dydt) {{ dydt[0] = -theta[0] * y[0] + theta[1] * INPUT; }}
__device__ double smc_user_obs(double t, const double *y, {_SIG}) {{ return y[0]; }}
"""
SRC_CLOSED = SRC.replace("INPUT", "(cond[1] + cond[2] * t)")
SRC_TABLE = SRC.replace("INPUT", "smc_input(cond, 0, t)")
N_EX, T_END = 4, 10.0
U_A = np.array([0.5, 1.0, 0.2, 1.5])
U_B = np.array([2.0, 0.3, 1.2, 1.5])
VARIANTS = [("closed form", 0), ("2 knots", 2), ("64 knots", 64), ("256 knots", 256)]


def census():
    L = pkg.lib()
    for name, knots in VARIANTS:
        with tempfile.TemporaryDirectory() as d:
            src = SRC_TABLE if knots else SRC_CLOSED
            assert L.smc_user_model_dump_source5(src.encode(), 1, 3, 0, 1, 0, 1 if knots else 3, 1 if knots else 0, knots, d.encode()) == 0
            s = os.path.join(d, "listing.s")
            subprocess.run([HIPCC, *FLAGS, "-I", d, "-S", "--cuda-device-only", "-o", s, os.path.join(d, "smc_user_model.hip")], check=True,
                           stderr=subprocess.DEVNULL, timeout=900)
            meta = open(s).read()
        body = meta[meta.index("smc_user_solve_kernel:"):meta.index(".Lfunc_end", meta.index("smc_user_solve_kernel:"))]
        out = {"kernel": name, "solve_kernel_scratch_instructions": len(re.findall(r"\bscratch_(?:load|store)", body)),
               "solve_kernel_global_loads": len(re.findall(r"\bglobal_load", body))}
        for fn in ("smc_user_solve_kernel", "smc_user_predict_kernel"):
            k = meta.index(f".name:           {fn}\n")
            blk = meta[meta.rindex("  - .agpr_count", 0, k):]
            blk = blk[:blk.index("  - .agpr_count", 10) if "  - .agpr_count" in blk[10:] else len(blk)]
            out[fn] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                       for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}
        print(json.dumps(out), flush=True)


def bench(n, rounds):
    rs = np.random.RandomState(0)
    t = np.tile(np.linspace(0.0, T_END, 20), (N_EX, 1))
    y0 = np.array([1.0, 0.5, 2.0, 0.8])
    th_true = np.array([0.8, 1.2, 0.05])
    k = th_true[0]
    a, b = th_true[1] * U_A[:, None], th_true[1] * ((U_B - U_A) / T_END)[:, None]
    f = (y0[:, None] - a / k + b / k ** 2) * np.exp(-k * t) + (a + b * t) / k - b / k ** 2
    obs = f + th_true[2] * rs.standard_normal(f.shape)
    th = th_true + np.array([0.01, 0.015, 0.002]) * rs.standard_normal((n, 3))      # posterior-like
    engines = []
    try:
        for name, knots in VARIANTS:
            eng = pkg.HipEngine(n, 3, device=0)
            engines.append(eng)
            eng.set_prior({f"p{j}": {"dist": "uniform", "low": 0, "high": 10} for j in range(3)})
            if knots:
                tk = np.tile(np.linspace(0.0, T_END, knots), (N_EX, 1))
                u = U_A[:, None] + (U_B - U_A)[:, None] * (tk / T_END)
                eng.set_model_user(SRC_TABLE, 1, t, obs, cond=y0[:, None], inputs={"t": tk, "u": u})
            else:
                eng.set_model_user(SRC_CLOSED, 1, t, obs, cond=np.column_stack([y0, U_A, (U_B - U_A) / T_END]))
            eng.upload_particles(pkg.SMC_SET_PRED, th)
            eng.loglik(pkg.SMC_SET_PRED)                      # warm-up
            eng.timing_enable(True)
        ms = [[] for _ in VARIANTS]
        info = [None] * len(VARIANTS)
        for _ in range(rounds):
            for j, eng in enumerate(engines):
                eng.timing_reset()
                info[j] = eng.loglik(pkg.SMC_SET_PRED)
                eng.synchronize()
                ms[j].append(eng.timing_get()["solve"]["ms"])
        med = [float(np.median(m)) for m in ms]
        for (name, knots), m, i in zip(VARIANTS, ms, info):
            print(json.dumps({"kernel": name, "particles": n, "experiments": N_EX, "solve_ms_median": round(float(np.median(m)), 4),
                              "solve_ms_min": round(min(m), 4), "solve_ms_max": round(max(m), 4), "solve_ms_all": [round(x, 4) for x in m],
                              "rk_attempts": i["rk_attempts"], "n_failed": i["n_failed"]}), flush=True)
        print(json.dumps({"ratio_to_closed_form": {name: round(med[j] / med[0], 4) for j, (name, _) in enumerate(VARIANTS)},
                          "spread_max_over_min": {name: round(max(ms[j]) / min(ms[j]), 4) for j, (name, _) in enumerate(VARIANTS)}}), flush=True)
    finally:
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    if "--census" in sys.argv:
        census()
    else:
        args = [x for x in sys.argv[1:] if not x.startswith("-")]
        bench(int(args[0]) if args else 65_536, int(args[1]) if len(args) > 1 else 9)
