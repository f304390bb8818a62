"""Cost of a noise model (include/smc_hip.h: smc_set_model_user4) in the solve kernel of CONSECUTIVE_REACTIONS_AB, RK45.

    python tools/user_noise_bench.py --census            registers, scratch and LDS of the three sweep kernels (no GPU: the
                                                          sources are dumped and compiled off line with hiprtc's flags)
    python tools/user_noise_bench.py [n] [rounds]        SMC_T_SOLVE of a likelihood sweep over n (default 10^6) posterior-like
                                                          particles: the smc_set_model_user3 path (one sigma), the additive-only
                                                          and the combined variant, ALTERNATING, `rounds` (default 7) times each

One JSON line per kernel.  The smc_set_model_user3 kernel is the parent revision's, instruction for instruction
(tools/user_source_equiv.py), so one build serves all three."""
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
ADD = {"additive": [("param", 2), ("param", 3)]}
# name, dim, keyword arguments of set_model_user, columns of (k1, k2, a0, a1, b0) the particles are made of
VARIANTS = [("user3 (one sigma)", 3, {}, (0, 1, 2)), ("additive-only", 4, {"noise": ADD}, (0, 1, 2, 3)),
            ("combined", 5, {"noise": NC.NOISE}, (0, 1, 2, 3, 4))]


def census():
    L = pkg.lib()
    for name, dim, kw, _ in VARIANTS:
        with tempfile.TemporaryDirectory() as d:
            if kw:
                rc = L.smc_user_model_dump_source4(SRC.encode(), 2, dim, 0, 2, int("proportional" in kw["noise"]), d.encode())
            else:
                rc = L.smc_user_model_dump_source3(SRC.encode(), 2, dim, 0, 2, d.encode())
            assert rc == 0
            s = os.path.join(d, "listing.s")
            subprocess.run([HIPCC, *FLAGS, "-I", d, "-S", "--cuda-device-only", "-o", s, os.path.join(d, "smc_user_model.hip")], check=True,
                           stderr=subprocess.DEVNULL, timeout=900)
            meta = open(s).read()
        out = {"kernel": name, "dim": dim}
        for fn in ("smc_user_solve_kernel", "smc_user_predict_kernel"):
            k = meta.index(f".name:           {fn}\n")
            blk = meta[meta.rindex("  - .agpr_count", 0, k):]
            blk = blk[:blk.index("  - .agpr_count", 10) if "  - .agpr_count" in blk[10:] else len(blk)]
            out[fn] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                       for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}
        print(json.dumps(out), flush=True)


def bench(n, rounds):
    t, obs = NC.make_data(0)
    rs = np.random.RandomState(0)
    mean, sd = np.array([0.7923, 0.2975, 0.0114, 0.0203, 0.0778]), np.array([0.0062, 0.0017, 0.0011, 0.0015, 0.0129])
    th = mean + sd * rs.standard_normal((n, 5))
    engines = []
    try:
        for name, dim, kw, cols in VARIANTS:
            eng = pkg.HipEngine(n, dim, device=0)
            engines.append(eng)
            eng.set_prior({f"p{j}": {"dist": "uniform", "low": 0, "high": 10} for j in range(dim)})
            eng.set_model_user(SRC, 2, t, obs, cond=NC.A0[:, None], **kw)
            eng.upload_particles(pkg.SMC_SET_PRED, np.ascontiguousarray(th[:, cols]))
            eng.loglik(pkg.SMC_SET_PRED)
            eng.timing_enable(True)
        ms = [[] for _ in VARIANTS]
        info = [None] * len(VARIANTS)
        for _ in range(rounds):
            for j, eng in enumerate(engines):
                eng.timing_reset()
                info[j] = eng.loglik(pkg.SMC_SET_PRED)
                eng.synchronize()
                ms[j].append(eng.timing_get()["solve"]["ms"])
        for (name, dim, _, _), m, i in zip(VARIANTS, ms, info):
            print(json.dumps({"kernel": name, "dim": dim, "particles": n, "solve_ms_median": round(float(np.median(m)), 4),
                              "solve_ms_min": round(min(m), 4), "solve_ms_all": [round(x, 4) for x in m], "rk_attempts": i["rk_attempts"],
                              "n_failed": i["n_failed"]}), flush=True)
    finally:
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    if "--census" in sys.argv:
        census()
    else:
        a = [x for x in sys.argv[1:] if not x.startswith("-")]
        bench(int(a[0]) if a else 1_000_000, int(a[1]) if len(a) > 1 else 7)
