"""Cost of state-triggered events (include/smc_hip.h: STATE-TRIGGERED EVENTS; csrc/user_root.h) in the RK45 solve kernel: the
model of tests/triggered_model.py's T1, y' = -th0 y, on 4 experiments of 20 times over [0, 10], three ways:

    (a) no roots       the source without the root names: the kernel text without its SMC_USER_ROOTS blocks
    (b) never fires    the root names compiled in with a threshold no state reaches: the same trajectory, the machinery's cost
    (c) fires          T1 itself, g = y - L falling, the event adds th1: several fires, hence segments, per solve

    python tools/user_root_bench.py --census          registers and scratch of the sweep and prediction kernels of (a) and (c)
                                                       (no GPU: the sources are dumped and compiled off line with hiprtc's flags)
    python tools/user_root_bench.py [n] [rounds]      SMC_T_SOLVE (HIP events) of a likelihood sweep over n (default 65 536)
                                                       posterior-like particles, one engine per variant, after a warm-up sweep
                                                       each, ALTERNATING, `rounds` (default 9) times each
    ... --plain-only                                   (a) alone: with SMC_HIP_LIB set to another build's library, the same
                                                       sweep on that build (a parent without the feature knows (a) only)

(a) and (b) integrate the same function and must report the same attempts.  One JSON line per variant, then the ratios to (a)
of the medians with the spread of the rounds."""
import ctypes
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
SRC_FIRES = pkg.user_models.THRESHOLD_REDOSED
SRC_PLAIN = "\n".join(ln for ln in SRC_FIRES.split("\n") if "smc_user_root" not in ln)
SRC_NEVER = SRC_FIRES.replace("g[0] = y[0] - cond[1];", "g[0] = y[0] + 1.0e3;")
N_EX, T_END = 4, 10.0
COND = np.array([[1.0, 0.4], [0.5, 0.2], [2.0, 0.7], [0.8, 0.3]])
VARIANTS = [("no roots", SRC_PLAIN), ("never fires", SRC_NEVER), ("fires", SRC_FIRES)]


def census():
    L = pkg.lib()
    for name, src in (VARIANTS[0], VARIANTS[2]):
        with tempfile.TemporaryDirectory() as d:
            spec = pkg.binding.UserSourceSpec(source=src.encode(), n_states=1, dim=3, method=0, n_obs=1, n_cond=2)
            assert L.smc_user_model_dump_source_spec(ctypes.byref(spec), d.encode()) == 0
            s = os.path.join(d, "listing.s")
            subprocess.run([HIPCC, *FLAGS, "-I", d, "-S", "--cuda-device-only", "-o", s, os.path.join(d, "smc_user_model.hip")], check=True,
                           stderr=subprocess.DEVNULL, timeout=900)
            meta = open(s).read()
        out = {"kernel": name}
        for fn in ("smc_user_solve_kernel", "smc_user_predict_kernel"):
            k = meta.index(f".name:           {fn}\n")
            blk = meta[meta.rindex("  - .agpr_count", 0, k):]
            blk = blk[:blk.index("  - .agpr_count", 10) if "  - .agpr_count" in blk[10:] else len(blk)]
            out[fn] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                       for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}
        print(json.dumps(out), flush=True)


def _exact(th, cond, t):
    """T1's exact y(t) for one experiment: decay, and a jump by th[1] at every crossing of cond[1]."""
    k, D, (y, L) = th[0], th[1], cond
    out, a = np.empty_like(t), 0.0
    for i, x in enumerate(t):
        while y * np.exp(-k * (x - a)) < L:      # a fire before x
            a += np.log(y / L) / k
            y = L + D
        out[i] = y * np.exp(-k * (x - a))
    return out


def bench(n, rounds, plain_only):
    rs = np.random.RandomState(0)
    t = np.tile(np.linspace(0.0, T_END, 20), (N_EX, 1))
    th_true = np.array([0.6, 0.9, 0.05])
    noise = th_true[2] * rs.standard_normal(t.shape)
    th = th_true + np.array([0.01, 0.01, 0.002]) * rs.standard_normal((n, 3))      # posterior-like
    variants = VARIANTS[:1] if plain_only else VARIANTS
    engines = []
    try:
        for name, src in variants:
            eng = pkg.HipEngine(n, 3, device=0)
            engines.append(eng)
            eng.set_prior({f"p{j}": {"dist": "uniform", "low": 0, "high": 10} for j in range(3)})
            clean = np.array([_exact(th_true, COND[e], t[e]) if name == "fires" else COND[e, 0] * np.exp(-th_true[0] * t[e]) for e in range(N_EX)])
            eng.set_model_user(src, 1, t, (clean + noise)[:, :, None], cond=COND)
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
        for (name, _), m, i in zip(variants, ms, info):
            print(json.dumps({"kernel": name, "library": os.environ.get("SMC_HIP_LIB", "this build"), "particles": n, "experiments": N_EX,
                              "solve_ms_median": round(float(np.median(m)), 4), "solve_ms_min": round(min(m), 4), "solve_ms_max": round(max(m), 4),
                              "solve_ms_all": [round(x, 4) for x in m], "rk_attempts": i["rk_attempts"], "n_failed": i["n_failed"]}), flush=True)
        if not plain_only:
            print(json.dumps({"ratio_to_no_roots": {name: round(med[j] / med[0], 4) for j, (name, _) in enumerate(variants)},
                              "spread_max_over_min": {name: round(max(ms[j]) / min(ms[j]), 4) for j, (name, _) in enumerate(variants)}}), flush=True)
    finally:
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    if "--census" in sys.argv:
        census()
    else:
        args = [x for x in sys.argv[1:] if not x.startswith("-")]
        bench(int(args[0]) if args else 65_536, int(args[1]) if len(args) > 1 else 9, "--plain-only" in sys.argv)
