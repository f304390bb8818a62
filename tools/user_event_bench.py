"""Cost of scheduled events (include/smc_hip.h: smc_set_model_user6, smc_user_event; csrc/user_event.h) in the RK45 solve kernel:
the one-compartment model of tests/dosed_model.py's E1, y' = -th0 y, on 4 experiments of 20 times over [0, 10], three ways:

    (a) no events      the source without smc_user_event, data without doses: the kernel text without its SMC_USER_EVENTS blocks
    (b) empty rows     the source with smc_user_event, the machinery compiled in (room for 3 events), every row empty
    (c) 3 events       three bolus doses per experiment at 2.5, 5 and 7.5 (none on a data time), data simulated with them

    python tools/user_event_bench.py --census         registers, scratch and LDS of the sweep and prediction kernels of (a) and (c)
                                                       (no GPU: the sources are dumped and compiled off line with hiprtc's flags)
    python tools/user_event_bench.py [n] [rounds]     SMC_T_SOLVE (HIP events) of a likelihood sweep over n (default 65 536)
                                                       posterior-like particles at the default tolerances, one engine per
                                                       variant, after a warm-up sweep each, ALTERNATING, `rounds` (default 9)
                                                       times each

(a) and (b) integrate the same function and must report the same attempts; (c) solves four segments per experiment, each with
its own start-up (two right-hand sides and a small first step), so it needs more attempts.  One JSON line per variant, then the
ratios to (a) of the medians with the spread of the rounds."""
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
SRC_EVENTS = pkg.user_models.ONE_COMPARTMENT_DOSED
SRC_PLAIN = "\n".join(ln for ln in SRC_EVENTS.split("\n") if "smc_user_event" not in ln)
N_EX, T_END, N_EV = 4, 10.0, 3
EV_T = np.tile([2.5, 5.0, 7.5], (N_EX, 1))
DOSE = np.array([[0.8, 0.5, 0.6], [0.4, 0.4, 0.4], [1.0, 0.2, 0.7], [0.3, 0.9, 0.5]])
VARIANTS = [("no events", SRC_PLAIN, None), ("empty rows", SRC_EVENTS, np.full((N_EX, N_EV), np.nan)), ("3 events", SRC_EVENTS, EV_T)]


def census():
    L = pkg.lib()
    for name, src, ev_t in (VARIANTS[0], VARIANTS[2]):
        with tempfile.TemporaryDirectory() as d:
            assert L.smc_user_model_dump_source6(src.encode(), 1, 2, 0, 1, 0, 1, 0, 0, 0 if ev_t is None else N_EV, 0 if ev_t is None else 1,
                                                 d.encode()) == 0
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


def _exact(k, y0, t, ev_t, dose):
    """y(t) (n_ex, n_t): every dose given before t decays from its own time."""
    y = y0[:, None] * np.exp(-k * t)
    if ev_t is not None:
        for j in range(ev_t.shape[1]):
            y = y + np.where(t > ev_t[:, j:j + 1], dose[:, j:j + 1] * np.exp(-k * (t - ev_t[:, j:j + 1])), 0.0)
    return y


def bench(n, rounds):
    rs = np.random.RandomState(0)
    t = np.tile(np.linspace(0.0, T_END, 20), (N_EX, 1))
    y0 = np.array([1.0, 0.5, 2.0, 0.8])
    th_true = np.array([0.6, 0.05])
    noise = th_true[1] * rs.standard_normal(t.shape)
    th = th_true + np.array([0.01, 0.002]) * rs.standard_normal((n, 2))      # posterior-like
    engines = []
    try:
        for name, src, ev_t in VARIANTS:
            eng = pkg.HipEngine(n, 2, device=0)
            engines.append(eng)
            eng.set_prior({f"p{j}": {"dist": "uniform", "low": 0, "high": 10} for j in range(2)})
            fires = ev_t is not None and not np.all(np.isnan(ev_t))
            obs = (_exact(th_true[0], y0, t, ev_t if fires else None, DOSE) + noise)[:, :, None]
            events = None if ev_t is None else {"t": ev_t, "values": DOSE[:, :, None]}
            eng.set_model_user(src, 1, t, obs, cond=y0[:, None], events=events)
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
        for (name, _, _), m, i in zip(VARIANTS, ms, info):
            print(json.dumps({"kernel": name, "particles": n, "experiments": N_EX, "solve_ms_median": round(float(np.median(m)), 4),
                              "solve_ms_min": round(min(m), 4), "solve_ms_max": round(max(m), 4), "solve_ms_all": [round(x, 4) for x in m],
                              "rk_attempts": i["rk_attempts"], "n_failed": i["n_failed"]}), flush=True)
        print(json.dumps({"ratio_to_no_events": {name: round(med[j] / med[0], 4) for j, (name, _, _) in enumerate(VARIANTS)},
                          "spread_max_over_min": {name: round(max(ms[j]) / min(ms[j]), 4) for j, (name, _, _) in enumerate(VARIANTS)}}), flush=True)
    finally:
        for eng in engines:
            eng.close()


if __name__ == "__main__":
    if "--census" in sys.argv:
        census()
    else:
        args = [x for x in sys.argv[1:] if not x.startswith("-")]
        bench(int(args[0]) if args else 65_536, int(args[1]) if len(args) > 1 else 9)
