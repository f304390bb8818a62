#!/usr/bin/env python3
"""Are the run-time compiled user-model sources of two builds of libsmc_hip.so the same - as text, or as machine code?

    tools/user_source_equiv.py PARENT/libsmc_hip.so CANDIDATE/libsmc_hip.so [--bytes] [--keep DIR] [--only SUBSTRING]

For every case of the matrix below both libraries write what they would hand to hiprtc (smc_user_model_dump_source2 .. 7:
no GPU is touched, so both load into this process).  The matrix: both methods over one-output and multi-output sources, with
and without a cost hint or a Jacobian, under additive and proportional noise, with measured inputs; and the models of
tests/dosed_model.py WITHOUT their scheduled events (the source without smc_user_event, n_ev = 0 - through
smc_user_model_dump_source6 where a library has it, else through dump_source5): a model without events must be compiled from
the text it had before events existed, byte for byte.  The event variants themselves have no counterpart in a parent without
events; tools/user_event_bench.py --census reports their registers.  Likewise the noise models of tests/noise_model_chain.py
WITHOUT censored observations through smc_user_model_dump_source7 (censor = 0) where a library has it, else through
dump_source4: the censored variants have no counterpart in a parent without them (tools/user_censor_bench.py --census).  --bytes: every dumped
file of the candidate must be the parent's byte for byte (an edit that only moves text), and a header only one of the two has
is reported.  Default: both dumps are compiled off line with hiprtc's flags
(hipcc --offload-arch=gfx950 -O3 -ffp-contract=on -fno-fast-math -I <dump> -S --cuda-device-only) and the listings compared
line by line after dropping the `__hip_cuid_<hash>` symbol, which differs between any two compilations: every instruction of
smc_user_solve_kernel, smc_user_predict_kernel and smc_user_cost_scan_kernel, their .amdhsa_ blocks and the metadata
(registers, scratch, LDS) must agree.  One line per case; exit status 1 if any case differs.

Both libraries are asked through the numbered dump functions, not through smc_user_model_dump_source_spec: a parent from before
the spec structs has no such function, and the numbered ones fill the same struct in a library that has it
(tests/test_user_spec.py compares the two entries case by case).

It is a tool, not a test: it needs a second build (the parent revision's), which the test suite has not got.
"""
import argparse
import ctypes
import difflib
import filecmp
import importlib.util
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-fno-fast-math"]      # user_model.hip: compile_user
RK45, BDF = 0, 1      # SMC_USER_METHOD_*
DIM = 3


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    """(label, source, n_states, method, n_obs, how) - n_obs None: the one-output dump (dump_source2), else dump_source3; how, when not
    None, says what dump_source4 / 5 need on top: dim, noise (0 none, 1 additive, 2 with a proportional part) and, for a model with
    inputs, n_cond, n_in, n_knot; "n_ev": 0 asks for dump_source6 with no events, "censor": 0 for dump_source7 without censoring.  The n_obs = 1 multi dumps are what a model of
    smc_set_model_user / 2 compiles at its first smc_user_predict."""
    um = _load(os.path.join(ROOT, "python-based-sequential-monte-carlo-method-with-likelihood-tempering_amd", "user_models.py"), "_um")
    chain8 = _load(os.path.join(ROOT, "tests", "test_user_model.py"), "_tum").CHAIN8
    chain_dim = len(_load(os.path.join(ROOT, "tests", "noise_model_chain.py"), "_nmc").THETA_TRUE)
    forced = _load(os.path.join(ROOT, "tests", "forced_linear_model.py"), "_flm").CASES
    one = [("MICHAELIS_MENTEN", 1, (RK45, BDF)), ("MICHAELIS_MENTEN_PLAIN", 1, (RK45,)), ("CONSECUTIVE_REACTIONS", 2, (RK45, BDF)),
           ("CHAIN8", 8, (RK45,)), ("ROBERTSON", 3, (BDF,)), ("ROBERTSON_NUMJAC", 3, (BDF,))]
    multi = [("MICHAELIS_MENTEN", 1, 1, (RK45,)), ("CONSECUTIVE_REACTIONS", 2, 1, (RK45, BDF)), ("ROBERTSON", 3, 1, (BDF,)),
             ("CONSECUTIVE_REACTIONS_AB", 2, 2, (RK45, BDF)), ("CONSECUTIVE_REACTIONS_ABC", 2, 3, (RK45,)),
             ("ROBERTSON_AC", 3, 2, (BDF, RK45))]
    # noise models (dump_source4): the chain of tests/noise_model_chain.py, and a source with smc_user_cost (and smc_div)
    noisy = [("CONSECUTIVE_REACTIONS_AB", 2, 2, chain_dim, (1, 2)), ("MICHAELIS_MENTEN", 1, 1, DIM, (1,))]
    src = lambda name: chain8 if name == "CHAIN8" else getattr(um, name)
    tag = lambda m: "bdf" if m else "rk45"
    out = []
    for name, ns, methods in one:
        out += [(f"{name}.{tag(m)}.one", src(name), ns, m, None, None) for m in methods]
    for name, ns, n_obs, methods in multi:
        out += [(f"{name}.{tag(m)}.nobs{n_obs}", src(name), ns, m, n_obs, None) for m in methods]
    for name, ns, n_obs, dim, kinds in noisy:
        out += [(f"{name}.{tag(m)}.nobs{n_obs}.{'prop' if k > 1 else 'add'}", src(name), ns, m, n_obs, {"dim": dim, "noise": k})
                for m in (RK45, BDF) for k in kinds]
    # inputs (dump_source5): the sources of tests/forced_linear_model.py with their geometry, each without noise and with the
    # noise kind that differs from its own case's
    for cid, methods, kinds in (("F1", (RK45, BDF), (0, 1)), ("F2", (BDF,), (0,)), ("F3", (RK45, BDF), (0, 2))):
        c = forced[cid]
        out += [(f"{cid}.{tag(m)}.nobs{c['n_obs']}.in{c['n_in']}" + ("", ".add", ".prop")[k], c["source"], c["ns"], m, c["n_obs"],
                 {"dim": c["dim"], "noise": k, "n_cond": c["n_cond"], "n_in": c["n_in"], "n_knot": c["n_knot"]})
                for m in methods for k in kinds]
    # the event models of tests/dosed_model.py without their events (dump_source6 with n_ev = 0, or dump_source5)
    sys.path.insert(0, os.path.join(ROOT, "tests"))      # dosed_model imports forced_linear_model
    dosed = _load(os.path.join(ROOT, "tests", "dosed_model.py"), "_dm")
    for cid, c in dosed.CASES.items():
        m = BDF if c["method"] == "BDF" else RK45
        out.append((f"{cid}.{tag(m)}.nobs{c['n_obs']}.noev", dosed.PLAIN[cid], c["ns"], m, c["n_obs"],
                    {"dim": c["dim"], "noise": 0, "n_cond": c["n_cond"], "n_in": c["n_in"], "n_knot": 5 if c["n_in"] else 0, "n_ev": 0}))
    # the noise models without censored observations (dump_source7 with censor = 0, or dump_source4)
    out += [(f"CONSECUTIVE_REACTIONS_AB.{tag(m)}.nobs2.{'prop' if k > 1 else 'add'}.nocens", um.CONSECUTIVE_REACTIONS_AB, 2, m, 2,
             {"dim": chain_dim, "noise": k, "censor": 0}) for m in (RK45, BDF) for k in (1, 2)]
    return out


def dump(lib, case, d):
    _, source, ns, method, n_obs, how = case
    os.makedirs(d)
    if how is not None and "censor" in how and hasattr(lib, "smc_user_model_dump_source7"):
        rc = lib.smc_user_model_dump_source7(source.encode(), ns, how["dim"], method, n_obs, how["noise"], 0, 0, 0, 0, 0, how["censor"],
                                             d.encode())
    elif how is not None and "n_ev" in how and hasattr(lib, "smc_user_model_dump_source6"):
        rc = lib.smc_user_model_dump_source6(source.encode(), ns, how["dim"], method, n_obs, how["noise"], how["n_cond"], how["n_in"],
                                             how["n_knot"], how["n_ev"], 0, d.encode())
    elif how is not None and "n_in" in how:
        rc = lib.smc_user_model_dump_source5(source.encode(), ns, how["dim"], method, n_obs, how["noise"], how["n_cond"], how["n_in"],
                                             how["n_knot"], d.encode())
    elif how is not None:
        rc = lib.smc_user_model_dump_source4(source.encode(), ns, how["dim"], method, n_obs, int(how["noise"] > 1), d.encode())
    elif n_obs is None:
        rc = lib.smc_user_model_dump_source2(source.encode(), ns, DIM, method, d.encode())
    else:
        rc = lib.smc_user_model_dump_source3(source.encode(), ns, DIM, method, n_obs, d.encode())
    if rc != 0:
        raise RuntimeError(f"{case[0]}: the dump function returned {rc}")


def listing(d):
    s = os.path.join(d, "listing.s")
    r = subprocess.run([HIPCC, *FLAGS, "-I", d, "-S", "--cuda-device-only", "-o", s, os.path.join(d, "smc_user_model.hip")],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{d} does not compile:\n{r.stderr[-3000:]}")
    return [ln for ln in open(s).read().splitlines() if "__hip_cuid_" not in ln]


def compare(case, pa, ca, work, by_bytes):
    """'' when the two dumps of the case agree, else what differs"""
    dp, dc = os.path.join(work, case[0], "parent"), os.path.join(work, case[0], "candidate")
    dump(pa, case, dp)
    dump(ca, case, dc)
    if by_bytes:
        fp, fc = set(os.listdir(dp)), set(os.listdir(dc))
        bad = [f for f in sorted(fp & fc) if not filecmp.cmp(os.path.join(dp, f), os.path.join(dc, f), shallow=False)]
        said = [f"differ: {bad}"] * bool(bad) + [f"only the parent has {sorted(fp - fc)}"] * bool(fp - fc) + \
               [f"only the candidate has {sorted(fc - fp)}"] * bool(fc - fp)
        return "; ".join(said)
    a, b = listing(dp), listing(dc)
    if a == b:
        return ""
    d = list(difflib.unified_diff(a, b, "parent", "candidate", lineterm="", n=2))
    return f"{sum(1 for ln in d if ln[:1] in '+-' and ln[:3] not in ('+++', '---'))} listing lines differ\n" + "\n".join(d[:60])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("candidate")
    ap.add_argument("--bytes", action="store_true", help="compare the dumped files byte for byte instead of the listings")
    ap.add_argument("--keep", metavar="DIR", help="write the dumps and listings there and keep them")
    ap.add_argument("--only", metavar="SUBSTRING", help="only the cases whose label contains it")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compilations at a time")
    args = ap.parse_args()
    pa, ca = ctypes.CDLL(os.path.abspath(args.parent)), ctypes.CDLL(os.path.abspath(args.candidate))
    todo = [c for c in cases() if not args.only or args.only in c[0]]
    tmp = None if args.keep else tempfile.TemporaryDirectory()
    work = args.keep or tmp.name
    with ThreadPoolExecutor(args.j) as ex:
        results = list(ex.map(lambda c: compare(c, pa, ca, work, args.bytes), todo))
    n_bad = 0
    for c, r in zip(todo, results):
        print(f"{c[0]:45s} {'identical' if not r else 'DIFFERENT: ' + r}")
        n_bad += bool(r)
    print(f"{len(todo) - n_bad} of {len(todo)} cases identical ({'bytes' if args.bytes else 'gfx950 listings'})")
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main())
