"""One description of a user model behind the numbered entry points (include/smc_hip.h: smc_user_source_spec, smc_user_model_spec).

CPU: smc_user_model_dump_source_spec writes, and smc_user_model_check_spec returns, what the numbered function of each case of
tools/user_source_equiv.py does; the refusals of check5 / 6 / 7; struct_size (a truncated struct reads as the feature being
absent, a size the library does not know is refused); the ctypes structures against the library's own offsets; the exports.
GPU (64 particles, the experiments of the case modules): every path of the dispatch set once through its numbered function and
once through smc_set_model_user_spec gives the same bits; every refusal gives the same words, which are literals here."""
import ctypes
import filecmp
import importlib.util
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import censored_chain as CC
import dosed_model as DM
import forced_linear_model as FM
import linear_chain_model as LC
import noise_model_chain as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RK45, BDF = 0, 1
N = 64

SOURCE_FIELDS = ("struct_size", "source", "n_states", "dim", "method", "n_obs", "noise", "n_cond", "n_in", "n_knot", "n_ev", "n_val",
                 "censor")
MODEL_FIELDS = ("struct_size", "source", "n_states", "method", "n_obs", "t", "obs", "cond", "obs_scale", "n_ex", "n_t", "n_cond",
                "est_sigma", "sigma_fixed", "add_index", "add_fixed", "prop_index", "prop_fixed", "rtol", "atol", "in_t", "in_u", "n_in",
                "n_knot", "ev_t", "ev_v", "n_ev", "n_val", "censor")


@pytest.fixture(scope="module")
def equiv():
    spec = importlib.util.spec_from_file_location("_user_source_equiv", os.path.join(ROOT, "tools", "user_source_equiv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _matrix(equiv, pkg):
    """The tool's cases, one with events (n_ev = 5, n_val = 2) and one with censor = 1; the two ride on the key "n_val" / a
    nonzero "censor", which the tool's own dump() passes on or ignores as the numbered function of the case does."""
    c = DM.CASES["E2"]
    ev = ("E2.rk45.nobs2.ev5", c["source"], c["ns"], RK45, c["n_obs"],
          {"dim": c["dim"], "noise": 0, "n_cond": c["n_cond"], "n_in": 0, "n_knot": 0, "n_ev": 5, "n_val": 2})
    cen = ("CONSECUTIVE_REACTIONS_AB.rk45.nobs2.prop.cens", pkg.user_models.CONSECUTIVE_REACTIONS_AB, 2, RK45, 2,
           {"dim": 5, "noise": 2, "censor": 1})
    return equiv.cases() + [ev, cen]


def _numbered_dump(L, equiv, case, d):
    """The numbered function the case uses today (the tool's dump), n_val included for the events variant."""
    _, source, ns, method, n_obs, how = case
    if how is not None and how.get("n_val"):
        os.makedirs(d)
        return L.smc_user_model_dump_source6(source.encode(), ns, how["dim"], method, n_obs, how["noise"], how["n_cond"], how["n_in"],
                                             how["n_knot"], how["n_ev"], how["n_val"], d.encode())
    equiv.dump(L, case, d)
    return 0


def _numbered_check(L, case, log, cap):
    _, source, ns, method, n_obs, how = case
    src = source.encode()
    if how is not None and "censor" in how:
        return L.smc_user_model_check7(src, ns, how["dim"], method, n_obs, how["noise"], 0, 0, 0, 0, 0, how["censor"], log, cap)
    if how is not None and "n_ev" in how:
        return L.smc_user_model_check6(src, ns, how["dim"], method, n_obs, how["noise"], how["n_cond"], how["n_in"], how["n_knot"],
                                       how["n_ev"], how.get("n_val", 0), log, cap)
    if how is not None and "n_in" in how:
        return L.smc_user_model_check5(src, ns, how["dim"], method, n_obs, how["noise"], how["n_cond"], how["n_in"], how["n_knot"], log, cap)
    if how is not None:
        return L.smc_user_model_check4(src, ns, how["dim"], method, n_obs, int(how["noise"] > 1), log, cap)
    if n_obs is None:
        return L.smc_user_model_check2(src, ns, 3, method, log, cap)
    return L.smc_user_model_check3(src, ns, 3, method, n_obs, log, cap)


def _source_spec(pkg, case):
    _, source, ns, method, n_obs, how = case
    how = how or {}
    return pkg.binding.UserSourceSpec(source=source.encode(), n_states=ns, dim=how.get("dim", 3), method=method, n_obs=n_obs or 0,
                                      noise=how.get("noise", 0), n_cond=how.get("n_cond", 0), n_in=how.get("n_in", 0),
                                      n_knot=how.get("n_knot", 0), n_ev=how.get("n_ev", 0), n_val=how.get("n_val", 0),
                                      censor=how.get("censor", 0))


def _same_files(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    return fa == fb and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in fa)


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_dump_source_spec_writes_the_numbered_functions_files_for_every_case(pkg, equiv, tmp_path):
    L = pkg.lib()
    cases = _matrix(equiv, pkg)
    assert len(cases) >= 42 and len({c[0] for c in cases}) == len(cases)
    for case in cases:
        dn, ds = tmp_path / case[0] / "numbered", tmp_path / case[0] / "spec"
        assert _numbered_dump(L, equiv, case, str(dn)) == 0, case[0]
        ds.mkdir()
        assert L.smc_user_model_dump_source_spec(ctypes.byref(_source_spec(pkg, case)), str(ds).encode()) == 0, case[0]
        assert _same_files(str(dn), str(ds)), case[0]
        assert "smc_user_model.hip" in os.listdir(ds) and len(os.listdir(ds)) >= 7
    with_events = tmp_path / "E2.rk45.nobs2.ev5" / "spec"
    assert "user_event.h" in os.listdir(with_events) and "#define SMC_USER_NVAL 2\n" in (with_events / "smc_user_model.hip").read_text()
    assert "user_censor.h" in os.listdir(tmp_path / "CONSECUTIVE_REACTIONS_AB.rk45.nobs2.prop.cens" / "spec")


def test_check_spec_returns_the_numbered_checks_code_for_every_case(pkg, equiv):
    L = pkg.lib()

    def both(case):
        log_n, log_s = ctypes.create_string_buffer(16384), ctypes.create_string_buffer(16384)
        return (_numbered_check(L, case, log_n, 16384), L.smc_user_model_check_spec(ctypes.byref(_source_spec(pkg, case)), log_s, 16384),
                log_s.value)

    cases = _matrix(equiv, pkg)
    broken = ("broken", "__device__ void smc_user_y0(", 1, RK45, None, None)      # a compile error is the same code 1 as well
    with ThreadPoolExecutor(min(8, len(os.sched_getaffinity(0)))) as ex:
        got = list(ex.map(both, cases + [broken]))
    for case, (rc_n, rc_s, log) in zip(cases, got):
        assert rc_n == rc_s == 0, (case[0], rc_n, rc_s, log[-2000:])
    assert got[-1][0] == got[-1][1] == 1 and got[-1][2]


def _ab_spec(pkg, **more):
    f = dict(source=pkg.user_models.CONSECUTIVE_REACTIONS_AB.encode(), n_states=2, dim=5, method=RK45, n_obs=2, noise=1, n_cond=1)
    f.update(more)
    return pkg.binding.UserSourceSpec(**f)


REFUSED = [("n_in", dict(n_in=9, n_knot=4)), ("n_knot", dict(n_in=1, n_knot=4097)), ("n_knot_0", dict(n_in=1, n_knot=0)),
           ("n_ev", dict(n_ev=257, n_val=1)), ("n_val", dict(n_ev=1, n_val=9)), ("censor_without_noise", dict(censor=1, noise=0)),
           ("n_obs", dict(n_obs=9)), ("method", dict(method=2)), ("noise", dict(noise=3)), ("source", dict(source=None))]


@pytest.mark.parametrize("name,fields", REFUSED, ids=[r[0] for r in REFUSED])
def test_check_spec_and_dump_source_spec_refuse_what_the_numbered_functions_refuse(pkg, tmp_path, name, fields):
    L = pkg.lib()
    s = _ab_spec(pkg, **fields)
    log = ctypes.create_string_buffer(256)
    args = (s.source, s.n_states, s.dim, s.method, s.n_obs, s.noise, s.n_cond, s.n_in, s.n_knot, s.n_ev, s.n_val, s.censor)
    assert L.smc_user_model_check7(*args, log, 256) == 2 and L.smc_user_model_dump_source7(*args, str(tmp_path).encode()) == 2
    assert L.smc_user_model_check_spec(ctypes.byref(s), log, 256) == 2
    assert L.smc_user_model_dump_source_spec(ctypes.byref(s), str(tmp_path).encode()) == 2
    assert os.listdir(tmp_path) == []


def test_a_null_dir_a_null_spec_and_features_on_the_one_output_source_are_refused(pkg, tmp_path):
    L = pkg.lib()
    assert L.smc_user_model_dump_source_spec(ctypes.byref(_ab_spec(pkg)), None) == 2
    assert L.smc_user_model_dump_source7(_ab_spec(pkg).source, 2, 5, RK45, 2, 1, 1, 0, 0, 0, 0, 0, None) == 2
    assert L.smc_user_model_dump_source_spec(None, str(tmp_path).encode()) == 2 and L.smc_user_model_check_spec(None, None, 0) == 2
    for more in (dict(noise=1), dict(noise=0, n_in=1, n_knot=4), dict(noise=0, n_ev=2), dict(noise=1, censor=1)):
        assert L.smc_user_model_check_spec(ctypes.byref(_ab_spec(pkg, n_obs=0, **{"noise": 0, **more})), None, 0) == 2, more
    assert L.smc_user_model_dump_source_spec(ctypes.byref(_ab_spec(pkg)), str(tmp_path).encode()) == 0      # the spec itself is sound


def test_a_truncated_source_spec_reads_as_the_feature_being_absent(pkg, tmp_path):
    L = pkg.lib()
    S = pkg.binding.UserSourceSpec
    src = DM.CASES["E2"]["source"].encode()
    plain = DM.PLAIN["E2"].encode()
    dirs = {k: tmp_path / k for k in ("cut_censor", "six", "cut_events", "five", "whole")}
    for d in dirs.values():
        d.mkdir()
    enc = lambda k: str(dirs[k]).encode()
    # everything set; struct_size ends just before censor: censor = 0, dump_source6's files
    s = S(source=src, n_states=2, dim=4, method=RK45, n_obs=2, noise=1, n_cond=1, n_ev=5, n_val=2, censor=1)
    assert L.smc_user_model_dump_source_spec(ctypes.byref(s), enc("whole")) == 0 and "user_censor.h" in os.listdir(dirs["whole"])
    s.struct_size = S.censor.offset
    assert L.smc_user_model_dump_source_spec(ctypes.byref(s), enc("cut_censor")) == 0
    assert L.smc_user_model_dump_source6(src, 2, 4, RK45, 2, 1, 1, 0, 0, 5, 2, enc("six")) == 0
    assert _same_files(dirs["cut_censor"], dirs["six"]) and "user_censor.h" not in os.listdir(dirs["six"])
    # ... just before n_ev: no events either, dump_source5's files (the source without smc_user_event)
    s = S(source=plain, n_states=2, dim=4, method=RK45, n_obs=2, noise=1, n_cond=1, n_ev=5, n_val=2, censor=1)
    s.struct_size = S.n_ev.offset
    assert L.smc_user_model_dump_source_spec(ctypes.byref(s), enc("cut_events")) == 0
    assert L.smc_user_model_dump_source5(plain, 2, 4, RK45, 2, 1, 1, 0, 0, enc("five")) == 0
    assert _same_files(dirs["cut_events"], dirs["five"]) and "user_event.h" not in os.listdir(dirs["five"])
    # the smallest struct the library takes ends behind n_obs; sizes it cannot know are refused
    s.struct_size = S.noise.offset
    assert L.smc_user_model_check_spec(ctypes.byref(s), None, 0) == 0
    for size in (0, S.noise.offset - 1, ctypes.sizeof(S) + 8):
        s.struct_size = size
        assert L.smc_user_model_check_spec(ctypes.byref(s), None, 0) == 2, size
        assert L.smc_user_model_dump_source_spec(ctypes.byref(s), enc("whole")) == 2, size


@pytest.mark.parametrize("which,cls,names", [(0, "UserSourceSpec", SOURCE_FIELDS), (1, "UserModelSpec", MODEL_FIELDS)])
def test_the_ctypes_structures_have_the_librarys_layout(pkg, which, cls, names):
    S = getattr(pkg.binding, cls)
    assert tuple(f[0] for f in S._fields_) == names
    off = (ctypes.c_int * 64)(*([-1] * 64))
    assert pkg.lib().smc_user_spec_layout(which, off, 64) == ctypes.sizeof(S)
    assert list(off[:len(names)]) == [getattr(S, nm).offset for nm in names] and off[len(names)] == -1
    assert pkg.lib().smc_user_spec_layout(which, off, 2) == ctypes.sizeof(S) and pkg.lib().smc_user_spec_layout(2, off, 64) == -1
    assert S().struct_size == ctypes.sizeof(S)


def test_the_new_names_are_declared_bound_and_exported_beside_the_numbered_ones(pkg):
    new = ["smc_set_model_user_spec", "smc_user_model_check_spec", "smc_user_model_dump_source_spec", "smc_user_spec_layout"]
    numbered = [f"{stem}{k}" for stem in ("smc_set_model_user", "smc_user_model_check", "smc_user_model_dump_source")
                for k in ("", 2, 3, 4, 5, 6, 7)]
    assert len(numbered) == 21
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    declared = set(pkg.header_symbols())
    for name in new + numbered:
        assert name in declared and name in pkg.binding.SIGNATURES and name in exported, name
    assert pkg.lib().smc_abi_version() == 3


# ---- GPU -----------------------------------------------------------------------------------------------------------

NUMBERED_ARGS = {2: ("source", "n_states", "t", "obs", "cond", "n_ex", "n_t", "n_cond", "est_sigma", "sigma_fixed", "rtol", "atol", "method"),
                 3: ("source", "n_states", "n_obs", "t", "obs", "cond", "obs_scale", "n_ex", "n_t", "n_cond", "est_sigma", "sigma_fixed",
                     "rtol", "atol", "method"),
                 4: ("source", "n_states", "n_obs", "t", "obs", "cond", "obs_scale", "n_ex", "n_t", "n_cond", "add_index", "add_fixed",
                     "prop_index", "prop_fixed", "rtol", "atol", "method")}
NUMBERED_ARGS[5] = NUMBERED_ARGS[4] + ("est_sigma", "sigma_fixed", "in_t", "in_u", "n_in", "n_knot")
NUMBERED_ARGS[6] = NUMBERED_ARGS[5] + ("ev_t", "ev_v", "n_ev", "n_val")
NUMBERED_ARGS[7] = NUMBERED_ARGS[6] + ("censor",)
POINTERS = {"t": np.float64, "obs": np.float64, "cond": np.float64, "obs_scale": np.float64, "add_fixed": np.float64,
            "prop_fixed": np.float64, "in_t": np.float64, "in_u": np.float64, "ev_t": np.float64, "ev_v": np.float64,
            "add_index": np.int32, "prop_index": np.int32, "censor": np.int8}
CTYPES = {np.float64: ctypes.c_double, np.int32: ctypes.c_int, np.int8: ctypes.c_int8}


class Model:
    """The fields of a smc_user_model_spec as NumPy arrays and numbers (what is not given is absent); the same arrays go to the
    numbered function and to the struct."""

    def __init__(self, pkg, dim, source, n_states, t, obs, cond, method="RK45", rtol=1e-3, atol=1e-6, est_sigma=True, sigma_fixed=5.0,
                 obs_scale=None, noise=None, inputs=None, events=None, censor=None, one_output=False):
        t = np.ascontiguousarray(t, dtype=np.float64)
        obs = np.asarray(obs, dtype=np.float64)
        if not one_output and obs.ndim == 2:
            obs = obs[:, :, None]
        cond = np.asarray(cond, dtype=np.float64).reshape(t.shape[0], -1)
        self.n_obs = 0 if one_output else obs.shape[2]
        f = dict(source=source.encode(), n_states=n_states, method=pkg.binding.USER_METHODS[method], n_obs=self.n_obs, t=t, obs=obs,
                 cond=cond, obs_scale=obs_scale, n_ex=t.shape[0], n_t=t.shape[1], n_cond=cond.shape[1], est_sigma=int(est_sigma),
                 sigma_fixed=float(sigma_fixed), rtol=float(rtol), atol=float(atol), n_in=0, n_knot=0, n_ev=0, n_val=0)
        if noise is not None:
            f["add_index"], f["add_fixed"], f["prop_index"], f["prop_fixed"] = pkg.user_models.noise_layout(noise, obs.shape[2], dim)
        if inputs is not None:
            u = np.asarray(inputs["u"], dtype=np.float64)
            u = u[:, :, None] if u.ndim == 2 else u
            f.update(in_t=inputs["t"], in_u=u, n_in=u.shape[2], n_knot=u.shape[1])
        if events is not None:
            v = events["values"]
            v = None if v is None else np.asarray(v, dtype=np.float64)
            f.update(ev_t=events["t"], ev_v=v, n_ev=np.shape(events["t"])[1], n_val=0 if v is None else v.shape[2])
        f["censor"] = censor
        for name, dtype in POINTERS.items():
            f[name] = None if f.get(name) is None else np.ascontiguousarray(f[name], dtype=dtype)
        self.f = f
        self.shape = (t.shape[0], t.shape[1], max(self.n_obs, 1))

    def but(self, **fields):
        """A copy with some fields replaced (arrays as they are, None for a NULL pointer)."""
        m = object.__new__(Model)
        m.n_obs, m.shape, m.f = self.n_obs, self.shape, dict(self.f)
        for name, v in fields.items():
            m.f[name] = np.ascontiguousarray(v, dtype=POINTERS[name]) if name in POINTERS and v is not None else v
        return m

    def _c(self, name):
        v = self.f[name]
        if name in POINTERS:
            return None if v is None else v.ctypes.data_as(ctypes.POINTER(CTYPES[POINTERS[name]]))
        return v

    def set_numbered(self, eng, k):
        args = [self._c(nm) for nm in NUMBERED_ARGS[k]]
        return getattr(eng.L, f"smc_set_model_user{k}")(eng.ctx, *args)

    def set_spec(self, pkg, eng, struct_size=None):
        spec = pkg.binding.UserModelSpec(**{nm: self._c(nm) for nm in MODEL_FIELDS[1:]})
        if struct_size is not None:
            spec.struct_size = struct_size
        return eng.L.smc_set_model_user_spec(eng.ctx, ctypes.byref(spec))


def _run(pkg, eng, m, th):
    """Everything a model computes for the particles th: lk and the counters of a sweep, the BDF totals (or their refusal) and,
    for a multi-output model, smc_user_predict's lk, predictions and counters."""
    eng.upload_particles(pkg.SMC_SET_PRED, th)
    info = eng.loglik(pkg.SMC_SET_PRED)
    out = {"lk": eng.download_lk(pkg.SMC_SET_PRED), "info": info}
    totals = (ctypes.c_int64 * 4)()
    out["bdf"] = (eng.L.smc_user_sweep_counters(eng.ctx, totals), tuple(totals))
    if m.n_obs > 0:
        lk, pred = np.empty(len(th)), np.full((len(th),) + m.shape, np.nan)
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert eng.L.smc_user_predict(eng.ctx, dp(np.ascontiguousarray(th)), len(th), dp(lk), dp(pred), ctypes.byref(nf), ctypes.byref(att)) == 0
        out["predict"] = (lk, pred, nf.value, att.value)
    return out


def _assert_same(a, b, what):
    assert np.array_equal(a["lk"], b["lk"], equal_nan=True), what
    assert a["info"] == b["info"] and a["bdf"] == b["bdf"], (what, a["info"], b["info"], a["bdf"], b["bdf"])
    assert ("predict" in a) == ("predict" in b)
    if "predict" in a:
        assert np.array_equal(a["predict"][0], b["predict"][0], equal_nan=True), what
        assert np.array_equal(a["predict"][1], b["predict"][1], equal_nan=True) and a["predict"][2:] == b["predict"][2:], what


def _chain_population(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([NC.K_TRUE[0] * (1 + 0.1 * rs.standard_normal(n)), NC.K_TRUE[1] * (1 + 0.1 * rs.standard_normal(n)),
                            rs.uniform(0.005, 0.03, n), rs.uniform(0.01, 0.05, n), rs.uniform(0.02, 0.2, n)])


def _paths(pkg):
    """name -> (dim, population, model, its numbered function, the model whose bits it must also give or None)"""
    um = pkg.user_models
    AB = um.CONSECUTIVE_REACTIONS_AB
    t, obs = NC.make_data(0)
    th5 = _chain_population(N, 3)
    chain = dict(dim=5, source=AB, n_states=2, t=t, obs=obs, cond=NC.A0[:, None])
    out = {}
    c = LC.CASES["R1"]
    t1, obs1, cond1 = LC.make_data("R1")
    out["one_output_rk45"] = (c["dim"], LC.population("R1")[:N], Model(pkg, c["dim"], LC.case_source("R1"), c["ns"], t1, obs1, cond1,
                                                                       one_output=True, **{k: v for k, v in LC.model_kwargs("R1").items() if k != "cond"}), 2, None)
    out["sigma_rule_bdf_obs_scale"] = (5, th5, Model(pkg, method="BDF", obs_scale=(1.0, 3.0), **chain), 3, None)
    out["noise_proportional"] = (5, th5, Model(pkg, noise=NC.NOISE, obs_scale=(1.0, 3.0), **chain), 4, None)
    out["noise_degenerate"] = (5, th5, Model(pkg, noise={"additive": [("param", 4), ("param", 4)]}, **chain), 4, Model(pkg, **chain))
    c = FM.CASES["F1"]
    tf, obsf, _ = FM.make_data("F1")
    out["inputs"] = (c["dim"], FM.population("F1")[:N], Model(pkg, c["dim"], c["source"], c["ns"], tf, obsf, **FM.model_kwargs("F1")), 5, None)
    c = DM.CASES["E4"]
    td, obsd, _ = DM.make_data("E4")
    out["events_with_inputs"] = (c["dim"], DM.population("E4")[:N], Model(pkg, c["dim"], c["source"], c["ns"], td, obsd, **DM.model_kwargs("E4")), 6, None)
    _, _, lower, upper = CC.two_sided(0)
    o, cen = um.censor_data(np.where(np.isnan(t)[:, :, None], np.nan, obs), lower, upper)
    out["censored_sigma_rule"] = (5, th5, Model(pkg, censor=cen, **{**chain, "obs": o}), 7, None)
    c = DM.CASES["E2"]
    td, values, _ = DM.make_data("E2")
    o2, cen2 = um.censor_data(values, lower=np.nanquantile(values, 0.3, axis=(0, 1)))
    out["censored_noise_events"] = (c["dim"], DM.population("E2")[:N],
                                    Model(pkg, c["dim"], c["source"], c["ns"], td, o2, censor=cen2,
                                          noise={"additive": [("param", 3), ("fixed", 0.05)], "proportional": [("fixed", 0.1), ("param", 3)]},
                                          **DM.model_kwargs("E2")), 7, None)
    return out


PATHS = ("one_output_rk45", "sigma_rule_bdf_obs_scale", "noise_proportional", "noise_degenerate", "inputs", "events_with_inputs",
         "censored_sigma_rule", "censored_noise_events")


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_the_numbered_function_and_the_spec_give_the_same_bits(pkg, path):
    dim, th, m, k, twin = _paths(pkg)[path]
    assert th.shape == (N, dim) and (m.f["censor"] is None or np.any(m.f["censor"] != 0))
    with pkg.HipEngine(N, dim, device=0) as eng:
        assert m.set_numbered(eng, k) == 0, eng.L.smc_last_error(eng.ctx)
        a = _run(pkg, eng, m, th)
        assert m.set_spec(pkg, eng) == 0, eng.L.smc_last_error(eng.ctx)
        b = _run(pkg, eng, m, th)
        if 2 < k < 7:      # ... and through the newest numbered function, whose absent features take the same path
            assert m.set_numbered(eng, 7) == 0, eng.L.smc_last_error(eng.ctx)
            _assert_same(a, _run(pkg, eng, m, th), f"{path}: smc_set_model_user7")
        if twin is not None:      # the degenerate specification lands on the sigma rule's path: smc_set_model_user3's bits
            assert twin.set_numbered(eng, 3) == 0, eng.L.smc_last_error(eng.ctx)
            _assert_same(a, _run(pkg, eng, twin, th), f"{path}: smc_set_model_user3")
    _assert_same(a, b, path)
    assert a["info"]["rk_attempts"] > 0 and np.isfinite(a["lk"]).mean() > 0.9
    assert a["bdf"][0] == (0 if m.f["method"] == BDF else 1) and (m.f["method"] != BDF or a["bdf"][1][0] > 0)


LDS_4 = ("data set too large for the kernel's LDS table ((8 + 2 n_ex + n_ex (n_t + 1) (n_obs + 2 rounded down to even) + 40 + 8 n_ex) x 8 B + "
         "pools): 154368 B needed, 153600 B available")
LDS_7 = ("data set too large for the kernel's LDS table with the flags of censored observations ((8 + 2 n_ex + n_ex (n_t + 1) (n_obs + 3 "
         "rounded down to even) + 40 + 8 n_ex) x 8 B + pools): 155776 B needed, 153600 B available")


def _refusals(pkg):
    """(what, model, numbered function or None, its whole message or None, the message of the spec entry after its prefix)"""
    um = pkg.user_models
    t, obs = NC.make_data(0)
    n_ex, n_t = t.shape
    base = Model(pkg, 5, um.CONSECUTIVE_REACTIONS_AB, 2, t, obs, NC.A0[:, None])
    knots = np.tile(np.array([0.0, 4.0, 9.0]), (n_ex, 1))
    u = np.ones((n_ex, 3, 1))
    ev_t = np.tile(np.array([2.0, 5.0]), (n_ex, 1))
    ev_v = np.ones((n_ex, 2, 1))
    with_in = base.but(in_t=knots, in_u=u, n_in=1, n_knot=3)
    with_ev = base.but(ev_t=ev_t, ev_v=ev_v, n_ev=2, n_val=1)
    ev_early = ev_t.copy()
    ev_early[:, 0] = t[:, 0]
    flag, obs_nan = np.zeros(obs.shape, dtype=np.int8), obs.copy()
    e, i = 0, 3
    assert np.isfinite(t[e, i])
    flag[e, i, 1], obs_nan[e, i, 1] = -1, np.nan
    good = np.zeros(obs.shape, dtype=np.int8)
    good[tuple(np.argwhere(np.isfinite(obs[:, :, 0]) & ~np.isnan(t))[0]) + (0,)] = 1
    ai, af = np.array([2, 3]), np.zeros(2)
    in_rule, ev_rule = "n_in = 0 with in_t or in_u given (both must be NULL)", "n_ev = 0 with ev_t or ev_v given (both must be NULL)"
    add_rule = "add_index is NULL (the sigma rule) and another part of a noise model is given"
    big4 = Model(pkg, 5, um.CONSECUTIVE_REACTIONS_AB, 2, np.tile(np.linspace(0.0, 10.0, 518), (8, 1)), np.zeros((8, 518, 2)), np.ones((8, 1)),
                 noise={"additive": NC.NOISE["additive"]})
    cen7 = np.zeros((4, 700, 3), dtype=np.int8)
    cen7[1, 5, 2] = -1
    big7 = Model(pkg, 5, um.CONSECUTIVE_REACTIONS_ABC, 2, np.tile(np.linspace(0.0, 10.0, 700), (4, 1)), np.zeros((4, 700, 3)), np.ones((4, 1)),
                 noise={"additive": [("param", 2), ("param", 3), ("param", 3)]}, censor=cen7)
    t_bad = t.copy()
    t_bad[0, 2] = t_bad[0, 1]
    return [
        ("n_in = 0 with in_t, from 5", base.but(in_t=knots), 5, "smc_set_model_user5: " + in_rule, in_rule),
        ("n_in = 0 with in_u, from 6 with events", with_ev.but(in_u=u), 6, "smc_set_model_user6: " + in_rule, in_rule),
        ("n_in = 0 with in_t, from 7 with a flag", base.but(in_t=knots, censor=good), 7, "smc_set_model_user7: " + in_rule, in_rule),
        ("n_ev = 0 with ev_t, from 6", base.but(ev_t=ev_t), 6, "smc_set_model_user6: " + ev_rule, ev_rule),
        ("n_ev = 0 with ev_v, from 7", with_in.but(ev_v=ev_v), 7, "smc_set_model_user6: " + ev_rule, ev_rule),
        ("add_index NULL with prop_index, from 5", base.but(prop_index=ai), 5, "smc_set_model_user5: " + add_rule, add_rule),
        ("add_index NULL with add_fixed, from 7 with events", with_ev.but(add_fixed=af), 7, "smc_set_model_user6: " + add_rule, add_rule),
        ("smc_set_model_user4 without add_index", base, 4, "smc_set_model_user4: NULL add_index or add_fixed (one entry per output)", None),
        ("add_index outside [0, dim), from 4", base.but(add_index=np.array([5, 3]), add_fixed=af), 4,
         "smc_set_model_user4: output 0: add_index outside [0, dim) (-1 selects add_fixed)", "output 0: add_index outside [0, dim) (-1 selects add_fixed)"),
        ("prop_fixed without prop_index, from 5 with inputs", with_in.but(add_index=ai, add_fixed=af, prop_fixed=af), 5,
         "smc_set_model_user5: prop_index and prop_fixed must both be given or both be NULL", "prop_index and prop_fixed must both be given or both be NULL"),
        ("a flag on a NaN value", base.but(obs=obs_nan, censor=flag), 7,
         f"smc_set_model_user7: censor flags a value that was not measured (obs is NaN) at row {e}, time {i}, output 1",
         f"smc_set_model_user7: censor flags a value that was not measured (obs is NaN) at row {e}, time {i}, output 1"),
        ("sigma_fixed = 0 under censoring", base.but(censor=good, est_sigma=0, sigma_fixed=0.0), 7,
         "smc_set_model_user7: sigma_fixed must be finite and > 0", "sigma_fixed must be finite and > 0"),
        ("an input layout error, from 7", with_in.but(in_t=knots[:, ::-1]), 7,
         "smc_set_model_user5: row 0 of in_t is not strictly increasing at knot 1", "smc_set_model_user5: row 0 of in_t is not strictly increasing at knot 1"),
        ("an event layout error, from 7", with_ev.but(ev_t=ev_early), 7,
         "smc_set_model_user6: row 0 of ev_t is not later than the row's first time t[e][0] at event 0",
         "smc_set_model_user6: row 0 of ev_t is not later than the row's first time t[e][0] at event 0"),
        ("a data rule, from 3", base.but(t=t_bad), 3, "smc_set_model_user3: row 0 of t is not strictly increasing",
         "smc_set_model_user3: row 0 of t is not strictly increasing"),
        ("n_obs = 9, from 3", base.but(n_obs=9), 3, "smc_set_model_user3: n_obs out of range (1 .. SMC_USER_MAX_OBS)",
         "smc_set_model_user3: n_obs out of range (1 .. SMC_USER_MAX_OBS)"),
        ("an unknown method, from 2", base.but(method=2, n_obs=0, obs=obs[:, :, 0]), 2,
         "smc_set_model_user: unknown method (SMC_USER_METHOD_RK45 or SMC_USER_METHOD_BDF)",
         "smc_set_model_user: unknown method (SMC_USER_METHOD_RK45 or SMC_USER_METHOD_BDF)"),
        ("the noise block that does not fit", big4, 4, "smc_set_model_user4: " + LDS_4, "smc_set_model_user4: " + LDS_4),
        ("the flags that do not fit", big7, 7, "smc_set_model_user7: " + LDS_7, "smc_set_model_user7: " + LDS_7),
        ("n_obs = 0 with obs_scale", base.but(n_obs=0, obs_scale=np.ones(2)), None, None,
         "n_obs = 0 (the one-output model) with obs_scale, a noise model, inputs, events or censor given"),
    ]


@pytest.mark.gpu
def test_refusals_come_in_the_same_words_through_both_entries(pkg):
    """Every call fails before anything is compiled.  The literals are the parent's: its source holds them, and its build gave
    them for these calls."""
    spec_name = "smc_set_model_user_spec: "
    with pkg.HipEngine(N, 5, device=0) as eng:
        err = lambda: eng.L.smc_last_error(eng.ctx).decode()
        for what, m, k, numbered, through_spec in _refusals(pkg):
            if k is not None:
                assert m.set_numbered(eng, k) != 0, what
                print(f"{what}: {err()}")
                assert err() == numbered, what
            if through_spec is not None:
                assert m.set_spec(pkg, eng) != 0, what
                assert err() in (spec_name + through_spec, through_spec) and err().endswith(through_spec), (what, err())
                assert err().startswith(spec_name) == (not through_spec.startswith("smc_set_model_user")), (what, err())
        m = _refusals(pkg)[0][1].but(in_t=None)      # a sound model: only struct_size is wrong
        S = pkg.binding.UserModelSpec
        for size in (0, S.in_t.offset - 8, ctypes.sizeof(S) + 8):
            assert m.set_spec(pkg, eng, struct_size=size) != 0 and "struct_size" in err(), size
        # ... and what ends behind atol is a whole model without the later features
        assert m.set_spec(pkg, eng, struct_size=S.in_t.offset) == 0, err()
