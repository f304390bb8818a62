"""HipEngine - Python handle on one libsmc_hip.so context (one per process and GPU).

Every method is a thin call through the C ABI (include/smc_hip.h); all arithmetic happens in the
HIP kernels.  NumPy is used only to own the host buffers the reference would own
("Ownership").
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import binding as B
from .binding import SMC_SET_FILT, SMC_SET_PRED, SmcError, check, lib


def _dp(a):
    return a.ctypes.data_as(B.c_dp)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


class _PinnedPool:
    """Page-locked host buffers for downloaded results (include/smc_hip.h: smc_pinned_alloc).  A buffer belongs to the NumPy array
    that views it and returns to the pool when that array (and every view of it) is garbage-collected; the memory is
    process-wide, so such an array stays valid after its engine is closed.  Buffers are reused by size: a run's final 24 + 8 MB
    download costs one DMA transfer each instead of the runtime's staged copy into pageable memory.
    Thread-safe (several engines may run in threads of one process); at most `cap_bytes` of returned buffers are kept - what
    exceeds the cap is unpinned and freed at once (smc_pinned_free), and release() / interpreter exit free the rest."""

    def __init__(self, cap_bytes=1 << 30):
        import threading
        self.free = {}          # nbytes -> [ptr, ...]
        self.pooled = 0         # bytes held in `free`
        self.cap_bytes = int(cap_bytes)
        self.lock = threading.Lock()

    def take(self, nbytes):
        with self.lock:
            lst = self.free.get(nbytes)
            if lst:
                self.pooled -= nbytes
                return lst.pop()
        p = ctypes.c_void_p(0)
        st = lib().smc_pinned_alloc(ctypes.c_size_t(nbytes), ctypes.byref(p))
        if st != 0:
            msg = lib().smc_last_error(None)
            raise SmcError(f"smc_pinned_alloc: {msg.decode() if msg else 'unknown error'}")
        return p.value

    def give(self, ptr, nbytes):
        with self.lock:
            if self.pooled + nbytes <= self.cap_bytes:
                self.free.setdefault(nbytes, []).append(ptr)
                self.pooled += nbytes
                return
        lib().smc_pinned_free(ctypes.c_void_p(ptr))

    def release(self):
        """Unpin and free every buffer the pool holds (buffers still owned by live arrays are not touched)."""
        with self.lock:
            ptrs = [p for lst in self.free.values() for p in lst]
            self.free.clear()
            self.pooled = 0
        for p in ptrs:
            lib().smc_pinned_free(ctypes.c_void_p(p))


_PINNED = _PinnedPool()


def release_pinned_pool():
    """Free the page-locked result buffers that are waiting for reuse (a size sweep would otherwise keep them for the life of the process)."""
    _PINNED.release()


import atexit  # noqa: E402

atexit.register(lambda: _PINNED.release() if B._LIB is not None else None)


class _PinnedOwner:
    """What a pinned result array keeps alive (ndarray.base): gives the buffer back to the pool when the last view is gone."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.nbytes = max(8, int(np.prod(self.shape)) * self.dtype.itemsize)
        self.ptr = _PINNED.take(self.nbytes)
        self.__array_interface__ = {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            _PINNED.give(self.ptr, self.nbytes)
        except Exception:       # interpreter shutdown
            pass


def pinned_empty(shape, dtype=np.float64):
    """np.empty in page-locked host memory (see _PinnedPool)."""
    return np.asarray(_PinnedOwner(shape, dtype))


class HipEngine:
    """Device-resident particle sets p_pred/lk and p_filt/lk1 plus the stages that act on them."""
    pinned_downloads = True     # download_particles / download_lk accept pinned=True (page-locked result arrays)

    def __init__(self, n_local: int, dim: int = 3, device: int = 0, n_global: int | None = None):
        self.L = lib()
        self.n_local = int(n_local)
        self.n_global = int(n_global if n_global is not None else n_local)
        self.dim = int(dim)
        self.device = int(device)
        self.rank, self.world = 0, 1
        ctx = B.c_ctx()
        st = self.L.smc_create(ctypes.byref(ctx), self.device, self.n_local, self.n_global, self.dim)
        if st != 0:
            msg = self.L.smc_last_error(None)
            raise SmcError(f"smc_create: {msg.decode() if msg else 'unknown error'}")
        self.ctx = ctx
        self.model = None
        self.user_n_obs = 1     # outputs per data time of a user model (set_model_user)
        self.user_n_cond = 0    # ... and its numbers per experiment
        self.user_n_in = 0      # ... and its time-varying inputs (set_model_user(inputs=))
        self.user_n_ev = 0      # ... its event capacity and the values per event (set_model_user(events=))
        self.user_n_val = 0
        if "smc_ess_search_global" in B.MISSING:   # A/B build of an older revision (SMC_HIP_LIB): the driver falls back
            self.ess_search_global = None
        self._peer_barrier = None

    # ---- lifetime ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.L.smc_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, st, what):
        check(self.ctx, st, what)

    def synchronize(self):
        self._ck(self.L.smc_synchronize(self.ctx), "smc_synchronize")

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        arch = ctypes.create_string_buffer(256)
        cu = ctypes.c_int(0)
        self._ck(self.L.smc_device_info(self.ctx, name, 256, arch, 256, ctypes.byref(cu)), "smc_device_info")
        return {"name": name.value.decode(), "arch": arch.value.decode(), "cu_count": cu.value}

    # ---- model / prior -------------------------------------------------------------------------
    def set_model_mm(self, t, P_obs, S0, est_sigma=True, sigma_fixed=5.0, rtol=1e-3, atol=1e-6):
        t = _f64(t)
        P_obs = _f64(P_obs, t.shape)
        S0 = _f64(S0, (t.shape[0],))
        self._ck(self.L.smc_set_model_mm(self.ctx, _dp(t), _dp(P_obs), _dp(S0), t.shape[0], t.shape[1],
                                         int(bool(est_sigma)), float(sigma_fixed), float(rtol), float(atol)),
                 "smc_set_model_mm")
        self.model = ("mm", t.shape[0], t.shape[1])

    def set_model_user(self, source: str, n_states: int, t, obs, cond=None, est_sigma=True, sigma_fixed=5.0, rtol=1e-3,
                       atol=1e-6, method="RK45", obs_scale=None, noise=None, inputs=None, events=None, censor=None):
        """A user-written model in place of Micmem_likelihood.py (include/smc_hip.h, smc_user_model_spec): `source`
        defines smc_user_y0 / smc_user_rhs / smc_user_obs as HIP device functions; t, obs: (n_ex, n_t); cond: (n_ex, n_cond)
        per-experiment numbers (e.g. the initial concentration).  method: "RK45" (solve_ivp's default) or "BDF" for a stiff
        model (then the source may also define smc_user_jac).  Raises ValueError for another method and SmcError with the
        compiler log if the source does not compile.
        Several measured outputs, missing data, ragged rows: obs (n_ex, n_t, n_obs) with NaN for a value
        that was not measured, t rows that may end in NaN times, obs_scale (n_obs,) relative noise scales; the source then
        defines smc_user_obs_vec.  A 3-D obs or any obs_scale takes this path (ValueError for data it refuses, see
        user_models.obs_layout); a 2-D obs without obs_scale, noise, inputs, events or
        censoring is the one-output model (n_obs = 0 in the spec) exactly as before.
        A noise model: noise={"additive": [("param", j) | ("fixed", v), ...], "proportional": [...]}, one
        entry per output, "proportional" optional - sd^2 = (a_k s_k)^2 + (b_k f)^2 (user_models.noise_loglik is the likelihood).
        est_sigma and sigma_fixed are then not used; ValueError for a specification that breaks user_models.noise_layout's rules.
        Time-varying measured inputs: inputs={"t": (n_ex, n_knot), "u": (n_ex, n_knot, n_in)} - knot times (a
        row may end in NaN) and the values of n_in inputs at them (2-D for one input); the source reads them as
        smc_input(cond, k, t), linear between knots (user_models.input_value is the definition, input_layout the rules: ValueError
        for inputs that break them).  With obs, obs_scale, noise / est_sigma as above.  inputs=None leaves the model as it is
        without them.
        Scheduled events: events={"t": (n_ex, n_ev), "values": (n_ex, n_ev, n_val) or None} - event times (a
        row may end in NaN, or hold none) and the numbers of every event; the source defines smc_user_event(j, t, y, theta, cond),
        which changes y in place at event j and reads its numbers as smc_event_value(cond, j, k).  The solve is the chain of
        solve_ivp calls between the events (include/smc_hip.h); user_models.event_layout states the rules (ValueError for events
        that break them).  events=None leaves the model as it is without them.
        State-triggered events (a re-dose when a level falls to a threshold, a relay, a tank that overflows) need no
        argument: a source that contains the name smc_user_root defines
            __device__ const int smc_user_root_dir[] = {-1, 0};   // per event function: -1 falling, +1 rising, 0 either; 1 .. 4
            __device__ void smc_user_root(double t, const double *y, const double *theta, const double *cond, double *g);
            __device__ void smc_user_root_event(int k, double t, double *y, const double *theta, const double *cond);
        and its solve is the chain of solve_ivp(events=...) calls with every event terminal: the root of an event function that
        crosses zero in its direction is found on the step's dense output (SciPy's brentq: user_models.brentq), the data times up
        to and including it see the state before the jump, smc_user_root_event changes y in place, and the integrator starts
        afresh from there (user_models.root_chain is the reference; include/smc_hip.h has the rules, among them that a jump which
        leaves the state on a firing surface, or fire number 257 of a solve, fails the solve).  Both functions may call smc_input
        and smc_event_value where the model has them; it combines with everything above and below.
        Censored observations: censor (n_ex, n_t, n_obs) integer flags beside obs - 0: obs is the measured
        value; -1: left-censored, the true value is <= obs, which holds the lower limit; +1: right-censored, >= obs, the upper limit.
        A censored value contributes log Phi(z) (user_models.censored_loglik is the likelihood, censor_layout the rules: ValueError
        for flags that break them, censor_data makes such data).  With a flag set the model takes the noise path; noise=None then
        stands for every output at the last parameter (est_sigma) or fixed at sigma_fixed.  Combines with everything above.
        censor=None or all zeros leaves the model as it is without them.
        Count observations (case counts, colony counts, read counts) need no argument either: a source that contains the name
        smc_user_obs_family defines
            __device__ const int smc_user_obs_family[] = {0, 2, 1};   // per output: 0 Gaussian, 1 Poisson, 2 negative binomial
        For a count output the model output is the MEAN and the variance is mean + (b_k mean)^2, b_k the output's entry of
        noise["proportional"] (negative binomial: a parameter or fixed > 0; Poisson: absent or ("fixed", 0.0)); its additive
        entry must be ("fixed", 1.0) and its obs_scale 1 (they are not used), its finite values non-negative integers, and it
        takes no censor flag.  The model takes the noise path; noise=None stands for the Gaussian outputs at est_sigma /
        sigma_fixed and the counts at fixed 1.  user_models.count_loglik is the likelihood, count_layout the rules (ValueError
        for what breaks them), obs_family reads the list; predictive_summary(noise=True) is refused for such a model, noise="family"
        draws replicated counts and pointwise_summary(count_pit=True) ranks the observed counts among them.  An
        all-zero list, or no such name, leaves the model as it is.  Every feature is a group of fields of one
        smc_user_model_spec, set by smc_set_model_user_spec; an absent feature takes the path, and gives the bits, it always had."""
        if method not in B.USER_METHODS:
            raise ValueError(f"set_model_user: method must be one of {sorted(B.USER_METHODS)}, not {method!r}")
        t = _f64(t)
        obs = np.asarray(obs)
        multi = obs.ndim == 3 or obs_scale is not None or noise is not None or inputs is not None or events is not None
        if multi:
            # several outputs, NaN = not measured, ragged rows; the same checks as the library's
            obs = _f64(obs if obs.ndim == 3 else obs.reshape(obs.shape + (1,)))
            from .user_models import obs_layout
            obs_layout(t, obs, obs_scale)
            n_obs = obs.shape[2]
            scale = None if obs_scale is None else _f64(np.asarray(obs_scale).reshape(-1), (n_obs,))
        else:
            obs = _f64(obs, t.shape)
            n_obs = 1
        cond = np.zeros((t.shape[0], 0)) if cond is None else _f64(np.asarray(cond).reshape(t.shape[0], -1))
        cbuf = np.ascontiguousarray(cond if cond.size else np.zeros((t.shape[0], 1)))
        ai = af = pi = pf = None
        if noise is not None:
            from .user_models import noise_layout
            ai, af, pi, pf = noise_layout(noise, n_obs, self.dim)
        n_in = n_ev = n_val = 0
        in_t = in_u = ev_t = ev_v = None
        if censor is not None:
            from .user_models import censor_layout
            censor = np.asarray(censor)
            if not multi:      # a 2-D obs: the flags of its one output
                obs3 = _f64(obs.reshape(obs.shape + (1,)))
                censor = censor.reshape(censor.shape + (1,)) if censor.ndim == 2 else censor
            censor_layout(t, obs if multi else obs3, censor)
            censor = censor if np.any(censor != 0) else None
        if censor is not None and not multi:
            multi, obs, n_obs, scale = True, obs3, 1, None
        if inputs is not None:
            in_t, in_u, n_in = self._inputs("set_model_user", inputs, t.shape[0])
        if events is not None:
            ev_t, ev_v, n_val = self._events("set_model_user", events, t)
            n_ev = ev_t.shape[1]
        # count outputs: the families come with the source (smc_user_obs_family); the same checks as the library's
        from .user_models import obs_family, count_layout
        family = obs_family(source)
        if family is not None:
            count_layout(t, obs, family, noise, scale if multi else None, censor, bool(est_sigma), self.dim)
        self.user_family = family
        # one description by field name (include/smc_hip.h: smc_user_model_spec); n_obs = 0: the one-output model.  `keep` holds the
        # arrays the struct points to until the call has returned
        keep = []

        def ptr(a, dtype, ctype):
            if a is None:
                return None
            keep.append(np.ascontiguousarray(a, dtype=dtype))
            return keep[-1].ctypes.data_as(ctype)

        spec = B.UserModelSpec(
            source=source.encode(), n_states=int(n_states), method=B.USER_METHODS[method], n_obs=n_obs if multi else 0,
            t=ptr(t, np.float64, B.c_dp), obs=ptr(obs, np.float64, B.c_dp), cond=ptr(cbuf, np.float64, B.c_dp),
            obs_scale=ptr(scale if multi else None, np.float64, B.c_dp), n_ex=t.shape[0], n_t=t.shape[1], n_cond=cond.shape[1],
            est_sigma=int(bool(est_sigma)), sigma_fixed=float(sigma_fixed), add_index=ptr(ai, np.int32, B.c_ip),
            add_fixed=ptr(af, np.float64, B.c_dp), prop_index=ptr(pi, np.int32, B.c_ip), prop_fixed=ptr(pf, np.float64, B.c_dp),
            rtol=float(rtol), atol=float(atol), in_t=ptr(in_t, np.float64, B.c_dp), in_u=ptr(in_u, np.float64, B.c_dp), n_in=n_in,
            n_knot=0 if in_t is None else in_t.shape[1], ev_t=ptr(ev_t, np.float64, B.c_dp), ev_v=ptr(ev_v, np.float64, B.c_dp),
            n_ev=n_ev, n_val=n_val, censor=ptr(censor, np.int8, B.c_i8p))
        self._ck(self.L.smc_set_model_user_spec(self.ctx, ctypes.byref(spec)), "smc_set_model_user_spec")
        self.model = ("user", t.shape[0], t.shape[1])      # the driver indexes this 3-tuple
        self.user_n_obs = n_obs
        self.user_n_cond = cond.shape[1]
        self.user_n_in = n_in
        self.user_n_ev, self.user_n_val = n_ev, n_val

    @staticmethod
    def _events(what, events, t):
        """events = {"t", "values"} checked by user_models.event_layout against the times t: contiguous ev_t (n_ex, n_ev), ev_v
        (n_ex, n_ev, n_val) or None for n_val = 0, n_val."""
        if not isinstance(events, dict) or set(events) != {"t", "values"}:
            raise ValueError(f'{what}: events must be {{"t": (n_ex, n_ev), "values": (n_ex, n_ev, n_val) or None}}')
        from .user_models import event_layout
        ev_t = _f64(events["t"])
        ev_v = None if events["values"] is None else _f64(events["values"])
        if ev_v is not None and ev_v.ndim == 2 and ev_t.ndim == 2:
            ev_v = np.ascontiguousarray(ev_v.reshape(ev_v.shape + (1,)))
        event_layout(t, ev_t, ev_v)
        if ev_v is not None and ev_v.shape[2] == 0:
            ev_v = None
        return ev_t, ev_v, 0 if ev_v is None else ev_v.shape[2]

    @staticmethod
    def _inputs(what, inputs, n_ex):
        """inputs = {"t", "u"} checked by user_models.input_layout: contiguous in_t (n_ex, n_knot), in_u (n_ex, n_knot, n_in), n_in."""
        if not isinstance(inputs, dict) or set(inputs) != {"t", "u"}:
            raise ValueError(f'{what}: inputs must be {{"t": (n_ex, n_knot), "u": (n_ex, n_knot, n_in)}}')
        from .user_models import input_layout
        in_t, in_u = _f64(inputs["t"]), _f64(inputs["u"])
        if in_u.ndim == 2 and in_t.ndim == 2:
            in_u = in_u.reshape(in_u.shape + (1,))
        input_layout(in_t, in_u, n_ex)
        return in_t, np.ascontiguousarray(in_u), in_u.shape[2]

    def set_model_methanation(self, cond, guess, obs, base_params, est_position, est_sigma=True, sigma_fixed=5.0,
                              tf=75.0, rtol=1e-6, atol=1e-6):
        """cond: dict with Ca_in..Ce_in, T_in, T_jacket, u_in, void, reactorlength (the reference's settings arrays,
        methanation_set_conditon.py:141-214) or an (n_data, 10) array; guess (n_data, 357); obs (5, n_data)."""
        if isinstance(cond, dict):
            n_data = int(cond.get("n_data", len(cond["Ca_in"])))
            cols = [np.asarray(cond[k], dtype=np.float64)[:n_data] for k in
                    ("Ca_in", "Cb_in", "Cc_in", "Cd_in", "Ce_in", "T_in", "T_jacket", "u_in", "void")]
            cols.append(np.asarray(cond["reactorlength"], dtype=np.float64)[:n_data] / (51 - 1))
            cond = np.column_stack(cols)
        cond = _f64(cond)
        n_data = cond.shape[0]
        guess = _f64(np.asarray(guess)[:n_data], (n_data, 357))
        obs = _f64(obs, (5, n_data))
        base = _f64(base_params, (9,))
        pos = np.ascontiguousarray(est_position, dtype=np.int32)
        assert pos.shape == (self.dim,)
        self._ck(self.L.smc_set_model_methanation(self.ctx, _dp(cond), _dp(guess), _dp(obs), n_data, _dp(base),
                                                  pos.ctypes.data_as(B.c_ip), int(bool(est_sigma)), float(sigma_fixed),
                                                  float(tf), float(rtol), float(atol)), "smc_set_model_methanation")
        self.model = ("methanation", n_data, 357)

    def set_prior(self, priors: dict):
        """priors: the reference's dict (Micmem_settings.py:55-67), one entry per parameter, in order.  A dict with a lognormal,
        gamma, beta, truncnormal or halfnormal entry (priors.py) goes through smc_set_prior_ex, every other through smc_set_prior
        as before."""
        from . import priors as P
        if P.has_new_kind(priors):
            k, a, b, lo, hi = P.prior_layout(priors)
            self._ck(self.L.smc_set_prior_ex(self.ctx, k.ctypes.data_as(B.c_ip), _dp(a), _dp(b), _dp(lo), _dp(hi), len(k)), "smc_set_prior_ex")
            return
        kinds, a, b = [], [], []
        for name, p in priors.items():
            if p["dist"] == "uniform":
                kinds.append(B.SMC_PRIOR_UNIFORM)
                a.append(p["low"])
                b.append(p["high"])
            elif p["dist"] == "normal":
                kinds.append(B.SMC_PRIOR_NORMAL)
                a.append(p["mu"])
                b.append(p["sigma"])
            elif p["dist"] == "flat":       # drawn like a normal, no factor in the prior density
                kinds.append(B.SMC_PRIOR_FLAT)
                a.append(p["mu"])
                b.append(p["sigma"])
            else:
                raise ValueError(f"Unknown prior: {p['dist']}")
        k = np.array(kinds, dtype=np.int32)
        a = np.array(a, dtype=np.float64)
        b = np.array(b, dtype=np.float64)
        self._ck(self.L.smc_set_prior(self.ctx, k.ctypes.data_as(B.c_ip), _dp(a), _dp(b), len(kinds)), "smc_set_prior")

    def meth_sweep_counters(self):
        """Device-counted work of the last methanation sweep: BDF steps, Newton iterations, factorisations, failed solves."""
        out = (ctypes.c_int64 * 4)()
        self._ck(self.L.smc_meth_sweep_counters(self.ctx, out), "smc_meth_sweep_counters")
        return {"bdf_steps": out[0], "newton_iters": out[1], "factorisations": out[2], "failed_solves": out[3]}

    def user_sweep_counters(self):
        """Device-counted work of the last sweep of a BDF user model: accepted steps, Newton iterations, LU factorisations,
        Jacobian evaluations (step attempts: the sweep's rk_attempts)."""
        out = (ctypes.c_int64 * 4)()
        self._ck(self.L.smc_user_sweep_counters(self.ctx, out), "smc_user_sweep_counters")
        return {"steps": out[0], "newton_iters": out[1], "lu_factorisations": out[2], "jacobian_evals": out[3]}

    def meth_sweep_check(self):
        """Completeness of the last methanation sweep (the library already fails the sweep when these disagree)."""
        out = (ctypes.c_int64 * 5)()
        self._ck(self.L.smc_meth_sweep_check(self.ctx, out), "smc_meth_sweep_check")
        return {"expected_solves": out[0], "completed_solves": out[1], "unsolved_items": out[2], "wave_split": out[3],
                "cancelled_solves": out[4]}

    def meth_download_solves(self, n=None):
        """Outlet flows (n, n_data, 5) and solver status (n, n_data) of the last methanation sweep."""
        n = self.n_local if n is None else n
        nd = self.model[1]
        flows = np.empty((n, nd, 5))
        status = np.empty((n, nd), dtype=np.int32)
        self._ck(self.L.smc_meth_download_solves(self.ctx, _dp(flows), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n),
                 "smc_meth_download_solves")
        return flows, status

    def set_prior_mode(self, mode):
        """"mask" (default; the live branch of both reference drivers), "ratio_mask" (normal_pred and taylor,
        SMC_methanation_main.py:320-349) or "ratio" (normal_pred, :358-374)."""
        m = B.PRIOR_MODES[mode] if isinstance(mode, str) else int(mode)
        self._ck(self.L.smc_set_prior_mode(self.ctx, m), "smc_set_prior_mode")

    def set_early_reject(self, enable=True):
        """Stop (Michaelis-Menten) or do not start (methanation) the solves of a proposal that is already certain to be rejected
        (include/smc_hip.h: smc_set_early_reject, smc_meth_sweep_check)."""
        self._ck(self.L.smc_set_early_reject(self.ctx, int(bool(enable))), "smc_set_early_reject")

    def set_exact_pow(self, enable=True):
        """Parity mode of the step controller: correctly rounded pow(x, -0.2) (include/smc_hip.h: smc_set_exact_pow)."""
        if "smc_set_exact_pow" in B.MISSING:       # A/B build of an older revision (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_exact_pow(self.ctx, int(bool(enable))), "smc_set_exact_pow")

    def set_in_phase(self, enable=True):
        """Let homogeneous Michaelis-Menten Metropolis sweeps run their waves in phase (include/smc_hip.h: smc_set_in_phase)."""
        if "smc_set_in_phase" in B.MISSING:        # A/B build of an older revision (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_in_phase(self.ctx, int(bool(enable))), "smc_set_in_phase")

    def set_cost_order(self, enable=True):
        """Cost-ordered, in-phase hand-out of heterogeneous Metropolis sweeps (include/smc_hip.h: smc_set_cost_order)."""
        if "smc_set_cost_order" in B.MISSING:      # A/B build of an earlier revision (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_cost_order(self.ctx, int(bool(enable))), "smc_set_cost_order")

    def set_fast_tail(self, enable=True):
        """Hand-written lone-chain attempt loop of the Michaelis-Menten kernel (include/smc_hip.h: smc_set_fast_tail)."""
        if "smc_set_fast_tail" in B.MISSING:       # A/B build of an earlier revision (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_fast_tail(self.ctx, int(bool(enable))), "smc_set_fast_tail")

    def set_share_replicates(self, enable=True):
        """One integration per group of replicate Michaelis-Menten experiments (include/smc_hip.h: smc_set_share_replicates)."""
        if "smc_set_share_replicates" in B.MISSING:    # A/B build of an earlier revision (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_share_replicates(self.ctx, int(bool(enable))), "smc_set_share_replicates")

    def share_info(self):
        """{"n_solve": solves per particle a Michaelis-Menten sweep schedules now, "rk_attempts_shared": device-counted attempts
        since timing_reset() that rk_attempts contains but nobody executed - the partners' copies} (smc_mm_share_info)."""
        if "smc_mm_share_info" in B.MISSING:           # A/B build of an earlier revision (SMC_HIP_LIB)
            return {"n_solve": self.model[1], "rk_attempts_shared": 0}
        ns, sh = ctypes.c_int(0), ctypes.c_int64(0)
        self._ck(self.L.smc_mm_share_info(self.ctx, ctypes.byref(ns), ctypes.byref(sh)), "smc_mm_share_info")
        return {"n_solve": ns.value, "rk_attempts_shared": sh.value}

    def set_start_reject(self, enable=True):
        """Do not start a Michaelis-Menten solve whose proposal its finished siblings already reject (include/smc_hip.h:
        smc_set_start_reject; no effect unless early rejection is on)."""
        if "smc_set_start_reject" in B.MISSING:        # A/B build of an earlier revision (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_start_reject(self.ctx, int(bool(enable))), "smc_set_start_reject")

    def start_reject_info(self):
        """{"solves_not_started": (particle, experiment) items of this engine's Metropolis sweeps cancelled before their first
        attempt, since the engine was created} (smc_mm_start_reject_info)."""
        if "smc_mm_start_reject_info" in B.MISSING:    # A/B build of an earlier revision (SMC_HIP_LIB)
            return {"solves_not_started": 0}
        v = ctypes.c_int64(0)
        self._ck(self.L.smc_mm_start_reject_info(self.ctx, ctypes.byref(v)), "smc_mm_start_reject_info")
        return {"solves_not_started": v.value}

    def set_stiff_first(self, enable=True):
        """Hand the predictably long Michaelis-Menten solves out first (include/smc_hip.h: smc_set_stiff_first)."""
        if "smc_set_stiff_first" in B.MISSING:     # A/B build of a revision before the stiff list (SMC_HIP_LIB)
            return
        self._ck(self.L.smc_set_stiff_first(self.ctx, int(bool(enable))), "smc_set_stiff_first")

    def set_resampling(self, scheme):
        """"residual_systematic" (default, Micmem_SMC_main.py:147-184) or "systematic"."""
        k = B.RESAMPLING[scheme] if isinstance(scheme, str) else int(scheme)
        self._ck(self.L.smc_set_resampling(self.ctx, k), "smc_set_resampling")

    # ---- movement ------------------------------------------------------------------------------
    def upload_particles(self, which, aos):
        aos = _f64(aos)
        assert aos.ndim == 2 and aos.shape[1] == self.dim
        self._ck(self.L.smc_upload_particles(self.ctx, which, _dp(aos), aos.shape[0]), "smc_upload_particles")

    def download_particles(self, which, n=None, pinned=False):
        """(n, d) particles of set `which`.  pinned: the array lives in page-locked host memory (one DMA transfer; see _PinnedPool)."""
        n = self.n_local if n is None else n
        out = pinned_empty((n, self.dim)) if pinned else np.empty((n, self.dim))
        self._ck(self.L.smc_download_particles(self.ctx, which, _dp(out), n), "smc_download_particles")
        return out

    def upload_lk(self, which, lk):
        lk = _f64(lk)
        self._ck(self.L.smc_upload_lk(self.ctx, which, _dp(lk), lk.shape[0]), "smc_upload_lk")

    def download_lk(self, which, n=None, pinned=False):
        n = self.n_local if n is None else n
        out = pinned_empty((n,)) if pinned else np.empty(n)
        self._ck(self.L.smc_download_lk(self.ctx, which, _dp(out), n), "smc_download_lk")
        return out

    def download_accept_flags(self):
        out = np.empty(self.n_local, dtype=np.uint8)
        self._ck(self.L.smc_download_accept_flags(self.ctx, out.ctypes.data_as(B.c_u8p), self.n_local),
                 "smc_download_accept_flags")
        return out

    def debug_set_order(self, order, patience=0):
        """Probes: hand the index-ordered items of every MM likelihood sweep out in this order (None: off); smc_debug_set_order."""
        if order is None:
            self._ck(self.L.smc_debug_set_order(self.ctx, None, 0, 0), "smc_debug_set_order")
            return
        o = np.ascontiguousarray(order, dtype=np.int32)
        self._ck(self.L.smc_debug_set_order(self.ctx, o.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), o.size, int(patience)), "smc_debug_set_order")

    def download_item_info(self, n=None):
        """(n_ex, n) records of the last Michaelis-Menten sweep: attempts | cancelled << 29 | failed << 30 (diagnostics)."""
        n = self.n_local if n is None else int(n)
        out = np.empty((self.model[1], n), dtype=np.int32)
        self._ck(self.L.smc_download_item_info(self.ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n), "smc_download_item_info")
        return out

    def download_item_sums(self, n=None):
        """(n_ex, n) sums of squared residuals of the last Michaelis-Menten sweep (diagnostics; -1: cancelled solve)."""
        n = self.n_local if n is None else int(n)
        out = np.empty((self.model[1], n), dtype=np.float64)
        self._ck(self.L.smc_download_item_sums(self.ctx, _dp(out), n), "smc_download_item_sums")
        return out

    def commit_filt_to_pred(self):
        self._ck(self.L.smc_commit_filt_to_pred(self.ctx), "smc_commit_filt_to_pred")

    def sample_prior_device(self, seed, global_offset=0):
        self._ck(self.L.smc_sample_prior_device(self.ctx, int(seed), int(global_offset)), "smc_sample_prior_device")

    # ---- likelihood ----------------------------------------------------------------------------
    def loglik(self, which=SMC_SET_PRED):
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_loglik(self.ctx, which, ctypes.byref(nf), ctypes.byref(att)), "smc_loglik")
        return {"n_failed": nf.value, "rk_attempts": att.value}

    def loglik_host(self, particle, want_pred=False):
        particle = _f64(particle)
        assert particle.ndim == 2 and particle.shape[1] == 3
        n = particle.shape[0]
        lk = np.empty(n)
        pred = np.empty((n, self.model[1], self.model[2])) if want_pred else None
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_mm_loglik_host(self.ctx, _dp(particle), n, _dp(lk), _dp(pred) if want_pred else None,
                                           ctypes.byref(nf), ctypes.byref(att)), "smc_mm_loglik_host")
        return lk, pred, {"n_failed": nf.value, "rk_attempts": att.value}

    def predict_user(self, particles):
        """A user model's predictions for host particles (n, dim) (include/smc_hip.h: smc_user_predict): returns lk (n,),
        pred (n, n_ex, n_t, n_obs) - the model's outputs at every finite data time, NaN past a row's end and from where a solve
        failed - and {"n_failed", "rk_attempts"} of this call.  Leaves the particle sets and their lk untouched."""
        if self.model is None or self.model[0] != "user":
            raise SmcError("predict_user: no user model has been set")
        particles = _f64(particles)
        if particles.ndim != 2 or particles.shape[1] != self.dim:
            raise ValueError(f"predict_user: particles must be (n, {self.dim}), got {particles.shape}")
        n = particles.shape[0]
        lk = np.empty(n)
        pred = np.empty((n, self.model[1], self.model[2], self.user_n_obs))
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_user_predict(self.ctx, _dp(particles), n, _dp(lk), _dp(pred), ctypes.byref(nf), ctypes.byref(att)),
                 "smc_user_predict")
        return lk, pred, {"n_failed": nf.value, "rk_attempts": att.value}

    def _design(self, what, t, cond, inputs=None, events=None):
        """(t, cond) of a prediction design as contiguous arrays and their C arguments; (None, None): the data's own design.
        inputs: the design's inputs ({"t", "u"} as set_model_user's), handed to the library (smc_user_set_design_inputs) before
        the call; None with an explicit design clears them, and a model with inputs then refuses the design with the reason.
        events: the design's events ({"t", "values"} as set_model_user's; smc_user_set_design_events), in the same way."""
        if t is None:
            if cond is not None or inputs is not None or events is not None:
                raise ValueError(f"{what}: cond, inputs or events without t (a design is all of them, or none for the data's own)")
            return None, None, (None, None, 0, 0), (self.model[1], self.model[2])
        from .user_models import design_layout
        t = _f64(t)
        design_layout(t, cond, self.user_n_cond)
        if inputs is not None:
            if self.user_n_in == 0:
                raise ValueError(f"{what}: inputs for a model that has none")
            in_t, in_u, n_in = self._inputs(what, inputs, t.shape[0])
            if n_in != self.user_n_in:
                raise ValueError(f"{what}: the model has {self.user_n_in} inputs, the design's u holds {n_in}")
            self._ck(self.L.smc_user_set_design_inputs(self.ctx, _dp(in_t), _dp(in_u), t.shape[0], in_t.shape[1]),
                     "smc_user_set_design_inputs")
        elif self.user_n_in:
            self._ck(self.L.smc_user_set_design_inputs(self.ctx, None, None, 0, 0), "smc_user_set_design_inputs")
        if events is not None:
            if self.user_n_ev == 0:
                raise ValueError(f"{what}: events for a model that has none")
            ev_t, ev_v, n_val = self._events(what, events, t)
            if n_val != self.user_n_val:
                raise ValueError(f"{what}: the model's events hold {self.user_n_val} values, the design's hold {n_val}")
            if ev_t.shape[1] > self.user_n_ev:
                raise ValueError(f"{what}: the model was compiled for {self.user_n_ev} events per row, the design's rows hold {ev_t.shape[1]}")
            self._ck(self.L.smc_user_set_design_events(self.ctx, _dp(ev_t), None if ev_v is None else _dp(ev_v), t.shape[0], ev_t.shape[1]),
                     "smc_user_set_design_events")
        elif self.user_n_ev:
            self._ck(self.L.smc_user_set_design_events(self.ctx, None, None, 0, 0), "smc_user_set_design_events")
        cond = np.zeros((t.shape[0], 0)) if cond is None else _f64(np.asarray(cond, dtype=np.float64).reshape(t.shape[0], -1))
        cbuf = np.ascontiguousarray(cond if cond.size else np.zeros((t.shape[0], 1)))
        return t, cbuf, (_dp(t), _dp(cbuf), t.shape[0], t.shape[1]), t.shape

    def predict_user_at(self, particles, t=None, cond=None, inputs=None, events=None):
        """A user model's predictions for host particles (n, dim) on a design of its own (include/smc_hip.h: smc_user_predict_at):
        t (n_ex_new, n_t_new) rows of output times (the first is the initial time; a row may end in NaN), cond
        (n_ex_new, n_cond) - other times, a longer horizon, an experiment that was never run.  Without a design: the data's,
        with predict_user's bits.  Returns pred (n, n_ex_new, n_t_new, n_obs), NaN past a row's end and from where a solve
        failed, and {"n_failed", "rk_attempts"}.  ValueError for a design that breaks the rules (user_models.design_layout).
        A model with inputs (set_model_user(inputs=)): an explicit design brings its own, inputs={"t": (n_ex_new, n_knot_new),
        "u": (n_ex_new, n_knot_new, n_in)} - "what if I feed like this instead"; without them it is refused (SmcError).
        A model with events (set_model_user(events=)): likewise events={"t": (n_ex_new, n_ev_new), "values": ...} with n_ev_new
        up to the model's n_ev - the dosing regimen that was never run; nothing is compiled again."""
        if self.model is None or self.model[0] != "user":
            raise SmcError("predict_user_at: no user model has been set")
        particles = _f64(particles)
        if particles.ndim != 2 or particles.shape[1] != self.dim:
            raise ValueError(f"predict_user_at: particles must be (n, {self.dim}), got {particles.shape}")
        t, cbuf, cargs, shape = self._design("predict_user_at", t, cond, inputs, events)
        n = particles.shape[0]
        pred = np.empty((n, shape[0], shape[1], self.user_n_obs))
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_user_predict_at(self.ctx, _dp(particles), n, *cargs, _dp(pred), ctypes.byref(nf), ctypes.byref(att)),
                 "smc_user_predict_at")
        return pred, {"n_failed": nf.value, "rk_attempts": att.value}

    def predictive_summary(self, which=SMC_SET_FILT, probs=(0.025, 0.5, 0.975), t=None, cond=None, noise=False, seed=0,
                           global_offset=0, max_staging_bytes=0, inputs=None, events=None):
        """Posterior predictive summaries of a resident particle set, formed on the device (include/smc_hip.h:
        smc_user_predict_summary): per cell (experiment, time, output) of the design (t, cond; None: the data's) over the set's
        equally weighted particles.  Returns {"mean", "sd", "n_finite": (n_ex, n_t, n_obs); "lower", "upper", "quantile":
        (n_probs, n_ex, n_t, n_obs) - the order statistics np.nanquantile picks with method "lower" / "higher" and the linear
        value between them (user_models.quantile_ranks, linear_quantile); "n_failed", "rk_attempts"; "kernel_ms":
        {"predict", "summary"}}.  noise=True: of replicated observations pred + sigma s_k z (Philox keyed by seed,
        global_offset + particle, cell); refused on a model with a count output.  noise="family": replicated observations of every
        family - a Gaussian output as under noise=True, bit for bit, a count output a Poisson / negative-binomial count drawn with
        the prediction as its mean (csrc/count_draw.h; NaN draws, e.g. of a negative mean, leave n_finite): the band that
        should hold the data.  On a model without count outputs it is noise=True.  Only the summaries cross the bus; the sets, their lk and the accept flags are untouched.
        With several ranks each rank summarises its own block only, and the caller passes the block's start as global_offset so
        that the noise is drawn under the particles' global numbers - run_smc(predictive=...) does; with the default 0 every rank
        would draw the noise of particles 0 .. n_local - 1 and the ranks' bands would be correlated copies.
        inputs, events: as predict_user_at's."""
        if self.model is None or self.model[0] != "user":
            raise SmcError("predictive_summary: no user model has been set")
        q = _f64(np.asarray(probs, dtype=np.float64).reshape(-1))
        if not 1 <= q.size <= B.SMC_PRED_MAX_PROBS or not np.all((q >= 0) & (q <= 1)):
            raise ValueError(f"predictive_summary: 1 .. {B.SMC_PRED_MAX_PROBS} probabilities in [0, 1], got {probs!r}")
        if isinstance(noise, str):
            if noise != "family":
                raise ValueError(f"predictive_summary: noise must be False, True or \"family\", got {noise!r}")
            noise_code = B.SMC_PRED_NOISE_FAMILY
        else:
            noise_code = B.SMC_PRED_NOISE_GAUSSIAN if noise else 0
        t, cbuf, cargs, shape = self._design("predictive_summary", t, cond, inputs, events)
        cells = (shape[0], shape[1], self.user_n_obs)
        mean, sd = np.empty(cells), np.empty(cells)
        lower, upper = np.empty((q.size,) + cells), np.empty((q.size,) + cells)
        nfin = np.empty(cells, dtype=np.int64)
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        ms = np.zeros(2)
        self._ck(self.L.smc_user_predict_summary(self.ctx, int(which), *cargs, _dp(q), q.size, noise_code, int(seed),
                                                 int(global_offset), int(max_staging_bytes), _dp(mean), _dp(sd), _dp(lower),
                                                 _dp(upper), nfin.ctypes.data_as(B.c_i64p), ctypes.byref(nf), ctypes.byref(att),
                                                 _dp(ms)), "smc_user_predict_summary")
        from .user_models import linear_quantile, quantile_ranks
        quantile = linear_quantile(lower, upper, quantile_ranks(np.maximum(nfin, 1)[None], q[:, None, None, None])[2])
        return {"mean": mean, "sd": sd, "n_finite": nfin, "lower": lower, "upper": upper, "quantile": quantile,
                "n_failed": nf.value, "rk_attempts": att.value, "kernel_ms": {"predict": float(ms[0]), "summary": float(ms[1])}}

    def pointwise_loglik(self, particles):
        """The log-likelihood term of every observation for host particles (n, dim) (include/smc_hip.h: smc_user_pointwise;
        user_models.pointwise_loglik is its definition): returns ll (n, n_ex, n_t, n_obs) - NaN where a cell is not observed or
        the prediction is NaN, -inf for parameters that make logL -inf - and {"n_failed", "rk_attempts"} as predict_user's.  The
        (draws x observations) matrix ArviZ / loo take.  Leaves the particle sets and their lk untouched."""
        if self.model is None or self.model[0] != "user":
            raise SmcError("pointwise_loglik: no user model has been set")
        particles = _f64(particles)
        if particles.ndim != 2 or particles.shape[1] != self.dim:
            raise ValueError(f"pointwise_loglik: particles must be (n, {self.dim}), got {particles.shape}")
        n = particles.shape[0]
        ll = np.empty((n, self.model[1], self.model[2], self.user_n_obs))
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_user_pointwise(self.ctx, _dp(particles), n, _dp(ll), ctypes.byref(nf), ctypes.byref(att)),
                 "smc_user_pointwise")
        return ll, {"n_failed": nf.value, "rk_attempts": att.value}

    def pointwise_summary(self, which=SMC_SET_FILT, max_staging_bytes=0, count_pit=False, seed=0, global_offset=0):
        """Per observation the statistics of its log-likelihood term over a resident particle set, formed on the device
        (include/smc_hip.h: smc_user_pointwise_summary).  Returns the dict of user_models.pointwise_stats - "n", "max", "sum_exp",
        "mean", "m2", "lpd", "var", each (n_ex, n_t, n_obs) - plus "pit" (quantified Gaussian cells; NaN on censored and count
        cells; count_pit=True below fills the count cells), "n_failed", "rk_attempts", "kernel_ms": {"predict", "pointwise"} and "waic"
        (user_models.waic of it).  Only the statistics cross the bus; the sets, their lk and the accept flags are untouched.
        With several ranks each rank describes its own block; user_models.pointwise_merge joins them (run_smc(pointwise=) does).
        count_pit=True (smc_user_pointwise_summary_opt): the PIT of count cells from replicated draws (Philox keyed by seed,
        global_offset + particle, cell - pass the block's start as global_offset on several ranks, as for predictive_summary).  The
        result gains "pit_below", "pit_equal", "pit_n" (int64: the particles' replicated counts below and at the observation, and
        how many particles count; 0 off the count cells), "pit_lower" = below / n and "pit_upper" = (below + equal) / n - the
        estimates of F(y - 1) and F(y), what user_models.pit_histogram takes; a Gaussian cell enters with both = pit - and "pit"
        on count cells becomes the randomised PIT user_models.count_pit(below, equal, n, seed).  Everything else is unchanged."""
        if self.model is None or self.model[0] != "user":
            raise SmcError("pointwise_summary: no user model has been set")
        cells = (self.model[1], self.model[2], self.user_n_obs)
        n = np.empty(cells, dtype=np.int64)
        mx, se, mean, m2, pit = (np.empty(cells) for _ in range(5))
        nf, att = ctypes.c_int64(0), ctypes.c_int64(0)
        ms = np.zeros(2)
        if count_pit:
            below, equal, pn = (np.zeros(cells, dtype=np.int64) for _ in range(3))
            opts = B.PointwiseOpts(count_pit=1, seed=int(seed), global_offset=int(global_offset), pit_below=below.ctypes.data_as(B.c_i64p),
                                   pit_equal=equal.ctypes.data_as(B.c_i64p), pit_n=pn.ctypes.data_as(B.c_i64p))
            self._ck(self.L.smc_user_pointwise_summary_opt(self.ctx, int(which), int(max_staging_bytes), ctypes.byref(opts),
                                                           n.ctypes.data_as(B.c_i64p), _dp(mx), _dp(se), _dp(mean), _dp(m2), _dp(pit),
                                                           ctypes.byref(nf), ctypes.byref(att), _dp(ms)), "smc_user_pointwise_summary_opt")
        else:
            self._ck(self.L.smc_user_pointwise_summary(self.ctx, int(which), int(max_staging_bytes), n.ctypes.data_as(B.c_i64p), _dp(mx),
                                                       _dp(se), _dp(mean), _dp(m2), _dp(pit), ctypes.byref(nf), ctypes.byref(att),
                                                       _dp(ms)), "smc_user_pointwise_summary")
        from .user_models import count_pit_fill, pointwise_finish, waic
        out = pointwise_finish({"n": n, "max": mx, "sum_exp": se, "mean": mean, "m2": m2, "pit": pit})
        if count_pit:
            out.update(count_pit_fill(pit, below, equal, pn, getattr(self, "user_family", None), seed))
        out.update({"n_failed": nf.value, "rk_attempts": att.value, "kernel_ms": {"predict": float(ms[0]), "pointwise": float(ms[1])}})
        out["waic"] = waic(out)
        return out

    # ---- weights / ESS -------------------------------------------------------------------------
    def max_lk_local(self):
        v = ctypes.c_double(0)
        self._ck(self.L.smc_max_lk_local(self.ctx, ctypes.byref(v)), "smc_max_lk_local")
        return v.value

    def ess_partials(self, max_lk, gms):
        gms = _f64(gms)
        k = gms.shape[0]
        sw, sw2 = np.empty(k), np.empty(k)
        self._ck(self.L.smc_ess_partials(self.ctx, float(max_lk), _dp(gms), k, _dp(sw), _dp(sw2)), "smc_ess_partials")
        return sw, sw2

    # ---- the same stages reduced over all ranks on the device (RCCL in place, one read-back) ------
    def max_lk_global(self):
        v = ctypes.c_double(0)
        self._ck(self.L.smc_max_lk_global(self.ctx, ctypes.byref(v)), "smc_max_lk_global")
        return v.value

    def ess_partials_global(self, max_lk, gms):
        gms = _f64(gms)
        k = gms.shape[0]
        sw, sw2 = np.empty(k), np.empty(k)
        self._ck(self.L.smc_ess_partials_global(self.ctx, float(max_lk), _dp(gms), k, _dp(sw), _dp(sw2)),
                 "smc_ess_partials_global")
        return sw, sw2

    def ess_search_global(self, gms, with_max=True):
        """max(lk) and the weight sums of up to 32 candidate increments, all ranks, one synchronisation
        (include/smc_hip.h: smc_ess_search_global) -> (max_lk, sum_w, sum_w2)."""
        gms = _f64(gms)
        k = gms.shape[0]
        sw, sw2 = np.empty(k), np.empty(k)
        m = ctypes.c_double(0)
        self._ck(self.L.smc_ess_search_global(self.ctx, _dp(gms), k, int(bool(with_max)), ctypes.byref(m), _dp(sw), _dp(sw2)),
                 "smc_ess_search_global")
        return m.value, sw, sw2

    def resample_global(self, max_lk, gm, sum_w, wrand, first_step):
        o, cs = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_resample_global(self.ctx, float(max_lk), float(gm), float(sum_w), float(wrand),
                                            int(bool(first_step)), ctypes.byref(o), ctypes.byref(cs)), "smc_resample_global")
        return {"n_offspring": o.value, "count_sum": cs.value}

    def resample_enqueue(self, max_lk, gm, sum_w, wrand, first_step):
        """Resampling without a host synchronisation (one rank; include/smc_hip.h: smc_resample_enqueue); resample_result() later."""
        self._ck(self.L.smc_resample_enqueue(self.ctx, float(max_lk), float(gm), float(sum_w), float(wrand), int(bool(first_step))),
                 "smc_resample_enqueue")

    def resample_result(self):
        o, cs = ctypes.c_int64(0), ctypes.c_int64(0)
        self._ck(self.L.smc_resample_result(self.ctx, ctypes.byref(o), ctypes.byref(cs)), "smc_resample_result")
        return {"n_offspring": o.value, "count_sum": cs.value}

    def mh_iteration_device_rng(self, gamma, mhstep_ratio, w_cov, seed, stream, global_offset=0):
        """One fused Metropolis iteration (moments -> cov_m -> factor -> propose -> solve -> accept -> counts), all ranks
        together.  Accept counts and n_failed are totals over all ranks."""
        w_cov = _f64(w_cov, (self.dim, self.dim))
        o = self._mh_out()
        cov = np.empty((self.dim, self.dim))
        self._ck(self.L.smc_mh_iteration_device_rng(self.ctx, float(gamma), float(mhstep_ratio), _dp(w_cov), int(seed),
                                                    int(stream), int(global_offset), *[ctypes.byref(x) for x in o], _dp(cov)),
                 "smc_mh_iteration_device_rng")
        return {"accepted_now": o[0].value, "accepted_ever": o[1].value, "n_failed": o[2].value,
                "rk_attempts": o[3].value, "cov_m": cov}

    def mh_sweeps_device_rng(self, gamma, mhstep_ratio, w_cov, seed, stream0, n_iter, thr_stop, thr_halve, global_offset=0):
        """A batch of n_iter fused Metropolis iterations with the loop control (break / halve mhstep_ratio, Micmem_SMC_main.py:
        243-249) on the device and ONE synchronisation (include/smc_hip.h: smc_mh_sweeps_device_rng).  Returns how many ran,
        whether the loop ended by its break, the mhstep_ratio a following batch starts with, and one record per iteration that
        ran (counts are totals over all ranks, rk_attempts this rank's)."""
        w_cov = _f64(w_cov, (self.dim, self.dim))
        k = int(n_iter)
        nd, st, rn = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0)
        an, ae, nf, at = (np.zeros(k, dtype=np.int64) for _ in range(4))
        ru, cov = np.zeros(k), np.zeros((k, self.dim, self.dim))
        sc = np.zeros((k, B.SMC_SWEEP_COUNTER_WORDS), dtype=np.int64)
        self._ck(self.L.smc_mh_sweeps_device_rng(self.ctx, float(gamma), float(mhstep_ratio), _dp(w_cov), int(seed), int(stream0), k,
                                                 float(thr_stop), float(thr_halve), int(global_offset), ctypes.byref(nd),
                                                 ctypes.byref(st), ctypes.byref(rn), an.ctypes.data_as(B.c_i64p),
                                                 ae.ctypes.data_as(B.c_i64p), nf.ctypes.data_as(B.c_i64p),
                                                 at.ctypes.data_as(B.c_i64p), _dp(ru), _dp(cov), sc.ctypes.data_as(B.c_i64p)),
                 "smc_mh_sweeps_device_rng")
        its = [{"accepted_now": int(an[i]), "accepted_ever": int(ae[i]), "n_failed": int(nf[i]), "rk_attempts": int(at[i]),
                "mhstep_ratio": float(ru[i]), "cov_m": cov[i].copy()} for i in range(nd.value)]
        if self.model is not None and self.model[0] == "methanation":     # K8's work and completeness counters per sweep (the driver's books)
            for i, it in enumerate(its):
                it["counters"] = {nm: int(sc[i, q]) for q, nm in enumerate(B.SWEEP_COUNTER_NAMES)}
        return {"n_done": nd.value, "stopped": bool(st.value), "ratio_next": rn.value, "iterations": its}

    def proposal_factor_device(self, w_cov):
        """cov_m = np.cov(p_filt.T, bias=True) * w_cov over all ranks and its multivariate_normal factor, both on the device."""
        w_cov = _f64(w_cov, (self.dim, self.dim))
        cov, xf = np.empty((self.dim, self.dim)), np.empty((self.dim, self.dim))
        self._ck(self.L.smc_proposal_factor_device(self.ctx, _dp(w_cov), _dp(cov), _dp(xf)), "smc_proposal_factor_device")
        return cov, xf

    def mh_iteration_last_transform(self):
        out = np.empty((self.dim, self.dim))
        self._ck(self.L.smc_mh_iteration_last_transform(self.ctx, _dp(out)), "smc_mh_iteration_last_transform")
        return out

    # ---- resampling ----------------------------------------------------------------------------
    def resample_phase1(self, max_lk, gm, sum_w):
        r, c = ctypes.c_double(0), ctypes.c_int64(0)
        self._ck(self.L.smc_resample_phase1(self.ctx, float(max_lk), float(gm), float(sum_w), ctypes.byref(r),
                                            ctypes.byref(c)), "smc_resample_phase1")
        return r.value, c.value

    def resample_phase2(self, max_lk, gm, sum_w, residual_prefix, wrand):
        o = ctypes.c_int64(0)
        self._ck(self.L.smc_resample_phase2(self.ctx, float(max_lk), float(gm), float(sum_w), float(residual_prefix),
                                            float(wrand), ctypes.byref(o)), "smc_resample_phase2")
        return o.value

    def download_offspring(self):
        out = np.empty(self.n_local, dtype=np.int64)
        self._ck(self.L.smc_download_offspring(self.ctx, out.ctypes.data_as(B.c_i64p), self.n_local),
                 "smc_download_offspring")
        return out

    def resample_phase3(self, out_base_all, offspring_all, first_step):
        b = np.ascontiguousarray(out_base_all, dtype=np.int64)
        o = np.ascontiguousarray(offspring_all, dtype=np.int64)
        assert b.shape == o.shape == (self.world,)
        self._ck(self.L.smc_resample_phase3(self.ctx, b.ctypes.data_as(B.c_i64p), o.ctypes.data_as(B.c_i64p),
                                            int(bool(first_step))), "smc_resample_phase3")
        if self._peer_barrier is not None:      # loopback rehearsal: pack | barrier | pull | barrier
            self._peer_barrier()
            self._ck(self.L.smc_resample_phase3_pull(self.ctx), "smc_resample_phase3_pull")
            self._peer_barrier()

    def debug_set_local_peers(self, engines, rank, barrier):
        """Loopback rehearsal of the multi-rank path on one device (see include/smc_hip.h)."""
        arr = (B.c_ctx * len(engines))(*[e.ctx for e in engines])
        self._ck(self.L.smc_debug_set_local_peers(self.ctx, arr, int(rank), len(engines)), "smc_debug_set_local_peers")
        self.rank, self.world = int(rank), len(engines)
        self._peer_barrier = barrier

    def debug_peer_collectives(self, enable=True):
        """Loopback rehearsal with the collectives inside the engine (include/smc_hip.h: smc_debug_peer_collectives): the
        *_global entry points reduce among the local peers; the Python-side pull of resample_phase3 is no longer needed."""
        self._ck(self.L.smc_debug_peer_collectives(self.ctx, int(bool(enable))), "smc_debug_peer_collectives")
        if enable:
            self._peer_barrier = None

    # ---- moments -------------------------------------------------------------------------------
    def moment_sums_local(self):
        out = np.empty(self.dim)
        self._ck(self.L.smc_moment_sums_local(self.ctx, _dp(out)), "smc_moment_sums_local")
        return out

    def moment_centered_local(self, mean):
        mean = _f64(mean, (self.dim,))
        out = np.empty((self.dim, self.dim))
        self._ck(self.L.smc_moment_centered_local(self.ctx, _dp(mean), _dp(out)), "smc_moment_centered_local")
        return out

    # ---- MH ------------------------------------------------------------------------------------
    def reset_accept_flags(self):
        self._ck(self.L.smc_reset_accept_flags(self.ctx), "smc_reset_accept_flags")

    def _mh_out(self):
        return [ctypes.c_int64(0) for _ in range(4)]

    def mh_step_host_rng(self, gamma, mhstep_ratio, noise, rr):
        noise = _f64(noise, (self.n_local, self.dim))
        rr = _f64(rr, (self.n_local,))
        o = self._mh_out()
        self._ck(self.L.smc_mh_step_host_rng(self.ctx, float(gamma), float(mhstep_ratio), _dp(noise), _dp(rr),
                                             self.n_local, *[ctypes.byref(x) for x in o]), "smc_mh_step_host_rng")
        return {"accepted_now": o[0].value, "accepted_ever": o[1].value, "n_failed": o[2].value,
                "rk_attempts": o[3].value}

    def mh_step_device_rng(self, gamma, mhstep_ratio, transform, seed, stream, global_offset=0):
        transform = _f64(transform, (self.dim, self.dim))
        o = self._mh_out()
        self._ck(self.L.smc_mh_step_device_rng(self.ctx, float(gamma), float(mhstep_ratio), _dp(transform), int(seed),
                                               int(stream), int(global_offset), *[ctypes.byref(x) for x in o]),
                 "smc_mh_step_device_rng")
        return {"accepted_now": o[0].value, "accepted_ever": o[1].value, "n_failed": o[2].value,
                "rk_attempts": o[3].value}

    def set_debug_capture(self, enable=True):
        self._ck(self.L.smc_set_debug_capture(self.ctx, int(enable)), "smc_set_debug_capture")

    def download_debug_proposals(self):
        n = self.n_local
        aos, lk2 = np.empty((n, self.dim)), np.empty(n)
        p0, r = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
        self._ck(self.L.smc_download_debug_proposals(self.ctx, _dp(aos), _dp(lk2), p0.ctypes.data_as(B.c_u8p),
                                                     r.ctypes.data_as(B.c_u8p), n), "smc_download_debug_proposals")
        return aos, lk2, p0, r

    def debug_rccl_self_exchange(self, row, cnt, dst_row):
        self._ck(self.L.smc_debug_rccl_self_exchange(self.ctx, int(row), int(cnt), int(dst_row)), "smc_debug_rccl_self_exchange")

    # ---- collectives (RCCL) --------------------------------------------------------------------
    @staticmethod
    def comm_get_unique_id() -> bytes:
        buf = (ctypes.c_uint8 * 128)()
        st = lib().smc_comm_get_unique_id(buf)
        if st != 0:
            msg = lib().smc_last_error(None)
            raise SmcError(f"smc_comm_get_unique_id: {msg.decode() if msg else ''}")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        self._ck(self.L.smc_comm_init(self.ctx, buf, int(rank), int(world)), "smc_comm_init")
        self.rank, self.world = int(rank), int(world)

    def comm_info(self):
        """RCCL's own view of this context's communicator: {"count", "user_rank", "device"} (count 0: none)."""
        n, r, d = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.L.smc_comm_info(self.ctx, ctypes.byref(n), ctypes.byref(r), ctypes.byref(d)), "smc_comm_info")
        return {"count": n.value, "user_rank": r.value, "device": d.value}

    def comm_allreduce_sum_f64(self, x):
        x = _f64(x).copy()
        self._ck(self.L.smc_comm_allreduce_sum_f64(self.ctx, _dp(x), x.size), "smc_comm_allreduce_sum_f64")
        return x

    def comm_allreduce_max_f64(self, x):
        x = _f64(x).copy()
        self._ck(self.L.smc_comm_allreduce_max_f64(self.ctx, _dp(x), x.size), "smc_comm_allreduce_max_f64")
        return x

    def comm_allreduce_sum_i64(self, x):
        x = np.ascontiguousarray(x, dtype=np.int64).copy()
        self._ck(self.L.smc_comm_allreduce_sum_i64(self.ctx, x.ctypes.data_as(B.c_i64p), x.size),
                 "smc_comm_allreduce_sum_i64")
        return x

    def comm_allgather_f64(self, x):
        x = _f64(x)
        out = np.empty((self.world,) + x.shape)
        self._ck(self.L.smc_comm_allgather_f64(self.ctx, _dp(x), x.size, _dp(out)), "smc_comm_allgather_f64")
        return out

    def comm_allgather_i64(self, x):
        x = np.ascontiguousarray(x, dtype=np.int64)
        out = np.empty((self.world,) + x.shape, dtype=np.int64)
        self._ck(self.L.smc_comm_allgather_i64(self.ctx, x.ctypes.data_as(B.c_i64p), x.size,
                                               out.ctypes.data_as(B.c_i64p)), "smc_comm_allgather_i64")
        return out

    def comm_barrier(self):
        self._ck(self.L.smc_comm_barrier(self.ctx), "smc_comm_barrier")

    # ---- timing --------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._ck(self.L.smc_timing_enable(self.ctx, int(on)), "smc_timing_enable")

    def timing_reset(self):
        self._ck(self.L.smc_timing_reset(self.ctx), "smc_timing_reset")

    def timing_get(self):
        out = {}
        for which, name in B.TIMING_NAMES.items():
            n, ms = ctypes.c_int64(0), ctypes.c_double(0)
            self._ck(self.L.smc_timing_get(self.ctx, which, ctypes.byref(n), ctypes.byref(ms)), "smc_timing_get")
            out[name] = {"launches": n.value, "ms": ms.value}
        return out

    def work_totals(self):
        """Device-counted Michaelis-Menten work since timing_reset(): solves that produced their outputs, RK45 attempts, solve
        launches with work, speculative launches that found the loop ended (smc_work_totals)."""
        if "smc_work_totals" in B.MISSING:         # A/B build of an older revision (SMC_HIP_LIB)
            return None
        out = (ctypes.c_int64 * 4)()
        self._ck(self.L.smc_work_totals(self.ctx, out), "smc_work_totals")
        return {"solved_items": out[0], "rk_attempts": out[1], "solve_launches": out[2], "noop_launches": out[3]}
