"""Example sources for HipEngine.set_model_user (include/smc_hip.h: smc_set_model_user) - what a user of the
reference writes instead of a new Micmem_likelihood.py (README.md:4, "modify for your problem")."""

# Micmem_likelihood.py:14-33 as a user model: theta = (Vmax, Km, sigma), cond = (S0,), one state S, observed P = S0 - S
MICHAELIS_MENTEN_PLAIN = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = smc_div((-theta[0]) * y[0], theta[1] + y[0]);     // a / b, faster (include/smc_hip.h)
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return cond[0] - y[0]; }
"""
# ... with the optional cost hint (include/smc_hip.h): explicit RK45 runs on its stability limit for about 3.7 Vmax / Km step
# attempts, so the sweeps hand those solves out first and run the longest one per wave - results are the same either way
MICHAELIS_MENTEN = MICHAELIS_MENTEN_PLAIN + r"""
__device__ double smc_user_cost(const double *theta) { return theta[1] > 0.0 ? 3.7 * theta[0] / theta[1] : 0.0; }
"""

# two states: A -> B -> C with rate constants theta = (k1, k2, sigma), cond = (A0,), the intermediate B is observed
CONSECUTIVE_REACTIONS = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = -theta[0] * y[0];
    dydt[1] = theta[0] * y[0] - theta[1] * y[1];
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[1]; }
"""

# Robertson's stiff kinetics (A -> B, B + B -> C + B, B + C -> A + C) for method="BDF" (include/smc_hip.h): the rate constants
# k1 = theta[0] and k3 = theta[1] are estimated, k2 = 3e7 is fixed; theta = (k1, k3, sigma), cond = (A0,), the product C is
# observed.  With the classic k1 = 0.04, k3 = 1e4 explicit RK45 runs on its stability limit (tens of thousands of attempts).
ROBERTSON_NUMJAC = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; y[2] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    const double k1 = theta[0], k2 = 3e7, k3 = theta[1];
    dydt[0] = -k1 * y[0] + k3 * y[1] * y[2];
    dydt[1] = k1 * y[0] - k3 * y[1] * y[2] - k2 * y[1] * y[1];
    dydt[2] = k2 * y[1] * y[1];
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[2]; }
"""
# ... with the analytic Jacobian (row-major J[i * 3 + j] = d dydt[i] / d y[j])
ROBERTSON = ROBERTSON_NUMJAC + r"""
__device__ void smc_user_jac(double t, const double *y, const double *theta, const double *cond, double *J) {
    const double k1 = theta[0], k2 = 3e7, k3 = theta[1];
    J[0] = -k1; J[1] = k3 * y[2];                    J[2] = k3 * y[1];
    J[3] = k1;  J[4] = -k3 * y[2] - 2.0 * k2 * y[1]; J[5] = -k3 * y[1];
    J[6] = 0.0; J[7] = 2.0 * k2 * y[1];              J[8] = 0.0;
}
"""

# several observed outputs (include/smc_hip.h: smc_set_model_user3, n_obs = 2): A -> B -> C as above with both A and B measured.
# Closed form: A = A0 e^(-k1 t), B = A0 k1 / (k2 - k1) (e^(-k1 t) - e^(-k2 t)), C = A0 - A - B (the unobserved product)
CONSECUTIVE_REACTIONS_AB = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = -theta[0] * y[0];
    dydt[1] = theta[0] * y[0] - theta[1] * y[1];
}
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) {
    out[0] = y[0];
    out[1] = y[1];
}
"""
# ... and the unobserved product C = A0 - A - B as a third output, for predictions (give it an all-NaN column of obs)
CONSECUTIVE_REACTIONS_ABC = CONSECUTIVE_REACTIONS_AB.replace("    out[1] = y[1];\n", "    out[1] = y[1];\n    out[2] = cond[0] - y[0] - y[1];\n")

# Robertson's kinetics (ROBERTSON, method="BDF") with A and C measured: A falls from A0 while C stays below about 1e-2 A0 over
# the data times - outputs orders of magnitude apart, what obs_scale is for
ROBERTSON_AC = ROBERTSON.replace(
    "__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[2]; }\n",
    "__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) {\n"
    "    out[0] = y[0];\n    out[1] = y[2];\n}\n")

# Scheduled events (include/smc_hip.h: smc_set_model_user6).  A one-compartment model under repeated bolus doses:
# theta = (k, sigma), cond = (y0,), dC/dt = -k C and event j adds its value 0 (the dose over the volume) to C
ONE_COMPARTMENT_DOSED = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) { dydt[0] = -theta[0] * y[0]; }
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[0]; }
__device__ void smc_user_event(int j, double t, double *y, const double *theta, const double *cond) { y[0] += smc_event_value(cond, j, 0); }
"""
# Oral dosing, gut -> central -> out: theta = (ka, ke, F, sigma), cond = (gut0,), both compartments observed.  An event holds
# (amount, kind): kind 0 is a dose into the gut of which the fraction F = theta[2] arrives (the jump depends on theta), kind 1
# empties the central compartment (a washout)
ORAL_DOSING = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = -theta[0] * y[0];
    dydt[1] = theta[0] * y[0] - theta[1] * y[1];
}
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) {
    out[0] = y[0];
    out[1] = y[1];
}
__device__ void smc_user_event(int j, double t, double *y, const double *theta, const double *cond) {
    if (smc_event_value(cond, j, 1) == 0.0)
        y[0] += theta[2] * smc_event_value(cond, j, 0);
    else
        y[1] = 0.0;
}
"""

# State-triggered events (include/smc_hip.h: STATE-TRIGGERED EVENTS).  A level that decays and is re-dosed whenever it falls to a
# threshold: theta = (k, D, sigma), cond = (y0, L), dC/dt = -k C; event function g = C - L, falling; the event adds D = theta[1].
# The fire times depend on the parameters: the first at log(y0 / L) / k, then every log((L + D) / L) / k.
THRESHOLD_REDOSED = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) { dydt[0] = -theta[0] * y[0]; }
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[0]; }
__device__ const int smc_user_root_dir[] = {-1};
__device__ void smc_user_root(double t, const double *y, const double *theta, const double *cond, double *g) { g[0] = y[0] - cond[1]; }
__device__ void smc_user_root_event(int k, double t, double *y, const double *theta, const double *cond) { y[0] += theta[1]; }
"""

SMC_USER_MAX_ROOTS, SMC_USER_MAX_ROOT_FIRES = 4, 256


def brentq(f, a, b, xtol=4 * 2.220446049250313e-16, rtol=4 * 2.220446049250313e-16, maxiter=100, full_output=False):
    """scipy.optimize.brentq(f, a, b, xtol, rtol, maxiter) restated in Python floats, statement by statement (Zeros/brentq.c) - the
    text the kernels follow (csrc/user_root.h), with the tolerances solve_ivp's events use as defaults.  Returns the root, with
    full_output (root, function calls, iterations): bit for bit SciPy's.  Raises ValueError where f(a) and f(b) have one sign or
    f returns NaN, RuntimeError without convergence within maxiter iterations - where SciPy raises."""
    import math

    def call(x):
        v = float(f(x))
        if math.isnan(v):
            raise ValueError(f"brentq: the function value at x={x} is NaN; solver cannot continue")
        return v

    def done(x, calls, it):
        return (x, calls, it) if full_output else x

    sign = lambda v: math.copysign(1.0, v) < 0
    xpre, xcur = float(a), float(b)
    xblk = fblk = spre = scur = 0.0
    fpre, fcur = call(xpre), call(xcur)
    calls = 2
    if fpre == 0:
        return done(xpre, calls, 0)
    if fcur == 0:
        return done(xcur, calls, 0)
    if sign(fpre) == sign(fcur):
        raise ValueError("brentq: f(a) and f(b) must have different signs")
    for it in range(1, int(maxiter) + 1):
        if fpre != 0 and fcur != 0 and sign(fpre) != sign(fcur):
            xblk, fblk = xpre, fpre
            spre = scur = xcur - xpre
        if abs(fblk) < abs(fcur):
            xpre, xcur = xcur, xblk
            xblk = xpre
            fpre, fcur = fcur, fblk
            fblk = fpre
        delta = (xtol + rtol * abs(xcur)) / 2
        sbis = (xblk - xcur) / 2
        if fcur == 0 or abs(sbis) < delta:
            return done(xcur, calls, it)
        if abs(spre) > delta and abs(fcur) < abs(fpre):
            if xpre == xblk:      # interpolate
                stry = -fcur * (xcur - xpre) / (fcur - fpre)
            else:                 # extrapolate
                dpre = (fpre - fcur) / (xpre - xcur)
                dblk = (fblk - fcur) / (xblk - xcur)
                stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre))
            if 2 * abs(stry) < min(abs(spre), 3 * abs(sbis) - delta):      # good short step
                spre, scur = scur, stry
            else:                 # bisect
                spre = scur = sbis
        else:                     # bisect
            spre = scur = sbis
        xpre, fpre = xcur, fcur
        if abs(scur) > delta:
            xcur += scur
        else:
            xcur += delta if sbis > 0 else -delta
        fcur = call(xcur)
        calls += 1
    raise RuntimeError(f"brentq: failed to converge after {maxiter} iterations")


def root_chain(rhs, y0, t_row, root, root_dir, root_event, method="RK45", rtol=1e-3, atol=1e-6, jac=None, scheduled=()):
    """A solve of a model with state-triggered events (include/smc_hip.h) as the chain of solve_ivp calls a SciPy user writes - the
    reference the kernels are held to.  rhs(t, y); y0 (ns,); t_row: the row's data times, strictly increasing, t_row[0] the
    initial time (NaN past the row's end is dropped); root(t, y) -> (n_root,) the event functions, root_dir their directions
    (-1 falling, 0 either, +1 rising), root_event(k, t, y) -> the state after the jump of event k; scheduled: [(tau, jump)],
    scheduled events with jump(t, y) -> y, of which those strictly inside the row fire.
    Every call is solve_ivp(rhs, (a, b), y, method, events = the event functions, all terminal, dense_output=True, rtol, atol[,
    jac]) with b the next scheduled time or the row's end.  The data times in (a, t_stop] (the first call: [t0, t_stop]) are read
    from the call's dense output, so a data time equal to a fire time holds the state before the jump.  A call that ends at an
    event (status 1) is followed by root_event on its end state - the earliest root, on a tie the lowest k - and the next call
    starts from (t*, y); a root at b meets the scheduled jump after the triggered one.  The rules a chain written by hand
    leaves open: a root at the start of its own call (the jump left the state on a firing surface; the chain would not move
    again) raises RuntimeError, and so does fire number SMC_USER_MAX_ROOT_FIRES + 1.
    Returns {"y": (len, ns) states at the row's times, "fires": [(k, t*)], "steps", "nlu", "njev": totals over the calls}."""
    import numpy as np
    from scipy.integrate import solve_ivp
    tt = np.asarray(t_row, dtype=np.float64)
    tt = tt[~np.isnan(tt)]
    t0, t_end = tt[0], tt[-1]
    ns = np.asarray(y0).size
    n_root = len(root_dir)
    events = []
    for k in range(n_root):
        ev = (lambda k: lambda t, y: float(np.asarray(root(t, y))[k]))(k)
        ev.terminal, ev.direction = True, float(root_dir[k])
        events.append(ev)
    out = np.full((tt.size, ns), np.nan)
    y = np.array(y0, dtype=np.float64)
    fires, steps, nlu, njev = [], 0, 0, 0
    if t_end == t0:
        out[0] = y
        return {"y": out, "fires": fires, "steps": 0, "nlu": 0, "njev": 0}
    bounds = [(tau, jump) for tau, jump in scheduled if t0 < tau < t_end] + [(t_end, None)]
    a, first = t0, True
    for b, jump in bounds:
        while True:
            kw = {"jac": jac} if (jac is not None and method != "RK45") else {}
            sol = solve_ivp(rhs, (a, b), y, method=method, events=events, dense_output=True, rtol=rtol, atol=atol, **kw)
            if sol.status < 0:
                raise RuntimeError(f"root_chain: {sol.message}")
            t_stop = sol.t[-1]
            steps += sol.t.size - 1
            nlu += sol.nlu
            njev += sol.njev
            take = ((tt > a) | (first & (tt == a))) & (tt <= t_stop)
            if take.any():
                out[take] = sol.sol(tt[take]).T
            first = False
            y = sol.y[:, -1].copy()
            if sol.status == 1:
                k = next(k for k in range(n_root) if sol.t_events[k].size)
                if t_stop == a:
                    raise RuntimeError(f"root_chain: event {k} fires at t = {a!r}, the start of its own segment")
                y = np.array(root_event(k, t_stop, y), dtype=np.float64)
                fires.append((k, float(t_stop)))
                if len(fires) > SMC_USER_MAX_ROOT_FIRES:
                    raise RuntimeError(f"root_chain: more than {SMC_USER_MAX_ROOT_FIRES} fires in one solve")
            a = t_stop
            if t_stop == b:
                break
        if jump is not None:
            y = np.array(jump(b, y), dtype=np.float64)
    return {"y": out, "fires": fires, "steps": steps, "nlu": nlu, "njev": njev}


def obs_layout(t, obs, obs_scale=None):
    """The data rules of smc_set_model_user3 (include/smc_hip.h), in NumPy: t (n_ex, n_t); obs (n_ex, n_t, n_obs) with NaN for a
    value that was not measured; obs_scale (n_obs,) relative scales s_k > 0 (None: ones).  A row of t is a strictly increasing
    run of finite times, possibly followed by NaN only.  Returns {"n_t_e": (n_ex,) int, "m_e": (n_ex,) finite observations at
    the row's times, "sum_log_scale": (n_ex,) sum of log s_k over them}; raises ValueError for data the library refuses."""
    import numpy as np
    t = np.asarray(t, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    if t.ndim != 2 or obs.ndim != 3 or obs.shape[:2] != t.shape:
        raise ValueError(f"obs_layout: t must be (n_ex, n_t) and obs (n_ex, n_t, n_obs), got {t.shape} and {obs.shape}")
    n_ex, n_t, n_obs = obs.shape
    if not 1 <= n_obs <= 8:
        raise ValueError(f"obs_layout: n_obs = {n_obs} outside 1 .. 8 (SMC_USER_MAX_OBS)")
    scale = np.ones(n_obs) if obs_scale is None else np.asarray(obs_scale, dtype=np.float64).reshape(-1)
    if scale.shape != (n_obs,):
        raise ValueError(f"obs_layout: obs_scale must have n_obs = {n_obs} entries, got {scale.shape}")
    if not np.all(np.isfinite(scale) & (scale > 0)):
        raise ValueError("obs_layout: obs_scale must be finite and > 0")
    nan_t = np.isnan(t)
    n_t_e = np.where(nan_t.any(axis=1), nan_t.argmax(axis=1), n_t)
    for e in range(n_ex):
        k = n_t_e[e]
        if not nan_t[e, k:].all():
            raise ValueError(f"obs_layout: row {e} of t has a NaN time before a number (only a trailing run of NaN may shorten a row)")
        if k == 0:
            raise ValueError(f"obs_layout: row {e} of t has no finite time")
        if not np.all(np.isfinite(t[e, :k])):
            raise ValueError(f"obs_layout: row {e} of t holds an infinite time")
        if not np.all(np.diff(t[e, :k]) > 0):
            raise ValueError(f"obs_layout: row {e} of t is not strictly increasing")
    inside = np.arange(n_t)[None, :] < n_t_e[:, None]
    o = np.where(inside[:, :, None], obs, np.nan)
    if np.any(np.isinf(o)):
        raise ValueError("obs_layout: obs holds an infinite value (NaN marks a value that was not measured)")
    seen = ~np.isnan(o)
    return {"n_t_e": n_t_e.astype(np.int64), "m_e": seen.sum(axis=(1, 2)).astype(np.int64),
            "sum_log_scale": np.sum(np.where(seen, np.log(scale)[None, None, :], 0.0), axis=(1, 2))}


def noise_layout(noise, n_obs, dim):
    """The rules of a noise specification (include/smc_hip.h: smc_set_model_user4), in NumPy.  noise = {"additive": [entry per
    output], "proportional": [entry per output] (optional)}, an entry ("param", j) - parameter j in [0, dim) - or ("fixed", v)
    with v finite and > 0 (additive) or >= 0 (proportional).  Returns (add_index, add_fixed, prop_index, prop_fixed): int32 /
    float64 arrays of n_obs entries, index -1 where the value is fixed; the last two None without a proportional part.  Raises
    ValueError for a specification the library refuses."""
    import numpy as np
    if not isinstance(noise, dict) or "additive" not in noise or set(noise) - {"additive", "proportional"}:
        raise ValueError('noise_layout: noise must be {"additive": [...], "proportional": [...] (optional)}')
    n_obs, dim = int(n_obs), int(dim)

    def part(name, lowest_ok):
        entries = list(noise[name])
        if len(entries) != n_obs:
            raise ValueError(f"noise_layout: {name!r} must have n_obs = {n_obs} entries, got {len(entries)}")
        index, fixed = np.full(n_obs, -1, dtype=np.int32), np.zeros(n_obs)
        for k, entry in enumerate(entries):
            if not (isinstance(entry, (tuple, list)) and len(entry) == 2 and entry[0] in ("param", "fixed")):
                raise ValueError(f'noise_layout: {name}[{k}] must be ("param", j) or ("fixed", v), got {entry!r}')
            if entry[0] == "param":
                j = int(entry[1])
                if j != entry[1] or not 0 <= j < dim:
                    raise ValueError(f"noise_layout: {name}[{k}] names parameter {entry[1]!r} outside [0, {dim})")
                index[k] = j
            else:
                v = float(entry[1])
                if not (np.isfinite(v) and lowest_ok(v)):
                    raise ValueError(f"noise_layout: {name}[{k}] fixed value {v!r} must be finite and "
                                     + ("> 0" if name == "additive" else ">= 0"))
                fixed[k] = v
        return index, fixed

    add_index, add_fixed = part("additive", lambda v: v > 0)
    if noise.get("proportional") is None:
        return add_index, add_fixed, None, None
    prop_index, prop_fixed = part("proportional", lambda v: v >= 0)
    return add_index, add_fixed, prop_index, prop_fixed


def noise_loglik(pred, t, obs, theta, noise, obs_scale=None):
    """The likelihood of a noise model (include/smc_hip.h: smc_set_model_user4) applied to given model outputs - its executable
    definition.  pred (n, n_ex, n_t, n_obs) outputs f, t (n_ex, n_t), obs (n_ex, n_t, n_obs), theta (n, dim).  With a_k, b_k
    taken from theta or fixed (noise_layout) and s_k = obs_scale:  sd^2 = (a_k s_k)^2 + (b_k f)^2,
    logL = sum over observed (e, i, k) [-1/2 log(2 pi) - log sd - (obs - f)^2 / (2 sd^2)]; observed = obs finite at a finite
    time of the row; -inf where any a_k <= 0 or any b_k < 0.  Returns (n,)."""
    import numpy as np
    pred = np.asarray(pred, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    n_obs = obs.shape[2]
    ai, af, pi, pf = noise_layout(noise, n_obs, theta.shape[1])
    scale = np.ones(n_obs) if obs_scale is None else np.asarray(obs_scale, dtype=np.float64).reshape(n_obs)
    a = np.where(ai >= 0, theta[:, np.maximum(ai, 0)], af[None, :])                      # (n, n_obs)
    b = np.zeros_like(a) if pi is None else np.where(pi >= 0, theta[:, np.maximum(pi, 0)], pf[None, :])
    seen = ~np.isnan(obs) & ~np.isnan(np.asarray(t, dtype=np.float64))[:, :, None]
    f = np.where(seen[None], pred, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd2 = (a * scale)[:, None, None, :] ** 2 + (b[:, None, None, :] * f) ** 2
        r = np.where(seen[None], obs[None] - f, 0.0)
        term = np.where(seen[None], -0.5 * np.log(2 * np.pi) - 0.5 * np.log(sd2) - r * r / (2 * sd2), 0.0)
        lk = term.sum(axis=(1, 2, 3))
    return np.where(np.all(a > 0, axis=1) & np.all(b >= 0, axis=1), lk, -np.inf)


def censor_layout(t, obs, censor):
    """The rules of the flags of censored observations (include/smc_hip.h: smc_set_model_user7), in NumPy, for t (n_ex, n_t) and
    obs (n_ex, n_t, n_obs) that obs_layout accepts: censor has obs's shape; a flag is 0 (obs is the measured value), -1
    (left-censored: the true value is <= obs, the lower limit) or +1 (right-censored: >= obs, the upper limit); a nonzero flag
    stands on a finite value at a finite time of its row.  Returns {"quantified": (n_ex, n_obs) int, "censored": (n_ex, n_obs)
    int}, the counts per experiment and output (quantified = m_ek); raises ValueError, in the library's words
    (smc_user_censor_check), for flags the library refuses - the first offence in row-major order."""
    import numpy as np
    t = np.asarray(t, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    n_t_e = obs_layout(t, obs)["n_t_e"]
    c = np.asarray(censor)
    if c.shape != obs.shape:
        raise ValueError(f"censor_layout: censor must have the shape of obs {tuple(int(v) for v in obs.shape)}, "
                         f"got {tuple(int(v) for v in c.shape)}")
    n_ex, n_t, n_obs = obs.shape
    inside = (np.arange(n_t)[None, :] < n_t_e[:, None])[:, :, None]
    set_ = c != 0
    bad_flag = set_ & (c != -1) & (c != 1)
    bad_end = set_ & ~inside
    bad_nan = set_ & np.isnan(obs)
    bad = bad_flag | bad_end | bad_nan
    if bad.any():
        e, i, k = (int(v) for v in np.unravel_index(int(np.flatnonzero(bad)[0]), c.shape))
        where = f"row {e}, time {i}, output {k}"
        if bad_flag[e, i, k]:
            v = c[e, i, k]
            raise ValueError(f"censor_layout: censor holds the flag {int(v) if v == int(v) else v} at {where} "
                             "(0: measured, -1: at or below obs, +1: at or above obs)")
        if bad_end[e, i, k]:
            raise ValueError(f"censor_layout: censor flags a value past the end of its row at {where}")
        raise ValueError(f"censor_layout: censor flags a value that was not measured (obs is NaN) at {where}")
    seen = ~np.isnan(obs) & inside
    return {"quantified": (seen & ~set_).sum(axis=1).astype(np.int64), "censored": set_.sum(axis=1).astype(np.int64)}


def censor_excess(z):
    """x = -log Phi(z), the excess of a censored term over its floor 0 (include/smc_hip.h: smc_set_model_user7), as the kernels
    form it (csrc/user_censor.h): z > 0: -log1p(-erfc(z / sqrt 2) / 2); z <= 0: z^2 / 2 - log(erfcx(-z / sqrt 2) / 2).  Accurate
    in both tails, >= 0 in floating point, finite out to z = -1e154 and exactly 0 from z = 40 on; NaN for NaN."""
    import numpy as np
    from scipy.special import erfc, erfcx
    z = np.asarray(z, dtype=np.float64)
    y = z / np.sqrt(2.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        right = -np.log1p(-0.5 * erfc(np.where(z > 0, y, 1.0)))
        zl = np.where(z > 0, 0.0, z)
        left = 0.5 * (zl * zl) - np.log(0.5 * erfcx(-zl / np.sqrt(2.0)))
    return np.where(z > 0, right, np.where(np.isnan(z), np.nan, left))


def censored_loglik(pred, t, obs, censor, theta, noise, obs_scale=None):
    """The likelihood of a noise model with censored observations (include/smc_hip.h: smc_set_model_user7) applied to given model
    outputs - its executable definition.  Arguments as noise_loglik's, and censor (n_ex, n_t, n_obs) by censor_layout's rules.
    With sd as in noise_loglik:
        logL = sum over quantified [-1/2 log(2 pi) - log sd - (obs - f)^2 / (2 sd^2)] + sum over censored log Phi(z),
        z = (obs - f) / sd  (flag -1, the true value is <= obs),   z = (f - obs) / sd  (flag +1, the true value is >= obs),
    log Phi(z) = -censor_excess(z); -inf where any a_k <= 0 or any b_k < 0.  Returns (n,).  With every flag 0 it is noise_loglik's
    array exactly."""
    import numpy as np
    obs = np.asarray(obs, dtype=np.float64)
    c = np.asarray(censor)
    censor_layout(t, obs, c)
    quantified = noise_loglik(pred, t, np.where(c != 0, np.nan, obs), theta, noise, obs_scale)
    if not np.any(c != 0):
        return quantified
    pred = np.asarray(pred, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    n_obs = obs.shape[2]
    ai, af, pi, pf = noise_layout(noise, n_obs, theta.shape[1])
    scale = np.ones(n_obs) if obs_scale is None else np.asarray(obs_scale, dtype=np.float64).reshape(n_obs)
    a = np.where(ai >= 0, theta[:, np.maximum(ai, 0)], af[None, :])
    b = np.zeros_like(a) if pi is None else np.where(pi >= 0, theta[:, np.maximum(pi, 0)], pf[None, :])
    cens = (c != 0)[None]
    f = np.where(cens, pred, 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sd = np.sqrt((a * scale)[:, None, None, :] ** 2 + (b[:, None, None, :] * f) ** 2)
        z = np.where(cens, np.where((c < 0)[None], obs[None] - f, f - obs[None]) / sd, 0.0)
        term = np.where(cens, censor_excess(z), 0.0)
        lk = quantified - term.sum(axis=(1, 2, 3))
    return np.where(np.all(a > 0, axis=1) & np.all(b >= 0, axis=1), lk, -np.inf)


def censor_data(values, lower=None, upper=None):
    """Pseudo-data with limits of quantification: values (..., n_obs); lower, upper: a limit per output ((n_obs,) or a scalar; None
    or NaN: no limit).  Returns (obs, censor) of values' shape: where a value falls below its lower limit obs holds that limit and
    censor -1, above its upper limit the upper limit and +1, else the value and 0; NaN (not measured) stays NaN with flag 0."""
    import numpy as np
    v = np.array(values, dtype=np.float64)
    n_obs = v.shape[-1]
    lim = lambda x: np.full(n_obs, np.nan) if x is None else np.broadcast_to(np.asarray(x, dtype=np.float64), (n_obs,))
    lo, hi = lim(lower), lim(upper)
    with np.errstate(invalid="ignore"):
        below, above = v < lo, v > hi
    obs = np.where(below, lo, np.where(above, hi, v))
    return obs, (above.astype(np.int8) - below.astype(np.int8))


# Count observations (include/smc_hip.h: COUNT OBSERVATIONS).  An SIR epidemic with weekly case counts: theta = (beta, gamma, b),
# cond = (N, I0); states S, I and the accumulator A of new infections, which a scheduled event resets at every report time - a data
# time equal to an event time sees the state before the jump, i.e. the week's incidence.  The one output is negative binomial with
# b = theta[2] estimated (noise={"additive": [("fixed", 1.0)], "proportional": [("param", 2)]}).
SIR_WEEKLY_CASES = r"""
__device__ const int smc_user_obs_family[] = {2};
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0] - cond[1]; y[1] = cond[1]; y[2] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    const double inf = theta[0] * y[0] * y[1] / cond[0];
    dydt[0] = -inf;
    dydt[1] = inf - theta[1] * y[1];
    dydt[2] = inf;
}
__device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out) { out[0] = y[2]; }
__device__ void smc_user_event(int j, double t, double *y, const double *theta, const double *cond) { y[2] = 0.0; }
"""

OBS_FAMILY_NAMES = {0: "Gaussian", 1: "Poisson", 2: "negative binomial"}


def obs_family(source):
    """The family list of a source (include/smc_hip.h: COUNT OBSERVATIONS), read as the library reads it (smc_user_obs_family):
    the integer literals of the initialiser list behind the first "smc_user_obs_family" that is followed by "[" - a comment or a
    use of the name is passed over.  Returns the entries as written (whether an entry is 0, 1 or 2 is count_layout's rule), None
    for a source without the name; raises ValueError, in the library's words, for a list that is not written as one."""
    import re
    name = "smc_user_obs_family"
    if name not in source:
        return None
    how = ("obs_family: smc_user_obs_family: the families are written as a list of the integers 0 (Gaussian), 1 (Poisson) or 2 "
           "(negative binomial) behind the first smc_user_obs_family[ of the source")
    m = re.search(name + r"[ \t]*\[", source)
    rest = source[m.start():] if m else source[source.index(name):]
    o, sc = rest.find("{"), rest.find(";")
    c = rest.find("}", o) if o >= 0 else -1
    if o < 0 or c < 0 or (0 <= sc < o):
        raise ValueError(how)
    body = rest[o + 1:c]
    if not re.fullmatch(r"\s*[+-]?\d+\s*(,\s*[+-]?\d+\s*)*,?\s*", body):
        raise ValueError(how)
    return [max(-1000, min(1000, int(v))) for v in re.findall(r"[+-]?\d+", body)]


def count_layout(t, obs, family, noise=None, obs_scale=None, censor=None, est_sigma=False, dim=None):
    """The rules of a model with count outputs (include/smc_hip.h: COUNT OBSERVATIONS), in NumPy, for t (n_ex, n_t) and obs (n_ex,
    n_t, n_obs) that obs_layout accepts (a 2-D obs: the one-output model, which has no count outputs) and flags that censor_layout
    accepts: family (obs_family's list; None: nothing to check) has one entry 0, 1 or 2 per output; a count output has obs_scale
    1, the additive entry ("fixed", 1.0), no proportional entry or ("fixed", 0.0) if Poisson and one (a parameter, or fixed > 0) if
    negative binomial; noise=None with est_sigma needs a Gaussian output; a finite value of a count output is a non-negative integer
    <= 2^53 and carries no censor flag.  Returns {"family": (n_obs,) int, "counts": (n_ex, n_obs) the values of the count outputs,
    "floor": (n_ex,) C_e, the sum of count_floor over the Poisson values}; raises ValueError, in the library's words
    (smc_user_count_check), for what the library refuses - the first offence in row-major order."""
    import numpy as np
    t = np.asarray(t, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    if family is None:
        return None
    fam = [int(v) for v in family]
    n_fam = len(fam)
    n_obs = obs.shape[2] if obs.ndim == 3 else 0
    if n_obs == 0:
        raise ValueError("count_layout: smc_user_obs_family: the name in a one-output source (n_obs = 0) - count outputs need the "
                         "multi-output source (smc_user_obs_vec, n_obs >= 1)")
    if n_fam != n_obs:
        raise ValueError(f"count_layout: smc_user_obs_family: {n_fam} entries for n_obs = {n_obs} outputs (one entry per output)")
    for k, f in enumerate(fam):
        if f not in (0, 1, 2):
            raise ValueError(f"count_layout: smc_user_obs_family: entry {f} of output {k} is none of 0 (Gaussian), 1 (Poisson), "
                             "2 (negative binomial)")
    n_t_e = obs_layout(t, obs)["n_t_e"]
    if censor is not None:
        censor_layout(t, obs, censor)
    ai = af = pi = pf = None
    if noise is not None:
        ai, af, pi, pf = noise_layout(noise, n_obs, int(dim) if dim is not None else 1 << 30)
    scale = None if obs_scale is None else np.asarray(obs_scale, dtype=np.float64).reshape(-1)
    for k, f in enumerate(fam):
        if f == 0:
            continue
        if scale is not None and scale[k] != 1.0:
            raise ValueError(f"count_layout: output {k}: the obs_scale of a count output must be 1")
        if ai is not None and not (ai[k] == -1 and af[k] == 1.0):
            raise ValueError(f"count_layout: output {k}: the additive entry of a count output must be fixed at 1 (it is not used)")
        has_b = pi is not None and not (pi[k] == -1 and pf[k] == 0.0)
        if f == 1 and has_b:
            raise ValueError(f"count_layout: output {k}: a Poisson output takes no proportional entry (absent, or fixed at 0)")
        if f == 2 and not has_b:
            raise ValueError(f"count_layout: output {k}: a negative-binomial output needs a proportional entry (its b_k: a "
                             "parameter, or fixed > 0)")
    if noise is None and est_sigma and 0 not in fam:
        raise ValueError("count_layout: est_sigma without a noise model and no Gaussian output: the last parameter would be a noise "
                         "level that nothing uses")
    n_ex, n_t = t.shape
    inside = (np.arange(n_t)[None, :] < n_t_e[:, None])[:, :, None]
    is_count = (np.asarray(fam) != 0)[None, None, :]
    seen = inside & is_count & ~np.isnan(obs)
    v = np.where(seen, obs, 0.0)
    neg, big, frac = seen & (v < 0), seen & (v > 2.0 ** 53), seen & (v != np.floor(v))
    flag = seen & (np.asarray(censor) != 0) if censor is not None else np.zeros_like(seen)
    bad = neg | big | frac | flag
    if bad.any():
        e, i, k = (int(x) for x in np.unravel_index(int(np.flatnonzero(bad)[0]), bad.shape))
        where = f" at row {e}, time {i}, output {k}"
        if neg[e, i, k]:
            raise ValueError("count_layout: obs holds a negative value on a count output" + where)
        if big[e, i, k]:
            raise ValueError("count_layout: obs holds a value above 2^53 on a count output" + where)
        if frac[e, i, k]:
            raise ValueError("count_layout: obs holds a value that is not an integer on a count output" + where)
        raise ValueError("count_layout: censor flags a value of a count output" + where + " (censored counts are not supported)")
    pois = seen & (np.asarray(fam) == 1)[None, None, :]
    return {"family": np.asarray(fam, dtype=np.int64), "counts": seen.sum(axis=1).astype(np.int64),
            "floor": np.where(pois, count_floor(v), 0.0).sum(axis=(1, 2))}


def count_floor(y):
    """c(y) = gammaln(y + 1) - xlogy(y, y) + y: minus the log-probability of the saturated Poisson model at the count y, the floor
    of a Poisson term (log p = -c(y) - count_excess).  As written below y = 32, where nothing cancels yet; from there on by its
    Stirling series 1/2 log(2 pi y) + 1/(12 y) - 1/(360 y^3) + 1/(1260 y^5) - 1/(1680 y^7), whose next term is below 1e-16 - the
    three terms of the definition reach 1e7 at y = 1e6 and would leave c(y), a number below 10, with an error of 1e-9.  The
    library's host code (csrc/user_model.hip: count_floor) is the same."""
    import numpy as np
    from scipy.special import gammaln, xlogy
    y = np.asarray(y, dtype=np.float64)
    small = np.where(y < 32.0, y, 1.0)
    large = np.where(y < 32.0, 32.0, y)
    r = 1.0 / large
    r2 = r * r
    series = 0.5 * np.log(6.283185307179586 * large) + r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))))
    return np.where(y < 32.0, (gammaln(small + 1.0) - xlogy(small, small)) + small, series)


def count_bd0(x, m):
    """The deviance part of Loader's saddle-point form, bd0(x, m) = x log(x / m) + m - x >= 0 for x > 0 and m > 0, as the kernels
    form it (csrc/user_count.h: bd0), operation for operation.  With v = (x - m) / (x + m): where |x - m| < 0.1 (x + m) the series
    (x - m) v + 2 x (v^3 / 3 + v^5 / 5 + ... + v^19 / 19) - every term has one sign, nothing cancels, and the first term left out is
    below 1e-18 of the sum; elsewhere x L + (m - x) with L = log(x / m), or log x - log m for m < x / 2 (the same number, where
    x / m may overflow).  Exactly 0 at m = x."""
    import numpy as np
    x, m = np.asarray(x, dtype=np.float64), np.asarray(m, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = x - m
        s = x + m
        v = d / s
        v2 = v * v
        p = 1.0 / 19.0
        for c in (17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            p = p * v2 + 1.0 / c
        series = d * v + ((2.0 * x) * v) * (v2 * p)
        low = m < 0.5 * x
        l = np.where(low, np.log(x) - np.log(m), np.log(x / m))
        return np.where(np.abs(d) < 0.1 * s, series, x * l + (m - x))


def count_stirlerr(n):
    """The remainder of Stirling's formula, stirlerr(n) = gammaln(n + 1) - (n + 1/2) log n + n - 1/2 log(2 pi) for n > 0, as the
    kernels form it (csrc/user_count.h: stirlerr), operation for operation: as written up to n = 15 (its terms stay below 45, an
    absolute error of 1e-14), above by the series 1/(12 n) - 1/(360 n^3) + 1/(1260 n^5) - 1/(1680 n^7) + 1/(1188 n^9) -
    691/(360360 n^11) + 1/(156 n^13), whose next term is below 1e-19 at n = 15."""
    import numpy as np
    from scipy.special import gammaln
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        small = np.where(n <= 15.0, n, 1.0)
        direct = ((gammaln(small + 1.0) - (small + 0.5) * np.log(small)) + small) - 0.9189385332046727
        r = 1.0 / np.where(n <= 15.0, 16.0, n)
        r2 = r * r
        series = r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0 - r2 * (1.0 / 1188.0 - r2 * (
            691.0 / 360360.0 - r2 * (1.0 / 156.0)))))))
    return np.where(n <= 15.0, direct, series)


def count_excess(y, mu, b, family):
    """x >= 0, the excess of a count term over its floor (include/smc_hip.h: COUNT OBSERVATIONS), as the kernels form it
    (csrc/user_count.h), operation for operation.  y the count, mu the model's mean, b the overdispersion, family 1 (Poisson: log
    p = -count_floor(y) - x, b is not used) or 2 (negative binomial: log p = -x).  Arrays broadcast; family is one number.  Both
    are written in Loader's saddle-point form (count_bd0, count_stirlerr), in which no large numbers cancel:
      Poisson:  x = bd0(y, mu);  x = mu for y = 0.
      negative binomial, u = b^2 mu, phi = 1 / b^2, n = phi + y, n p = n / (1 + u), n q = mu (1 + b^2 y) / (1 + u), L = log1p(b^2 y):
                x = L - [stirlerr(n) - stirlerr(phi) - stirlerr(y) - bd0(phi, n p) - bd0(y, n q)] - 1/2 [L - log(2 pi y)];
                y = 0: phi log1p(u).
    Both: clamped at >= 0; NaN for mu NaN; +inf for mu < 0, mu = +inf, or mu = 0 with y > 0; 0 for mu = 0 with y = 0.  A negative
    binomial b that is not > 0 gives 0 (such parameters have logL = -inf, which count_loglik decides)."""
    import numpy as np
    family = int(family)
    if family not in (1, 2):
        raise ValueError(f"count_excess: family {family} is neither 1 (Poisson) nor 2 (negative binomial)")
    y, mu, b = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(b, dtype=np.float64))
    inf_case = (mu < 0) | (mu == np.inf) | ((mu == 0) & (y > 0))
    safe_mu = np.where(inf_case | np.isnan(mu) | (mu == 0), 1.0, mu)
    safe_y = np.where(y > 0, y, 1.0)
    with np.errstate(all="ignore"):
        if family == 1:
            x = count_bd0(safe_y, safe_mu)
            x = np.where(y == 0, mu, x)
        else:
            ok_b = b > 0
            b2 = np.where(ok_b, b * b, 1.0)
            phi = 1.0 / b2
            u = b2 * safe_mu
            l1 = np.log1p(u)
            pl = phi * l1
            n = phi + safe_y
            den = 1.0 + u
            b2y = b2 * safe_y
            ly = np.log1p(b2y)
            n_p = n / den
            n_q = safe_mu * ((1.0 + b2y) / den)
            lc = (((count_stirlerr(n) - count_stirlerr(phi)) - count_stirlerr(safe_y)) - count_bd0(phi, n_p)) - count_bd0(safe_y, n_q)
            x = (ly - lc) - 0.5 * (ly - np.log(6.283185307179586 * safe_y))
            x = np.where(y == 0, np.where(mu == 0, 0.0, pl), x)
        x = np.where(x < 0, 0.0, x)
        x = np.where(inf_case, np.inf, x)
        if family == 2:
            x = np.where(ok_b, x, 0.0)
            x = np.where(np.isnan(mu) & ok_b, np.nan, x)
        else:
            x = np.where(np.isnan(mu), np.nan, x)
    return x


def count_loglik(pred, t, obs, theta, family, noise, obs_scale=None, censor=None):
    """The likelihood of a model with count outputs (include/smc_hip.h: COUNT OBSERVATIONS) applied to given model outputs - its
    executable definition.  Arguments as censored_loglik's (censor None: no flags) and family, one entry per output: 0 a Gaussian
    output with its terms of noise_loglik / censored_loglik, 1 Poisson, 2 negative binomial with the output's proportional entry
    b_k as overdispersion (variance mu + (b_k mu)^2).  With mu = pred:
        logL = [the Gaussian outputs' logL] - sum over Poisson values [count_floor(y) + count_excess(y, mu, 0, 1)]
               - sum over negative-binomial values count_excess(y, mu, b_k, 2);
    -inf where any a_k <= 0, any b_k < 0, or b_k <= 0 on a negative-binomial output.  noise=None is not accepted here: give the
    specification the library forms (count outputs ("fixed", 1.0)).  Returns (n,).  With every family 0 it is censored_loglik's
    (noise_loglik's without flags) array exactly."""
    import numpy as np
    obs = np.asarray(obs, dtype=np.float64)
    pred = np.asarray(pred, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    n_obs = obs.shape[2]
    fam = np.asarray([int(v) for v in family], dtype=np.int64)
    gauss = lambda o: (noise_loglik(pred, t, o, theta, noise, obs_scale) if censor is None
                       else censored_loglik(pred, t, o, censor, theta, noise, obs_scale))
    if not np.any(fam != 0):
        if fam.shape != (n_obs,):
            raise ValueError(f"count_loglik: smc_user_obs_family: {fam.size} entries for n_obs = {n_obs} outputs (one entry per output)")
        return gauss(obs)
    count_layout(t, obs, fam, noise, obs_scale, censor, dim=theta.shape[1])
    lk = gauss(np.where((fam != 0)[None, None, :], np.nan, obs))       # a_k > 0 and b_k >= 0 are decided here
    ai, af, pi, pf = noise_layout(noise, n_obs, theta.shape[1])
    b = np.zeros((theta.shape[0], n_obs)) if pi is None else np.where(pi >= 0, theta[:, np.maximum(pi, 0)], pf[None, :])
    seen = ~np.isnan(obs) & ~np.isnan(np.asarray(t, dtype=np.float64))[:, :, None]
    valid = np.ones(theta.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in np.flatnonzero(fam != 0):
            s = seen[:, :, k]
            y = np.where(s, obs[:, :, k], 0.0)
            mu = np.where(s[None], pred[:, :, :, k], 0.0)
            x = count_excess(y[None], mu, b[:, k][:, None, None], int(fam[k]))
            if fam[k] == 1:
                x = x + count_floor(y)[None]
            else:
                valid &= b[:, k] > 0
            lk = lk - np.where(s[None], x, 0.0).sum(axis=(1, 2))
    return np.where(valid, lk, -np.inf)


def input_layout(in_t, in_u, n_ex):
    """The data rules of a model's time-varying inputs (include/smc_hip.h: smc_set_model_user5), in NumPy: in_t (n_ex, n_knot) knot
    times, a row by the row rules of obs_layout's t - a strictly increasing finite run of at least one knot, possibly followed by
    NaN only; in_u (n_ex, n_knot, n_in) the values of n_in = 1 .. 8 inputs at the knots ((n_ex, n_knot) for one input), finite at a
    row's finite knots - with every slope between neighbours finite - and ignored past them; n_knot <= 4096.  Returns the knots
    per row, (n_ex,) int; raises ValueError, in the library's words (smc_user_input_check), for inputs the library refuses."""
    import numpy as np
    t = np.asarray(in_t, dtype=np.float64)
    u = np.asarray(in_u, dtype=np.float64)
    if u.ndim == 2 and t.ndim == 2:
        u = u.reshape(u.shape + (1,))
    n_ex = int(n_ex)
    if t.ndim != 2 or u.ndim != 3 or u.shape[:2] != t.shape or t.shape[0] != n_ex:
        raise ValueError(f"input_layout: in_t must be ({n_ex}, n_knot) and in_u ({n_ex}, n_knot, n_in), got {t.shape} and {u.shape}")
    n_knot, n_in = t.shape[1], u.shape[2]
    if not 1 <= n_in <= 8:
        raise ValueError(f"input_layout: n_in = {n_in} outside 1 .. 8 (SMC_USER_MAX_INPUTS)")
    if n_knot < 1:
        raise ValueError(f"input_layout: n_knot = {n_knot}: a row needs at least one knot")
    if n_knot > 4096:
        raise ValueError(f"input_layout: n_knot = {n_knot} above the knot capacity 4096 (SMC_USER_MAX_KNOTS)")
    if n_ex < 1:
        raise ValueError(f"input_layout: n_ex = {n_ex}: no experiment")
    m = np.zeros(n_ex, dtype=np.int64)
    for e in range(n_ex):
        nan = np.isnan(t[e])
        k = int(nan.argmax()) if nan.any() else n_knot
        late = np.flatnonzero(~nan[k:])
        if late.size:
            raise ValueError(f"input_layout: row {e} of in_t has a NaN knot before a number at knot {k + late[0]} "
                             "(only a trailing run of NaN may shorten a row)")
        if k == 0:
            raise ValueError(f"input_layout: row {e} of in_t has no finite knot")
        for i in range(k):
            if not np.isfinite(t[e, i]):
                raise ValueError(f"input_layout: row {e} of in_t holds an infinite knot at knot {i}")
            if i > 0 and not t[e, i] > t[e, i - 1]:
                raise ValueError(f"input_layout: row {e} of in_t is not strictly increasing at knot {i}")
        with np.errstate(over="ignore", invalid="ignore"):
            steep = np.zeros((k, n_in), dtype=bool)
            steep[1:] = ~np.isfinite(np.diff(u[e, :k], axis=0) / np.diff(t[e, :k])[:, None])
        for i in range(k):
            for j in range(n_in):
                if not np.isfinite(u[e, i, j]):
                    raise ValueError(f"input_layout: row {e} of in_u is not finite at knot {i} of input {j}")
                if steep[i, j]:
                    raise ValueError(f"input_layout: row {e} of in_u has a slope that overflows at knot {i} of input {j}")
        m[e] = k
    return m


def event_layout(t, ev_t, ev_v=None):
    """The data rules of a model's scheduled events (include/smc_hip.h: smc_set_model_user6), in NumPy: t (n_ex, n_t) the data
    times; ev_t (n_ex, n_ev) event times, every row a strictly increasing finite run - it may be empty - possibly followed by NaN
    only, every finite event time later than the row's first time t[e][0]; ev_v (n_ex, n_ev, n_val) the n_val = 0 .. 8 numbers of
    every event (None for n_val = 0), finite at a row's finite events and ignored past them; n_ev = 1 .. 256.  Which events fire
    is the solve's matter: those with t[e][0] < tau < the row's last finite time.  Returns the events per row, (n_ex,) int; raises
    ValueError, in the library's words (smc_user_event_check), for events the library refuses."""
    import numpy as np
    t = np.asarray(t, dtype=np.float64)
    et = np.asarray(ev_t, dtype=np.float64)
    if t.ndim != 2 or et.ndim != 2 or et.shape[0] != t.shape[0]:
        raise ValueError(f"event_layout: t must be (n_ex, n_t) and ev_t (n_ex, n_ev), got {t.shape} and {et.shape}")
    n_ex, n_ev = et.shape
    ev = np.zeros((n_ex, n_ev, 0)) if ev_v is None else np.asarray(ev_v, dtype=np.float64)
    if ev.ndim != 3 or ev.shape[:2] != et.shape:
        raise ValueError(f"event_layout: ev_v must be ({n_ex}, {n_ev}, n_val) or None, got {ev.shape}")
    n_val = ev.shape[2]
    if n_ev < 1:
        raise ValueError(f"event_layout: n_ev = {n_ev}: a model with events needs room for at least one")
    if n_ev > 256:
        raise ValueError(f"event_layout: n_ev = {n_ev} above the event capacity 256 (SMC_USER_MAX_EVENTS)")
    if n_val > 8:
        raise ValueError(f"event_layout: n_val = {n_val} outside 0 .. 8 (SMC_USER_MAX_EVENT_VALUES)")
    if n_ex < 1:
        raise ValueError(f"event_layout: n_ex = {n_ex}: no experiment")
    if t.shape[1] < 1:
        raise ValueError(f"event_layout: n_t = {t.shape[1]}: no time")
    m = np.zeros(n_ex, dtype=np.int64)
    for e in range(n_ex):
        nan = np.isnan(et[e])
        k = int(nan.argmax()) if nan.any() else n_ev
        late = np.flatnonzero(~nan[k:])
        if late.size:
            raise ValueError(f"event_layout: row {e} of ev_t has a NaN event time before a number at event {k + late[0]} "
                             "(only a trailing run of NaN may shorten a row)")
        for i in range(k):
            if not np.isfinite(et[e, i]):
                raise ValueError(f"event_layout: row {e} of ev_t holds an infinite event time at event {i}")
            if i > 0 and not et[e, i] > et[e, i - 1]:
                raise ValueError(f"event_layout: row {e} of ev_t is not strictly increasing at event {i}")
            if not et[e, i] > t[e, 0]:
                raise ValueError(f"event_layout: row {e} of ev_t is not later than the row's first time t[e][0] at event {i}")
        for i in range(k):
            for j in range(n_val):
                if not np.isfinite(ev[e, i, j]):
                    raise ValueError(f"event_layout: row {e} of ev_v is not finite at event {i}, value {j}")
        m[e] = k
    return m


def input_value(tk, u, t):
    """smc_input (include/smc_hip.h: smc_set_model_user5) for one row and one input - its executable definition: tk (m,) strictly
    increasing finite knots, u (m,) values, t any shape.  u[0] for t <= tk[0], u[m-1] for t >= tk[m-1], else with j the last knot
    <= t:  u[j] + s_j (t - tk[j]),  s_j = (u[j+1] - u[j]) / (tk[j+1] - tk[j]),  clamped to [min(u[j], u[j+1]), max(u[j], u[j+1])] -
    what np.interp(t, tk, u) computes, up to rounding.  Equal to u[j] at t == tk[j]; never outside the bracket."""
    import numpy as np
    tk = np.asarray(tk, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    t = np.asarray(t, dtype=np.float64)
    m = tk.size
    if m < 1 or u.size != m:
        raise ValueError(f"input_value: tk and u must hold the same number (>= 1) of entries, got {tk.size} and {u.size}")
    j = np.clip(np.searchsorted(tk, t, side="right") - 1, 0, m - 1)          # the last knot <= t
    j1 = np.minimum(j + 1, m - 1)
    s = np.concatenate([np.diff(u) / np.diff(tk), [0.0]])
    u0, u1 = u[j], u[j1]
    v = u0 + s[j] * np.maximum(t - tk[j], 0.0)
    return np.minimum(np.maximum(v, np.minimum(u0, u1)), np.maximum(u0, u1))


def design_layout(t_new, cond_new, n_cond):
    """The rules of a prediction design (include/smc_hip.h: smc_user_predict_at), in NumPy: t_new (n_ex_new, n_t_new) by the row
    rules of obs_layout - a strictly increasing run of finite times, possibly followed by NaN only; t_new[e][0] is the initial
    time - and cond_new (n_ex_new, n_cond) finite numbers (None only for n_cond = 0).  Returns n_t_e (n_ex_new,) int, the finite
    times per row; raises ValueError, in obs_layout's words where the rule is the same (a row "of t" is then a row of t_new), for a design the library refuses."""
    import numpy as np
    t = np.asarray(t_new, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"design_layout: t_new must be (n_ex_new, n_t_new), got {t.shape}")
    n_ex = t.shape[0]
    n_cond = int(n_cond)
    if cond_new is None:
        if n_cond != 0:
            raise ValueError(f"design_layout: cond_new must be ({n_ex}, {n_cond}), got None")
    else:
        c = np.asarray(cond_new, dtype=np.float64)
        if c.shape != (n_ex, n_cond) and not (c.ndim == 1 and n_cond == 1 and c.shape == (n_ex,)):
            raise ValueError(f"design_layout: cond_new must be ({n_ex}, {n_cond}), got {c.shape}")
        if not np.all(np.isfinite(c)):
            raise ValueError("design_layout: cond_new must be finite")
    try:
        return obs_layout(t, np.full(t.shape + (1,), np.nan))["n_t_e"]
    except ValueError as e:
        raise ValueError(str(e).replace("obs_layout: ", "design_layout: ", 1)) from None


def quantile_ranks(m, probs):
    """Which order statistics a quantile is made of (include/smc_hip.h: smc_user_predict_summary): for m >= 1 sorted values and
    probabilities in [0, 1] returns (lo, hi, frac) with lo = floor((m - 1) q), hi = ceil((m - 1) q) - the elements
    np.quantile(method="lower" / "higher") picks - and frac the weight of the upper one in the linear rule,
    quantile = x[lo] + (x[hi] - x[lo]) * frac.  m may be an array (one count per cell): the results broadcast m against probs."""
    import numpy as np
    m = np.asarray(m, dtype=np.int64)
    q = np.asarray(probs, dtype=np.float64)
    if np.any(m < 1):
        raise ValueError("quantile_ranks: m must be >= 1")
    if not np.all((q >= 0) & (q <= 1)):
        raise ValueError("quantile_ranks: probabilities must lie in [0, 1]")
    pos = (m - 1).astype(np.float64) * q
    lo = np.minimum(np.floor(pos).astype(np.int64), m - 1)
    hi = np.minimum(np.where(lo.astype(np.float64) < pos, lo + 1, lo), m - 1)
    return lo, hi, pos - lo.astype(np.float64)


def linear_quantile(lower, upper, frac):
    """The linear rule between two order statistics, from whichever of them is nearer: lower + (upper - lower) * frac for
    frac < 1/2, upper - (upper - lower) * (1 - frac) from there on - NumPy's own form (np.quantile, method="linear").  One
    formula from `lower` alone is off by an ulp of the larger element where the result is small next to it: between -3 and 0
    at frac = 1 - 2**-53 it gives -4.4e-16 for -3.3e-16.  Never outside [lower, upper]; NaN where an argument is."""
    import numpy as np
    lower, upper, frac = np.broadcast_arrays(np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64),
                                             np.asarray(frac, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        d = upper - lower
        q = np.where(frac >= 0.5, upper - d * (1.0 - frac), lower + d * frac)
        q = np.where(upper == lower, lower, q)
        return np.minimum(np.maximum(q, lower), upper)       # rounding cannot leave the bracket


# ---- pointwise log-likelihood, WAIC and PIT (include/smc_hip.h: smc_user_pointwise, smc_user_pointwise_summary) --------------------
def _pointwise_parts(pred, t, obs, theta, noise, obs_scale, censor, family):
    """What pointwise_loglik and pointwise_pit share: (pred, obs, seen, a, b, scale, flag, fam, valid) with a, b (n, n_obs) the
    particles' noise parameters and valid (n,) whether they allow a likelihood at all."""
    import numpy as np
    pred = np.asarray(pred, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    if obs.ndim == 2:                                   # the one-output model: one cell per time
        obs = obs[:, :, None]
    if pred.ndim == 3:
        pred = pred[:, :, :, None]
    n_obs = obs.shape[2]
    if pred.shape[1:] != obs.shape or pred.shape[0] != theta.shape[0]:
        raise ValueError(f"pointwise_loglik: pred must be (n, n_ex, n_t, n_obs) = {(theta.shape[0],) + obs.shape}, got {pred.shape}")
    ai, af, pi, pf = noise_layout(noise, n_obs, theta.shape[1])
    scale = np.ones(n_obs) if obs_scale is None else np.asarray(obs_scale, dtype=np.float64).reshape(n_obs)
    fam = np.zeros(n_obs, dtype=np.int64) if family is None else np.asarray([int(v) for v in family], dtype=np.int64)
    flag = np.zeros(obs.shape, dtype=np.int8) if censor is None else np.asarray(censor)
    if censor is not None:
        censor_layout(t, obs, flag)
    if np.any(fam != 0):
        count_layout(t, obs, fam, noise, obs_scale, censor, dim=theta.shape[1])
    a = np.where(ai >= 0, theta[:, np.maximum(ai, 0)], af[None, :])
    b = np.zeros_like(a) if pi is None else np.where(pi >= 0, theta[:, np.maximum(pi, 0)], pf[None, :])
    seen = ~np.isnan(obs) & ~np.isnan(np.asarray(t, dtype=np.float64))[:, :, None]
    with np.errstate(invalid="ignore"):
        valid = np.all(a > 0, axis=1) & np.all(b >= 0, axis=1) & np.all((b > 0) | (fam != 2)[None, :], axis=1)
    return pred, obs, seen, a, b, scale, flag, fam, valid


def pointwise_loglik(pred, t, obs, theta, noise, obs_scale=None, censor=None, family=None):
    """The log-likelihood term of every cell (experiment e, time i, output k) for every particle - the executable definition of
    smc_user_pointwise (include/smc_hip.h), written with the functions that define the sums (noise_layout, censor_excess,
    count_floor, count_excess), operation for operation as the kernels form it (csrc/pointwise_kernels.hip: pw_term).  Arguments as
    count_loglik's: pred (n, n_ex, n_t, n_obs) model outputs f, t (n_ex, n_t), obs (n_ex, n_t, n_obs), theta (n, dim), noise the
    specification (the sigma rule is {"additive": [("param", dim - 1)] * n_obs}, or ("fixed", sigma)), censor and family optional.
    A 2-D obs with a 3-D pred is the one-output model.  A cell is observed when obs is finite at a finite time of its row; censored
    values are observed.  With sd^2 = (a_k s_k)^2 + (b_k f)^2 and r = obs - f the term l is
        Gaussian, quantified   -1/2 log(2 pi) - 1/2 log sd^2 - r^2 / (2 sd^2)
        censored (flag -1, +1) -censor_excess(z),  z = r / sd and -r / sd
        Poisson                -(count_floor(y) + count_excess(y, f, 0, 1))
        negative binomial      -count_excess(y, f, b_k, 2)
    NaN where the cell is not observed or f is NaN (a failed solve, or the model's own NaN); -inf in every other observed cell of a
    particle whose parameters make logL -inf (any a_k <= 0, any b_k < 0, b_k <= 0 on a negative-binomial output).  Returns
    (n, n_ex, n_t, n_obs); its nansum over the cells is noise_loglik / censored_loglik / count_loglik up to the order of the sum."""
    import numpy as np
    pred, obs, seen, a, b, scale, flag, fam, valid = _pointwise_parts(pred, t, obs, theta, noise, obs_scale, censor, family)
    f = np.where(seen[None], pred, 0.0)
    y = np.where(seen, obs, 0.0)
    with np.errstate(all="ignore"):
        sd2 = (a * scale)[:, None, None, :] ** 2 + (b[:, None, None, :] * f) ** 2
        r = y[None] - f
        ll = -0.5 * np.log(2 * np.pi) - 0.5 * np.log(sd2) - r * r / (2 * sd2)
        cens = (flag != 0)[None]
        z = np.where((flag < 0)[None], r, -r) / np.sqrt(sd2)
        ll = np.where(cens, -censor_excess(np.where(cens, z, 0.0)), ll)
        for k in np.flatnonzero(fam != 0):
            yk, fk = y[None, :, :, k], f[:, :, :, k]
            if fam[k] == 1:
                ll[..., k] = -(count_floor(yk) + count_excess(yk, fk, 0.0, 1))
            else:
                ll[..., k] = -count_excess(yk, fk, np.where(valid, b[:, k], 1.0)[:, None, None], 2)
    ll = np.where(valid[:, None, None, None], ll, -np.inf)
    return np.where(seen[None] & ~np.isnan(pred), ll, np.nan)


def pointwise_pit(pred, t, obs, theta, noise, obs_scale=None, censor=None, family=None):
    """The probability integral transform of every quantified Gaussian value under the equally weighted particles - the definition
    of smc_user_pointwise_summary's pit: per observed cell with flag 0 on a Gaussian output
        pit = sum Phi((obs - f) / sd) / n_pit,   Phi(z) = erfc(-z / sqrt 2) / 2,
    over the n_pit particles with a finite f and valid noise parameters (n_pit = 0: NaN); NaN on every other cell - the PIT of a
    censored value is not formed, that of a count comes from replicated draws instead of a CDF (count_pit).  Arguments as pointwise_loglik's; returns
    (n_ex, n_t, n_obs).  A calibrated model has PIT values uniform on (0, 1) over the cells."""
    import numpy as np
    from scipy.special import erfc
    pred, obs, seen, a, b, scale, flag, fam, valid = _pointwise_parts(pred, t, obs, theta, noise, obs_scale, censor, family)
    cell = seen & (flag == 0) & (fam == 0)[None, None, :]
    use = cell[None] & np.isfinite(pred) & valid[:, None, None, None]
    f = np.where(use, pred, 0.0)
    with np.errstate(all="ignore"):
        sd2 = (a * scale)[:, None, None, :] ** 2 + (b[:, None, None, :] * f) ** 2
        z = (np.where(seen, obs, 0.0)[None] - f) / np.sqrt(sd2)
        phi = np.where(use, 0.5 * erfc(-z / np.sqrt(2.0)), 0.0)
        pit = phi.sum(axis=0) / use.sum(axis=0)
    return np.where(cell, pit, np.nan)


COUNT_PIT_TAG = 0x504954      # the Philox tag of the PIT's replicated counts (csrc/count_draw.h) and the second word of count_pit's generator


def count_pit(below, equal, n, seed=0):
    """The randomised PIT of count observations from the counts of HipEngine.pointwise_summary(count_pit=True): per cell
        (below + v_c equal) / n,   v_c uniform on [0, 1), one per cell from np.random.default_rng([seed, 0x504954]).random(shape),
    with below = #{replicated counts < y}, equal = #{= y} over the n particles that count; n = 0 gives NaN.  below / n estimates
    F(y - 1) and equal / n the mass at y, so this is the value u = F(y - 1) + v (F(y) - F(y - 1)) that is uniform on (0, 1) under a
    calibrated model (Smith 1985; Czado, Gneiting & Held 2009) - the mid-point v = 1/2 is not, for small counts."""
    import numpy as np
    below, equal, n = (np.asarray(x) for x in (below, equal, n))
    v = np.random.default_rng([int(seed), COUNT_PIT_TAG]).random(np.shape(n))
    with np.errstate(all="ignore"):
        u = (below.astype(np.float64) + v * equal.astype(np.float64)) / n.astype(np.float64)
    return np.where(n > 0, u, np.nan)


def count_pit_fill(pit, below, equal, n, family, seed=0):
    """What count_pit=True adds to a pointwise summary, from the Gaussian cells' pit (..., n_obs) and the counts: {"pit_below",
    "pit_equal", "pit_n", "pit_lower" = below / n, "pit_upper" = (below + equal) / n, "pit"}.  On the outputs whose family is a
    count, pit is count_pit(...) and lower / upper the two estimates (NaN where n = 0); on every other output pit stays and
    lower = upper = pit.  family: the list of the source (obs_family), None: no count output."""
    import numpy as np
    pit = np.asarray(pit, dtype=np.float64)
    below, equal, n = (np.asarray(x, dtype=np.int64) for x in (below, equal, n))
    is_count = np.zeros(pit.shape, dtype=bool)
    if family is not None:
        is_count[..., np.asarray(family) != 0] = True
    with np.errstate(all="ignore"):
        nf = n.astype(np.float64)
        lower = np.where(n > 0, below / nf, np.nan)
        upper = np.where(n > 0, (below + equal) / nf, np.nan)
    return {"pit_below": below, "pit_equal": equal, "pit_n": n, "pit_lower": np.where(is_count, lower, pit),
            "pit_upper": np.where(is_count, upper, pit), "pit": np.where(is_count, count_pit(below, equal, n, seed), pit)}


def pit_histogram(lower, upper, bins=10):
    """The non-randomised PIT histogram of Czado, Gneiting & Held (2009) for counts, and the ordinary one for continuous values:
    per cell F_c(u) = 0 for u <= lower, (u - lower) / (upper - lower) in between, 1 for u >= upper (lower = upper: the step at that
    value, a continuous observation's PIT); the result is the mean of F_c over the cells with finite lower and upper, differenced
    over the `bins` equal bins of [0, 1]: heights that sum to 1, each 1 / bins under a calibrated model.  No cell: NaN."""
    import numpy as np
    lower, upper = np.asarray(lower, dtype=np.float64).reshape(-1), np.asarray(upper, dtype=np.float64).reshape(-1)
    use = np.isfinite(lower) & np.isfinite(upper)
    lo, up = lower[use][:, None], upper[use][:, None]
    if lo.size == 0:
        return np.full(int(bins), np.nan)
    edges = np.linspace(0.0, 1.0, int(bins) + 1)[None, :]
    with np.errstate(all="ignore"):
        ramp = np.clip((edges - lo) / (up - lo), 0.0, 1.0)
    F = np.where(up > lo, ramp, (edges >= lo).astype(np.float64))
    F[:, 0], F[:, -1] = 0.0, 1.0      # the whole mass lies in [0, 1]: a step at 0 belongs to the first bin
    return np.diff(F.mean(axis=0))


def pointwise_finish(stats):
    """lpd = max + log(sum_exp / n) and var = m2 / (n - 1) added to raw statistics {"n", "max", "sum_exp", "mean", "m2"[, "pit"]}:
    n = 0 gives NaN in both, n = 1 var NaN, max = -inf lpd -inf; everything else is what the expressions give."""
    import numpy as np
    out = dict(stats)
    n = np.asarray(out["n"], dtype=np.int64)
    nf = n.astype(np.float64)
    with np.errstate(all="ignore"):
        lpd = out["max"] + np.log(out["sum_exp"] / nf)
        lpd = np.where(np.isneginf(out["max"]), -np.inf, lpd)
        out["lpd"] = np.where(n == 0, np.nan, lpd)
        out["var"] = np.where(n >= 2, out["m2"] / (nf - 1.0), np.nan)
    return out


def pointwise_stats(ll):
    """Per cell the statistics of the terms ll (n, ...) over the particles whose term is not NaN (-inf counts) - what
    smc_user_pointwise_summary forms on the device: {"n", "max", "sum_exp" = sum exp(l - max), "mean" = sum l / n, "m2" = sum
    (l - mean)^2 (two-pass), "lpd" = max + log(sum_exp / n), "var" = m2 / (n - 1)}, each of ll's shape without the first axis.
    n = 0: NaN everywhere except n; n = 1: var NaN; max = -inf: lpd -inf; everything else is whatever these expressions give
    under errstate(all="ignore") (a -inf term next to finite ones: mean -inf, m2 NaN)."""
    import numpy as np
    ll = np.asarray(ll, dtype=np.float64)
    ok = ~np.isnan(ll)
    n = ok.sum(axis=0).astype(np.int64)
    nf = n.astype(np.float64)
    with np.errstate(all="ignore"):
        mx = np.where(n > 0, np.max(np.where(ok, ll, -np.inf), axis=0), np.nan)
        sum_exp = np.where(n > 0, np.sum(np.where(ok, np.exp(ll - mx[None]), 0.0), axis=0), np.nan)
        mean = np.where(n > 0, np.sum(np.where(ok, ll, 0.0), axis=0) / nf, np.nan)
        d = np.where(ok, ll - mean[None], 0.0)
        m2 = np.where(n > 0, np.sum(d * d, axis=0), np.nan)
    return pointwise_finish({"n": n, "max": mx, "sum_exp": sum_exp, "mean": mean, "m2": m2})


def pointwise_merge(blocks):
    """The statistics of disjoint blocks of particles (dicts of pointwise_stats / HipEngine.pointwise_summary) merged in list order
    into those of all of them - what a run over several ranks returns (csrc/pointwise_reduce.h: merge is the same in C++): n adds
    and max is the larger; sum_exp is rescaled to the common max (a block whose max is -inf under a finite one adds 0); mean and
    m2 by Chan's update, delta = mean_b - mean_a: mean = mean_a + delta n_b / n, m2 = m2_a + m2_b + delta^2 n_a n_b / n (a -inf
    mean on either side: mean -inf, m2 NaN, as the expressions of the whole give); "pit", where the blocks carry it, weighted by
    n.  A block with n = 0 in a cell changes nothing there.  lpd and var are formed anew (pointwise_finish).  Where every block
    carries the count PIT's "pit_below", "pit_equal" and "pit_n" they add (integers: exact in any order); "pit" on count cells,
    "pit_lower" and "pit_upper" are then formed from the sums by count_pit_fill, which the caller applies (it knows the families
    and the seed; run_smc(pointwise={"count_pit": True}) does)."""
    import numpy as np
    blocks = list(blocks)
    if not blocks:
        raise ValueError("pointwise_merge: no block")
    with_pit = all("pit" in b for b in blocks)
    acc = {k: np.array(blocks[0][k], dtype=np.int64 if k == "n" else np.float64) for k in ("n", "max", "sum_exp", "mean", "m2")}
    if with_pit:
        acc["pit"] = np.array(blocks[0]["pit"], dtype=np.float64)
    with np.errstate(all="ignore"):
        for blk in blocks[1:]:
            na, nb = acc["n"].astype(np.float64), np.asarray(blk["n"], dtype=np.float64)
            n = na + nb
            ma, mb = acc["max"], np.asarray(blk["max"], dtype=np.float64)
            mx = np.where(mb > ma, mb, ma)

            def rescaled(s, m):
                return np.where(m == mx, s, np.where(np.isneginf(m), 0.0, s * np.exp(m - mx)))
            sum_exp = rescaled(acc["sum_exp"], ma) + rescaled(np.asarray(blk["sum_exp"], dtype=np.float64), mb)
            mean_a, mean_b = acc["mean"], np.asarray(blk["mean"], dtype=np.float64)
            delta = mean_b - mean_a
            mean = mean_a + delta * (nb / n)
            m2 = (acc["m2"] + np.asarray(blk["m2"], dtype=np.float64)) + (delta * delta) * (na * nb / n)
            low = np.isneginf(mean_a) | np.isneginf(mean_b)
            mean, m2 = np.where(low, -np.inf, mean), np.where(low, np.nan, m2)
            new = {"max": mx, "sum_exp": sum_exp, "mean": mean, "m2": m2}
            if with_pit:
                new["pit"] = (acc["pit"] * na + np.asarray(blk["pit"], dtype=np.float64) * nb) / n
            for k, v in new.items():      # an empty block changes nothing
                acc[k] = np.where(nb == 0, acc[k], np.where(na == 0, np.asarray(blk[k], dtype=np.float64), v))
            acc["n"] = acc["n"] + np.asarray(blk["n"], dtype=np.int64)
    out = pointwise_finish(acc)
    counts = ("pit_below", "pit_equal", "pit_n")
    if all(k in b for b in blocks for k in counts):
        for k in counts:
            out[k] = np.sum([np.asarray(b[k], dtype=np.int64) for b in blocks], axis=0)
    return out


def waic(stats):
    """WAIC (Watanabe; Vehtari, Gelman & Gabry 2017) from per-cell statistics, over the C cells with n >= 2 terms: lppd = sum lpd,
    p_waic = sum var, elpd_waic = lppd - p_waic, se = sqrt(C var_c(lpd_c - var_c, ddof=1)).  Returns {"lppd", "p_waic",
    "elpd_waic", "se", "n_cells", "pointwise": lpd - var per cell, NaN where the cell does not count}."""
    import numpy as np
    n = np.asarray(stats["n"])
    use = n >= 2
    lpd, var = np.asarray(stats["lpd"], dtype=np.float64), np.asarray(stats["var"], dtype=np.float64)
    with np.errstate(all="ignore"):
        point = np.where(use, lpd - var, np.nan)
        c = int(use.sum())
        lppd, p_waic = float(np.sum(lpd[use])), float(np.sum(var[use]))
        se = float(np.sqrt(c * np.var(point[use], ddof=1))) if c >= 2 else float("nan")
    return {"lppd": lppd, "p_waic": p_waic, "elpd_waic": lppd - p_waic, "se": se, "n_cells": c, "pointwise": point}
