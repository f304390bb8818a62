"""The models, data, exact solutions, chained-SciPy references and bounds of tests/test_user_events.py: linear models under
scheduled events (include/smc_hip.h: smc_set_model_user6, smc_user_event), whose solution is known exactly, so that the
run-time compiled kernels with the event machinery are held to |error| <~ atol + rtol |y| and not only to "the same numbers as
SciPy's solver" - in the manner of tests/forced_linear_model.py.

    python tests/dosed_model.py [case ...]     # prints, per case, the worst ratio and K = 2 x that ratio

The cases, each three experiments on one grid of N_T = 10 times (TIMES below):
  E1  RK45, 1 state:  y' = -th0 y, y(t0) = cond[0]; event j: y += value 0.  theta = (k, sigma).  Exact: a sum of exponentials.
  E2  RK45, 2 states, 2 outputs, with smc_user_cost: gut -> central -> out with rates th0, th1.  An event holds (amount, kind):
      kind 0 is y0 += th2 * amount (bioavailability: the jump depends on theta), kind 1 is y1 = 0 (a reset).  theta = (ka, ke,
      F, sigma).  Of the 320 particles 24 have a cost hint above 220 and 4 above 3700, so that events also fire in listed items
      and in the solo phase on wave-uniform operands.  Exact: Bateman's closed form per segment.
  E3  BDF with smc_user_jac: the same chain with th1 about 2e4 (stiff), events as E2.
  E4  RK45: tests/forced_linear_model.py's F1, y' = -th0 y + th1 u0(t) with its measured input, plus bolus events: inputs and
      events in one model.
Rows: row 0 has an event AT a data time (whose next representable neighbour is a data time too), two events between consecutive
data times and one event beyond the row's end; row 1 has no event at all; row 2 is ragged and its last finite time IS an event
time (that event never fires), and one of its events falls on a data time.

The exact solution (exact_outputs): between breakpoints the state moves by expm of the (input-augmented) system,
forced_linear_model.exact_row, and at an event that lies strictly inside the row the jump is applied - a data time equal to
the event time holds the state before the jump.  closed_outputs is the independent cross-check: the closed forms, segment by
segment.

The reference (chain_solve): the chain of solve_ivp calls a SciPy user would write - per segment t_eval = the row's data times in
(a, b] (the first: [t0, b]) with b appended when it is no data time, the jump applied to the last column, the next call started
from (b, y).  BDF is driven step by step as solve_ivp does it, for its step, LU and Jacobian counts.

The bound.  K[case] = 2 x the worst |y_chain - y_exact| / (atol + rtol |y_exact|) over the case's population: measured on the CPU
from the chained SciPy reference alone, before the first device run - the rule of forced_linear_model.K."""
import functools
import multiprocessing
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

import forced_linear_model as FL

N_T, N = 10, 320
RTOL, ATOL = 1e-3, 1e-6
TAU = 1.5                                  # row 0's event at a data time
_SIG = "const double *theta, const double *cond"

TIMES = np.array([[0.0, 0.7, TAU, np.nextafter(TAU, np.inf), 2.5, 4.1, 5.0, 6.5, 7.5, 8.5],
                  [0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0],
                  [0.0, 0.9, 2.0, 3.0, 4.5, 6.0, np.nan, np.nan, np.nan, np.nan]])
N_EV = 5
# event times; 3.2 and 3.6 lie between the data times 2.5 and 4.1, 20.0 is beyond row 0's end, 6.0 is row 2's end
EV_T = np.array([[TAU, 3.2, 3.6, 6.0, 20.0],
                 [np.nan] * 5,
                 [1.2, 2.0, 6.0, np.nan, np.nan]])
# (amount, kind): kind matters to E2 / E3 only (1 = reset of the central compartment); junk past a row's events, ignored
EV_V = np.array([[[0.8, 0], [0.5, 0], [9.0, 1], [0.6, 0], [0.4, 0]],
                 [[7.0, 3]] * 5,
                 [[0.7, 0], [9.0, 1], [0.3, 0], [7.0, 3], [7.0, 3]]], dtype=np.float64)

_CHAIN = f"""
__device__ void smc_user_y0({_SIG}, double *y) {{ y[0] = cond[0]; y[1] = 0.0; }}
__device__ void smc_user_rhs(double t, const double *y, {_SIG}, double *dydt) {{
    dydt[0] = -theta[0] * y[0];
    dydt[1] = theta[0] * y[0] - theta[1] * y[1];
}}
__device__ void smc_user_obs_vec(double t, const double *y, {_SIG}, double *out) {{ out[0] = y[0]; out[1] = y[1]; }}
"""
_CHAIN_EVENT = f"""__device__ void smc_user_event(int j, double t, double *y, {_SIG}) {{
    if (smc_event_value(cond, j, 1) == 0.0)
        y[0] += theta[2] * smc_event_value(cond, j, 0);
    else
        y[1] = 0.0;
}}
"""
_BOLUS_EVENT = f"__device__ void smc_user_event(int j, double t, double *y, {_SIG}) {{ y[0] += smc_event_value(cond, j, 0); }}\n"
_E1 = f"""
__device__ void smc_user_y0({_SIG}, double *y) {{ y[0] = cond[0]; }}
__device__ void smc_user_rhs(double t, const double *y, {_SIG}, double *dydt) {{ dydt[0] = -theta[0] * y[0]; }}
__device__ double smc_user_obs(double t, const double *y, {_SIG}) {{ return y[0]; }}
"""
# the hint: explicit RK45 sits on its stability limit for about T (ka + ke) / 3.3 attempts, T = 8.5
_E2 = _CHAIN + "__device__ double smc_user_cost(const double *theta) { return 2.6 * (theta[0] + theta[1]); }\n"
_E3 = _CHAIN + f"""__device__ void smc_user_jac(double t, const double *y, {_SIG}, double *J) {{
    J[0] = -theta[0]; J[1] = 0.0;
    J[2] = theta[0];  J[3] = -theta[1];
}}
"""
# "plain": the same model without smc_user_event, for a model without events; "source" = plain + the event
PLAIN = {"E1": _E1, "E2": _E2, "E3": _E3, "E4": FL.F1_SOURCE}
E1_SOURCE, E2_SOURCE, E3_SOURCE, E4_SOURCE = _E1 + _BOLUS_EVENT, _E2 + _CHAIN_EVENT, _E3 + _CHAIN_EVENT, FL.F1_SOURCE + _BOLUS_EVENT

CASES = {
    "E1": {"method": "RK45", "ns": 1, "n_obs": 1, "dim": 2, "n_val": 1, "n_in": 0, "source": E1_SOURCE},
    "E2": {"method": "RK45", "ns": 2, "n_obs": 2, "dim": 4, "n_val": 2, "n_in": 0, "source": E2_SOURCE},
    "E3": {"method": "BDF", "ns": 2, "n_obs": 2, "dim": 4, "n_val": 2, "n_in": 0, "source": E3_SOURCE},
    "E4": {"method": "RK45", "ns": 1, "n_obs": 1, "dim": 3, "n_val": 1, "n_in": 1, "source": E4_SOURCE},
}
for _c in CASES.values():
    _c.update(n=N, n_ex=3, n_cond=1, n_ev=N_EV, tol=(RTOL, ATOL))
THETA_TRUE = {"E1": (0.6, 0.05), "E2": (1.1, 0.45, 0.8, 0.05), "E3": (1.1, 2.0e4, 0.8, 0.05), "E4": (0.8, 1.2, 0.05)}
COND = np.array([[1.0], [1.4], [0.6]])

# `python tests/dosed_model.py` (SciPy 1.15.3): K = 2 x the worst ratio, fixed before the first device run
K = {"E1": 6.168, "E2": 5.898, "E3": 12.101, "E4": 77.408}


def events(cid, ev_t=EV_T, ev_v=EV_V):
    """The events= argument of HipEngine.set_model_user for the case: its n_val leading values."""
    return {"t": np.array(ev_t, dtype=np.float64), "values": np.ascontiguousarray(np.asarray(ev_v, dtype=np.float64)[:, :, :CASES[cid]["n_val"]])}


def events_inside():
    """EV_T / EV_V without the events at or beyond a row's end (row 0's 20.0, row 2's 6.0): the same solves."""
    ev_t, ev_v = EV_T.copy(), EV_V.copy()
    ev_t[0, 4] = np.nan
    ev_t[2, 2] = np.nan
    return ev_t, ev_v


def inputs(cid):
    return FL.make_inputs("F1") if CASES[cid]["n_in"] else None


def matrices(cid, th):
    """(A (ns, ns), B (ns, 1)) of y' = A y + B u: u is E4's input, absent (B = 0) elsewhere."""
    if cid == "E1":
        return np.array([[-th[0]]]), np.zeros((1, 1))
    if cid == "E4":
        return np.array([[-th[0]]]), np.array([[th[1]]])
    return np.array([[-th[0], 0.0], [th[0], -th[1]]]), np.zeros((2, 1))


def y_start(cid, cond_e):
    return np.array([cond_e[0]] + [0.0] * (CASES[cid]["ns"] - 1))


def apply_event(cid, th, v, y):
    """smc_user_event of the case on a copy of y; v: the event's values (amount, kind)."""
    y = np.array(y, dtype=np.float64)
    if cid in ("E1", "E4"):
        y[0] += v[0]
    elif v[1] == 0.0:
        y[0] += th[2] * v[0]
    else:
        y[1] = 0.0
    return y


def _knots(cid, e, inp):
    """(tk (m,), u (m, 1)) of experiment e: E4's input row, else a single knot of value 0."""
    if inp is None:
        return np.array([0.0]), np.zeros((1, 1))
    return FL._row(inp, e)


def segments(t_row, ev_row):
    """The segments of a row: [(a, b, data times in (a, b] - the first: [t0, b] -, index of the event at b or None)]."""
    tt = t_row[~np.isnan(t_row)]
    t_end = tt[-1]
    fire = [j for j in range(ev_row.size) if not np.isnan(ev_row[j]) and tt[0] < ev_row[j] < t_end]
    out, a = [], tt[0]
    for s, b in enumerate([ev_row[j] for j in fire] + [t_end]):
        inside = tt[((tt > a) | ((s == 0) & (tt == a))) & (tt <= b)]
        out.append((a, b, inside, fire[s] if s < len(fire) else None))
        a = b
    return out


# ---- data ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def population(cid):
    rs = np.random.RandomState(2000 + list(CASES).index(cid))
    span = {"E1": [(0.2, 1.5), (0.02, 0.1)],
            "E2": [(0.5, 2.0), (0.2, 1.5), (0.5, 1.0), (0.02, 0.1)],
            "E3": [(0.5, 2.0), (1.0e4, 3.0e4), (0.5, 1.0), (0.02, 0.1)],
            "E4": [(0.3, 1.5), (0.5, 2.0), (0.02, 0.1)]}[cid]
    th = np.column_stack([rs.uniform(lo, hi, N) for lo, hi in span])
    if cid == "E2":      # hint 2.6 (ka + ke): 24 particles above 220 (the list), 4 of them above 3700 (solo), spread over the blocks
        where = rs.permutation(N)[:24]
        th[where[:20], 1] = rs.uniform(90.0, 400.0, 20)
        th[where[20:], 1] = rs.uniform(1500.0, 2000.0, 4)
    return th


def cost_hint(th):
    return 2.6 * (th[:, 0] + th[:, 1])


def priors(cid):
    high = {"E1": (3.0, 1.0), "E2": (4.0, 4000.0, 2.0, 1.0), "E3": (4.0, 6.0e4, 2.0, 1.0), "E4": (3.0, 4.0, 1.0)}[cid]
    return {f"p{j}": {"dist": "uniform", "low": 0, "high": h} for j, h in enumerate(high)}


@functools.lru_cache(maxsize=None)
def make_data(cid):
    """(t, obs (n_ex, n_t, n_obs), cond): the exact outputs at THETA_TRUE plus Gaussian noise of its sigma."""
    rs = np.random.RandomState(400 + list(CASES).index(cid))
    f = exact_outputs(cid, np.array([THETA_TRUE[cid]]), TIMES, COND, EV_T, EV_V, inputs(cid))[0]
    return TIMES.copy(), f + THETA_TRUE[cid][-1] * rs.standard_normal(f.shape), COND.copy()


def model_kwargs(cid, ev=None):
    """The keyword arguments of HipEngine.set_model_user after (source, n_states, t, obs)."""
    c = CASES[cid]
    kw = {"cond": COND, "rtol": RTOL, "atol": ATOL, "method": c["method"], "events": events(cid) if ev is None else ev}
    if c["n_in"]:
        kw["inputs"] = inputs(cid)
    return kw


# ---- exact solutions ---------------------------------------------------------------------------------------------------

def exact_outputs(cid, th, t, cond, ev_t, ev_v, inp=None):
    """(n, n_ex, n_t, ns) exact states for parameters th (n, dim) on a design with its events, NaN past a row's end."""
    c = CASES[cid]
    y = np.full((th.shape[0], t.shape[0], t.shape[1], c["ns"]), np.nan)
    for e in range(t.shape[0]):
        tk, u = _knots(cid, e, inp)
        segs = segments(t[e], ev_t[e])
        for p in range(th.shape[0]):
            A, B = matrices(cid, th[p])
            now, i = y_start(cid, cond[e]), 0
            for a, b, inside, j in segs:
                stops = np.concatenate([[a], inside[inside > a], [b] if (inside.size == 0 or inside[-1] != b) else []])
                ys = FL.exact_row(A, B, now, tk, u, stops)
                first = 0 if (inside.size and inside[0] == a) else 1
                y[p, e, i:i + inside.size] = ys[first:first + inside.size]
                i += inside.size
                now = ys[-1] if j is None else apply_event(cid, th[p], ev_v[e, j], ys[-1])
    return y


def closed_outputs(cid, th, t, cond, ev_t, ev_v, inp=None):
    """The same from the closed forms, one time at a time: E1 a sum of exponentials (every fired dose decays from its own time),
    E2 / E3 Bateman's form from the last event, E4 forced_linear_model.f1_closed_row from the last event."""
    c = CASES[cid]
    y = np.full((th.shape[0], t.shape[0], t.shape[1], c["ns"]), np.nan)
    for e in range(t.shape[0]):
        tt = t[e][~np.isnan(t[e])]
        fire = [j for j in range(ev_t.shape[1]) if not np.isnan(ev_t[e, j]) and tt[0] < ev_t[e, j] < tt[-1]]
        tk, u = _knots(cid, e, inp)
        for p in range(th.shape[0]):
            q = th[p]
            if cid == "E1":
                for i, x in enumerate(tt):
                    y[p, e, i, 0] = cond[e, 0] * np.exp(-q[0] * (x - tt[0])) + sum(ev_v[e, j, 0] * np.exp(-q[0] * (x - ev_t[e, j]))
                                                                                  for j in fire if ev_t[e, j] < x)
                continue
            state, at, nxt = y_start(cid, cond[e]), tt[0], 0      # the state just after the last event (or the start), its time
            for i, x in enumerate(tt):
                while nxt < len(fire) and ev_t[e, fire[nxt]] < x:
                    j = fire[nxt]
                    state = apply_event(cid, q, ev_v[e, j], _flow(cid, q, state, at, ev_t[e, j], tk, u))
                    at, nxt = ev_t[e, j], nxt + 1
                y[p, e, i] = _flow(cid, q, state, at, x, tk, u)
    return y


def _flow(cid, q, y, a, b, tk, u):
    """The state at b of the solution through (a, y), no event in between."""
    if b == a:
        return np.array(y, dtype=np.float64)
    if cid == "E4":
        return np.array([FL.f1_closed_row(q, y[0], tk, u, np.array([a, b]))[1]])
    ka, ke, d = q[0], q[1], b - a
    g = y[0] * np.exp(-ka * d)
    return np.array([g, y[1] * np.exp(-ke * d) + y[0] * ka / (ke - ka) * (np.exp(-ka * d) - np.exp(-ke * d))])


# ---- the chained SciPy reference ------------------------------------------------------------------------------------------

def chain_solve(cid, th, cond_e, t_row, ev_row, ev_val, tk, u):
    """The chain of solve_ivp calls: states at the row's finite times (len, ns) and, for BDF, (steps, LU, Jacobians) summed over
    the segments."""
    from scipy.integrate import BDF, solve_ivp
    c = CASES[cid]
    A, B = matrices(cid, th)
    forced = bool(np.any(B != 0.0))
    f = (lambda t, y: A @ y + B[:, 0] * np.interp(t, tk, u[:, 0])) if forced else (lambda t, y: A @ y)
    y, out, counts = y_start(cid, cond_e), [], np.zeros(3, dtype=np.int64)
    for a, b, inside, j in segments(t_row, ev_row):
        if b == a:                                           # a row of one time: nothing to integrate
            out.append(np.repeat(y[None, :], inside.size, axis=0))
            continue
        own = inside.size > 0 and inside[-1] == b
        t_eval = inside if own else np.concatenate([inside, [b]])
        if c["method"] == "RK45":
            sol = solve_ivp(f, (a, b), y, method="RK45", t_eval=t_eval, rtol=RTOL, atol=ATOL)
            assert sol.status == 0
            ys = np.asarray(sol.y).T.reshape(-1, c["ns"])    # solve_ivp returns a list, not an array, when t_eval is empty
        else:
            s = BDF(f, a, y, b, rtol=RTOL, atol=ATOL, jac=lambda t, y: A)
            got, i = [], 0
            while s.status == "running":
                s.step()
                assert s.status != "failed"
                counts[0] += 1
                k = np.searchsorted(t_eval, s.t, side="right")
                if k > i:
                    got.append(s.dense_output()(t_eval[i:k]).T)
                    i = k
            counts[1:] += (s.nlu, s.njev)
            ys = np.concatenate(got)
        out.append(ys[:inside.size])
        y = ys[-1] if j is None else apply_event(cid, th, ev_val[j], ys[-1])
    return np.concatenate(out), counts


def _chain_particle(args):
    cid, p = args
    c = CASES[cid]
    th = population(cid)[p]
    y = np.full((c["n_ex"], N_T, c["ns"]), np.nan)
    counts = np.zeros((c["n_ex"], 3), dtype=np.int64)
    for e in range(c["n_ex"]):
        ok = ~np.isnan(TIMES[e])
        tk, u = _knots(cid, e, inputs(cid))
        y[e, ok], counts[e] = chain_solve(cid, th, COND[e], TIMES[e], EV_T[e], EV_V[e], tk, u)
    return y, counts


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Computed once per process: {"exact": (n, n_ex, n_t, ns), "scipy": the same from the chain, "counts": (n, n_ex, 3) steps / LU /
    Jacobians, "ratio": worst |scipy - exact| / (atol + rtol |exact|)}."""
    exact = exact_outputs(cid, population(cid), TIMES, COND, EV_T, EV_V, inputs(cid))
    jobs = [(cid, p) for p in range(N)]
    if FL._workers() > 1:
        with ProcessPoolExecutor(max_workers=FL._workers(), mp_context=multiprocessing.get_context("spawn")) as ex:
            rows = list(ex.map(_chain_particle, jobs, chunksize=8))
    else:
        rows = [_chain_particle(j) for j in jobs]
    y = np.array([r[0] for r in rows])
    counts = np.array([r[1] for r in rows])
    assert np.array_equal(np.isnan(y), np.isnan(exact))
    return {"exact": exact, "scipy": y, "counts": counts, "ratio": float(np.nanmax(np.abs(y - exact) / (ATOL + RTOL * np.abs(exact))))}


# ---- a regimen that was never run (predict_user_at with design events) ------------------------------------------------------

def design():
    """(t2, cond2, ev_t2, ev_v2): two experiments on a longer horizon under another regimen, narrower than the data's N_EV; row 1 is
    ragged, has a data time on an event and one event between its last two times."""
    t2 = np.array([[0.0, 1.0, 2.0, 4.0, 6.0, 9.0, 12.0], [0.5, 2.0, 3.0, 7.0, 11.0, np.nan, np.nan]])
    cond2 = np.array([[0.9], [1.2]])
    ev_t2 = np.array([[3.0, 5.0, 8.0], [3.0, 9.5, np.nan]])
    ev_v2 = np.array([[[0.6, 0], [9.0, 1], [0.9, 0]], [[1.1, 0], [0.2, 0], [7.0, 3]]], dtype=np.float64)
    return t2, cond2, ev_t2, ev_v2


def main():
    import scipy
    ids = sys.argv[1:] or list(CASES)
    print(f"SciPy {scipy.__version__}")
    print(f"{'case':4s} {'worst ratio':>12s} {'K':>9s}   steps / LU / Jacobians")
    for cid in ids:
        r = reference(cid)
        print(f"{cid:4s} {r['ratio']:12.4f} {2 * r['ratio']:9.3f}   {tuple(int(v) for v in r['counts'].sum(axis=(0, 1)))}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
