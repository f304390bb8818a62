"""The summary kernels (csrc/predictive_kernels.hip: pred_keys_kernel, pred_select_kernel) on planted values: a user model whose
outputs are its parameters (tests/planted_values.py) hands the kernels exactly the doubles a test uploaded, so the reference of
every summary is NumPy on the uploaded array alone.  CPU part: the populations hold what their table claims, the host core
(csrc/predictive_select.h) agrees with np.sort on these very columns, the linear rule is NumPy's, and the noise draw is restated
in NumPy (tests/philox_reference.py).  GPU part: counts, order statistics bit for bit, moments, at particle counts around every
boundary of the two kernels and with 1, 2 and 16 probabilities; then the noise term against its restatement - the counter
(seed, global particle, global cell), sigma fixed / estimated / from a noise model, staging groups, global_offset past 2**32."""
import ctypes

import numpy as np
import pytest

import philox_reference as PR
import planted_values as PV
from test_user_predictive import EPS, _bytes_of_one_experiment, _check_summary, _same_bits
from test_user_predictive import ps  # noqa: F401  (the fixture that compiles tests/hostcheck/predictive_select_hostcheck.cpp)

# one block iteration of pred_select_kernel takes 512 threads x 2 pairs = 2048 keys; a transpose tile is 32 particles wide
SIZES = (1, 2, 3, 63, 65, 511, 513, 2047, 2048, 2049, 4097, 70001)
PROB_SETS = {
    "median": (0.5,),
    "ends": (0.0, 1.0),
    # 32 ranks: the whole histogram; 0.5 twice; (m - 1) q an integer for many m; the largest double below 1
    "sixteen": (0.0, 1.0, 1 / 3, 0.25, 0.5, 0.5, 0.975, 1 - 2.0 ** -53, 0.025, 0.05, 0.1, 0.75, 0.9, 0.95, 2 / 3, 0.01),
}
SEEDS = (("SMC_SET_PRED", 10), ("SMC_SET_FILT", 11))        # descending and ascending column 5
FIELDS = ("mean", "sd", "lower", "upper", "quantile", "n_finite")
SIGMA = 0.05
OBS_SCALE = (1.0, 3.0, 0.5, 2.0, 1.5, 1.0, 0.25, 4.0)
_P, _F = (lambda j: ("param", j)), (lambda v: ("fixed", v))
NOISE = {"additive": [_P(7), _F(0.05), _P(7), _F(0.2), _P(7), _F(0.1), _P(7), _F(0.07)],
         "proportional": [_F(0.1), _P(7), _F(0.0), _F(0.3), _P(7), _F(0.0), _F(0.01), _F(0.5)]}
NOISE_SEEDS = (20240229, 0x1234567890ABCDEF)
NOISE_OFFSETS = (0, 12345, 2 ** 32 + 7)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _expected_counts(t, m):
    return (m[:, None, None] * ~np.isnan(t)[:, :, None] * np.ones(PV.N_OBS, dtype=np.int64)).astype(np.int64)


# ---- CPU -----------------------------------------------------------------------------------------------------------

def test_the_populations_hold_what_their_table_claims():
    for n in SIZES:
        for _, seed in SEEDS:
            th = PV.population(n, seed)
            b = _bits(th.T.copy())
            assert np.all(np.isfinite(th)) and th.shape == (n, 8)
            assert np.unique(th[:, 1]).size == 1 and th[0, 1] != 0.0
            # column 2: two adjacent doubles, 1 : 3, that share their top seven bytes
            x = np.array([PV.X2_BITS], dtype=np.uint64).view(np.float64)[0]
            assert set(b[2]) <= {PV.X2_BITS, PV.X2_BITS + 1} and int(np.sum(b[2] == PV.X2_BITS)) == (n + 3) // 4
            assert np.unique(b[2] >> np.uint64(8)).size == 1 and np.nextafter(x, np.inf) == (np.uint64(PV.X2_BITS + 1)).view(np.float64)
            # column 3: one top-six-byte prefix, up to 16 top-seven-byte prefixes, repeats
            j = b[3] - np.uint64(PV.X3_BITS)
            assert np.all(j < 4096) and np.unique(b[3] >> np.uint64(16)).size == 1
            assert np.unique(b[3] >> np.uint64(8)).size == np.unique(j >> np.uint64(8)).size <= 16
            if n >= 511:
                assert np.unique(b[3] >> np.uint64(8)).size == 16 and np.unique(j).size < n
            # column 4: fifteen values at most, zero always +0
            assert np.all(th[:, 4] == np.round(th[:, 4])) and np.all(np.abs(th[:, 4]) <= 7) and not np.any(np.signbit(th[th[:, 4] == 0, 4]))
            assert np.array_equal(th[:, 5], np.sort(th[:, 0])[::-1] if seed % 2 else np.sort(th[:, 0]))
            v7 = _bits(PV.outputs(th)[:, 7])
            assert set(v7) <= set(_bits(PV.SPECIALS)) and np.array_equal(PV.outputs(th)[:, :7], th[:, :7])
            if n >= 63:
                assert np.any(th[:, 0] < 0) and np.any(th[:, 0] > 0) and np.any(th[:, 4] < 0) and np.unique(th[:, 4]).size > 8
                assert set(v7) == set(_bits(PV.SPECIALS)) and np.unique(v7).size == 8          # +0, -0 and every denormal, both signs
                assert np.abs(th[:, 6]).max() / np.abs(th[:, 6]).min() > 1e200
            # column 6: NumPy's own two-pass mean and sd are finite at these magnitudes
            assert np.isfinite(np.mean(th[:, 6])) and np.isfinite(np.std(th[:, 6])) and np.abs(th[:, 6]).max() < 1e151
            assert np.array_equal(np.sort(th[:, 7]), (np.arange(n) + 0.5) / n)
            for cells in PV.DESIGNS:
                t, cond, m = PV.design(cells, n)
                pred = PV.planted(th, t, cond)
                assert pred.shape == (n,) + t.shape + (8,) and pred[0].size == cells
                assert np.array_equal(np.sum(np.isfinite(pred), axis=0), _expected_counts(t, m))       # exactly j per gated experiment
                assert np.array_equal(np.sum(~np.isnan(pred), axis=0), _expected_counts(t, m))
    want = {70001, 35001, 3, 2, 1, 0}
    assert want <= set(PV.design(264, 70001)[2]) and want - {3} <= set(PV.design(120, 70001)[2])
    assert np.isnan(PV.design(264, 5)[0]).sum() == 2 and np.isnan(PV.design(32, 5)[0]).sum() == 1
    th6 = PV.population(65, 10, gate=6)             # the last parameter a noise level, the gate before it, output 6 = -theta[5]
    assert th6.shape == (65, 8) and np.all(th6[:, 7] > 0.05) and np.array_equal(th6[:, :6], PV.population(65, 10)[:, :6])
    assert np.array_equal(np.sort(th6[:, 6]), (np.arange(65) + 0.5) / 65) and np.array_equal(PV.outputs(th6, 6)[:, 6], -th6[:, 5])
    assert np.array_equal(np.sum(np.isfinite(PV.planted(th6, *PV.design(264, 65)[:2], gate=6)), axis=0), _expected_counts(*PV.design(264, 65)[::2]))


def test_the_host_core_agrees_with_np_sort_on_the_planted_columns(ps):
    dp, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)
    lo, hi, fr = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
    for n in SIZES:
        th = PV.population(n, 10)
        counts = sorted({n, (n + 1) // 2, min(3, n), min(2, n), 1})
        for m in counts:
            is_open = th[:, 7] < m / n
            vals = PV.outputs(th)
            ranks = []
            for probs in PROB_SETS.values():
                for q in probs:
                    ps.ps_ranks(m, q, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(fr))
                    assert (lo.value, hi.value) == (int(np.floor((m - 1) * q)), int(np.ceil((m - 1) * q)))
                    ranks += [lo.value, hi.value]
            ranks = np.array(ranks, dtype=np.int64)
            qs = np.array([q for probs in PROB_SETS.values() for q in probs])
            for k in range(8):
                col = np.ascontiguousarray(np.where(is_open, vals[:, k], np.nan))
                out = np.empty(ranks.size)
                assert ps.ps_select(col.ctypes.data_as(dp), n, ranks.ctypes.data_as(lp), ranks.size, out.ctypes.data_as(dp)) == m
                srt = np.sort(col[is_open])
                if k == 7:      # NumPy's order between -0 and +0 is unspecified: by value, and the sign by the key order
                    assert np.array_equal(out, srt[ranks])
                    assert np.array_equal(np.signbit(out), ranks < np.sum(np.signbit(col[is_open])))
                else:
                    assert np.array_equal(_bits(out), _bits(srt[ranks])), (n, m, k)
                    assert np.array_equal(_bits(out[0::2]), _bits(np.nanquantile(col, qs, method="lower")))
                    assert np.array_equal(_bits(out[1::2]), _bits(np.nanquantile(col, qs, method="higher")))


def test_the_linear_rule_is_numpys_where_the_result_is_small_next_to_its_neighbours(pkg):
    lq = pkg.user_models.linear_quantile
    one = lq(-3.0, 0.0, 1 - 2.0 ** -53)                          # the value one formula from `lower` misses by a third
    assert one == np.quantile([-3.0, 0.0], 1 - 2.0 ** -53) and abs(one / (-3.0 * 2.0 ** -53) - 1) <= 4 * EPS
    assert np.isnan(lq(np.nan, np.nan, 0.0)) and lq(2.0, 2.0, 0.7) == 2.0 and lq(-1.0, 1.0, 0.5) == 0.0
    worst = 0.0
    for n in (2, 3, 63, 65, 2049):
        th = PV.population(n, 11)[:, :7]
        for q in PROB_SETS["sixteen"]:
            ref = np.quantile(th, q, axis=0, method="linear")
            lo, hi, frac = pkg.user_models.quantile_ranks(n, q)
            srt = np.sort(th, axis=0)
            got = lq(srt[lo], srt[hi], frac)
            assert np.all((srt[lo] <= got) & (got <= srt[hi]))
            worst = max(worst, np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))
    print(f"linear rule against np.quantile: worst relative difference {worst:.3g} (bound {4 * EPS:.3g})")
    assert worst <= 4 * EPS


def test_the_noise_draw_restated_in_numpy_is_philox_as_philox_h_states_it():
    for c, k, r in PR.KNOWN_ANSWERS:                                  # Random123's vectors, on ints and on arrays
        assert PR.philox(c, k) == r
        assert [int(w) for w in PR.philox_np(c, k)] == r
    assert PR.KNOWN_ANSWERS[0][2] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    rs = np.random.RandomState(0)
    seed = 0x1234567890ABCDEF
    gidx = np.array([0, 1, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 5_000_000_000, 2 ** 63 + 11], dtype=np.uint64)
    stream = np.uint64(PR.PRED_NOISE_STREAM) | rs.randint(0, 2 ** 31, gidx.size).astype(np.uint64)
    for block in (0, 3, 255):
        arr = PR.philox_block_np(seed, gidx, stream, block)
        for i in range(gidx.size):
            g, s = int(gidx[i]), int(stream[i])
            # the counter layout of philox_block: (gidx lo, gidx hi, stream lo, stream hi[23:0] << 8 | block)
            assert PR.block_counter(g, s, block) == [g & 0xFFFFFFFF, g >> 32, s & 0xFFFFFFFF, (0x505245 << 8) | block]
            one = PR.philox_block(seed, g, s, block)
            assert one == PR.philox(PR.block_counter(g, s, block), [seed & 0xFFFFFFFF, seed >> 32])
            assert [int(w[i]) for w in arr] == one
            assert PR.u01_from(one[0], one[1]) == float(PR.u01_from(arr[0], arr[1])[i])
    assert PR.u01_from(0xFFFFFFFF, 0xFFFFFFFF) == 1 - 2.0 ** -53 and PR.u01_from(0, 0) == 0.0 and PR.u01_from(1 << 31, 0) == 0.5
    # the draw of (particle, cell): rows move with global_offset, columns are the cells they were asked for
    cells = np.array([0, 1, 263, 2 ** 20])
    z = PR.pred_noise_z(seed, 2 ** 32 + 7, 5, cells)
    assert z.shape == (5, 4) and np.all(np.isfinite(z)) and np.unique(z).size == 20
    assert np.array_equal(PR.pred_noise_z(seed, 2 ** 32 + 8, 4, cells), z[1:])
    assert np.array_equal(PR.pred_noise_z(seed, 2 ** 32 + 7, 5, cells[2:3]), z[:, 2:3])
    x, y, zz, w = PR.philox_block(seed, 2 ** 32 + 9, PR.PRED_NOISE_STREAM | 263, 0)
    assert z[2, 2] == np.sqrt(-2.0 * np.log(1.0 - PR.u01_from(x, y))) * np.cos(6.283185307179586 * PR.u01_from(zz, w))
    big = PR.pred_noise_z(7, 0, 4096, np.arange(64))
    assert np.abs(big).max() <= 8.6 and abs(big.mean()) < 5 / 512 and abs(big.std() - 1) < 5 / 512 / np.sqrt(2)


# ---- GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted_engines(pkg):
    """One engine per (particle count, gate column, method, noise model) - an engine holds exactly its n particles - compiled once, both
    sets uploaded from different seeds; the data's own design is the 120-cell one."""
    made = {}

    def get(n, gate=7, method="RK45", noise=None):
        key = (n, gate, method, noise is not None)
        if key in made:
            return made[key]
        eng = pkg.HipEngine(n, 8, device=0)                  # SMC_MAX_DIM parameters: seven (six) values, the gate (, a noise level)
        made[key] = E = {"eng": eng, "n": n, "gate": gate, "sets": [(getattr(pkg, w), PV.population(n, s, gate)) for w, s in SEEDS]}
        t, cond, _ = PV.design(120, n)
        try:
            eng.set_prior({f"p{i}": {"dist": "flat", "mu": 0.0, "sigma": 1.0} for i in range(8)})
            eng.set_model_user(PV.source(gate=gate, jac=method == "BDF"), 1, t, np.full(t.shape + (8,), np.nan), cond=cond,
                               est_sigma=gate == 6, sigma_fixed=SIGMA, obs_scale=OBS_SCALE, method=method, noise=noise)
            for which, th in E["sets"]:
                eng.upload_particles(which, th)
        except pkg.SmcError as e:          # a device error: nothing more is started on a GPU that may have faulted
            pytest.exit(f"planted engine {key}: {e}", returncode=3)
        return E

    yield get
    for E in made.values():
        E["eng"].close()


def _design_kw(cells, n):
    t, cond, m = PV.design(cells, n)
    return t, cond, m, ({} if cells == 120 else {"t": t, "cond": cond})


def _assert_predicts_the_planted_bits(E):
    """Before the model is relied on: predict_user_at returns the uploaded bits, and NaN exactly where the gate and the rows say."""
    for _, th in E["sets"]:
        for cells in PV.DESIGNS:
            t, cond, m, kw = _design_kw(cells, E["n"])
            pred, info = E["eng"].predict_user_at(th, **kw)
            want = PV.planted(th, t, cond, E["gate"])
            assert info["n_failed"] == 0 and pred.shape == want.shape
            assert np.array_equal(np.isnan(pred), np.isnan(want))
            assert np.array_equal(_bits(np.nan_to_num(pred, nan=1.0)), _bits(np.nan_to_num(want, nan=1.0)))      # -0 and denormals as they are


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_model_predicts_the_planted_bits(planted_engines, n):
    _assert_predicts_the_planted_bits(planted_engines(n))


def _check_column_7(pkg, out, pred, probs):
    """Signed zeros and denormals: NumPy's order between -0 and +0 is unspecified, so by value; the device's order is the key's
    (-0 just below +0): rank r carries the sign bit exactly when r < the number of negative entries, zeros included."""
    col = pred[..., 7]
    q = np.asarray(probs)
    fin = np.isfinite(col)
    m = fin.sum(axis=0)
    some = m > 0
    neg = np.sum(np.signbit(col) & fin, axis=0)
    lo, hi, _ = pkg.user_models.quantile_ranks(np.maximum(m, 1)[None], q[:, None, None])
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            lower = np.nanquantile(col, q, axis=0, method="lower")
            upper = np.nanquantile(col, q, axis=0, method="higher")
    for name, ref, rank in (("lower", lower, lo), ("upper", upper, hi)):
        got = out[name][..., 7]
        assert np.isnan(got[:, ~some]).all(), name
        assert np.array_equal(got[:, some], ref[:, some]), name
        assert np.array_equal(np.signbit(got)[:, some], (rank < neg[None])[:, some]), name
    big = 2.2250738585072014e-308
    assert np.isnan(out["mean"][..., 7][~some]).all() and np.isnan(out["sd"][..., 7][~some]).all()
    assert np.all(np.abs(out["mean"][..., 7][some]) <= big) and np.all((0 <= out["sd"][..., 7][some]) & (out["sd"][..., 7][some] <= big * (1 + 8 * EPS)))


def _check_small_cells(out, pred, probs, m_cells):
    """m = 0: NaN in every field; m = 1: sd == 0 and every order statistic is the one value; m = 2 at q = 0.5: the two values."""
    none = m_cells == 0
    for name in ("mean", "sd", "lower", "upper", "quantile"):
        assert np.isnan(out[name][..., none]).all(), name
    assert np.all(out["n_finite"][none] == 0)
    one = m_cells == 1
    if one.any():
        v = np.sort(pred[:, one], axis=0)[0]                                      # NaN last
        assert np.all(out["sd"][one] == 0.0) and np.array_equal(out["mean"][one], v)      # by value: 0.0 + -0.0 is +0.0
        for name in ("lower", "upper", "quantile"):
            assert np.all(_bits(out[name][:, one]) == _bits(v)[None, :]), name
    two = (m_cells == 2) & (np.arange(PV.N_OBS) != 7)                            # column 7: _check_column_7
    if two.any() and 0.5 in probs:
        j = list(probs).index(0.5)
        srt = np.sort(pred[:, two], axis=0)
        assert np.array_equal(_bits(out["lower"][j][two]), _bits(srt[0])) and np.array_equal(_bits(out["upper"][j][two]), _bits(srt[1]))


def _check_planted_summaries(pkg, E, probs, cells):
    n, eng = E["n"], E["eng"]
    t, cond, m, kw = _design_kw(cells, n)
    counts = _expected_counts(t, m)
    for which, th in E["sets"]:
        pred = PV.planted(th, t, cond, E["gate"])
        out = eng.predictive_summary(which, probs=probs, **kw)
        again = eng.predictive_summary(which, probs=probs, **kw)
        assert _same_bits(out, again)                                             # a second call: the same bits
        assert out["n_failed"] == 0 and out["n_finite"].shape == counts.shape
        assert np.array_equal(out["n_finite"], counts)                            # the planted count; 0 where the gate shuts everyone out
        reached = _check_summary(pkg, {k: out[k][..., :7] for k in FIELDS}, pred[..., :7], probs, n)
        assert reached == int(np.sum(counts[..., :7] > 0))
        _check_column_7(pkg, out, pred, probs)
        _check_small_cells(out, pred, probs, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("cells", PV.DESIGNS)
@pytest.mark.parametrize("pset", list(PROB_SETS))
@pytest.mark.parametrize("n", SIZES)
def test_summaries_are_numpy_on_the_planted_array(pkg, planted_engines, n, pset, cells):
    _check_planted_summaries(pkg, planted_engines(n), PROB_SETS[pset], cells)


def _noise_sd(pkg, kind, th, pred):
    """sd of the noise term per (particle, cell), as include/smc_hip.h states it for the three ways a model carries its noise."""
    s = np.asarray(OBS_SCALE)
    if kind == "fixed":
        return np.broadcast_to(SIGMA * s, pred.shape)
    if kind == "est_sigma":
        return np.broadcast_to(th[:, 7, None, None, None] * s, pred.shape)
    ai, af, pi, pf = pkg.user_models.noise_layout(NOISE, PV.N_OBS, th.shape[1])
    a = np.where(ai >= 0, th[:, np.maximum(ai, 0)], af[None, :])
    b = np.where(pi >= 0, th[:, np.maximum(pi, 0)], pf[None, :])
    return np.hypot((a * s)[:, None, None, :], b[:, None, None, :] * pred)


def _noise_bound(sd, pred):
    """Per cell, the largest difference a value v + sd z can show between the kernel and its restatement, hence (sorting is
    1-Lipschitz in the sup norm) every order statistic.  Both sides form the same u1, u2 and the same cosine argument; |z| <= 8.6
    for a 53-bit u1.  ln, sqrt, cos and their product: z is off by at most ~4 ulp of itself, 35 EPS absolute; the products
    sigma s_k (or the square root of the noise model's sum of squares, ~2 ulp) and sd z: 4.3 EPS sd each; the final sum, rounded
    once or contracted into an FMA: EPS / 2 (|v| + 8.6 sd).  Together under 53 EPS sd + EPS |v|: 64 EPS sd + 2 EPS |v|."""
    with np.errstate(invalid="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return np.nanmax(np.where(np.isnan(pred), np.nan, 64 * EPS * sd + 2 * EPS * np.abs(pred)), axis=0)


def _check_noisy(pkg, E, kind, which, th, cells, probs, seed, goff, label, **extra):
    """predictive_summary(noise=True) against NumPy's order statistics of planted + sd z(seed, goff + p, global cell)."""
    import warnings
    n, eng = E["n"], E["eng"]
    t, cond, m, kw = _design_kw(cells, n)
    pred = PV.planted(th, t, cond, E["gate"])
    sd = _noise_sd(pkg, kind, th, pred)
    z = PR.pred_noise_z(seed, goff, n, np.arange(pred[0].size)).reshape(pred.shape)
    noisy = pred + sd * z
    out = eng.predictive_summary(which, probs=probs, noise=True, seed=seed, global_offset=goff, **kw, **extra)
    assert out["n_failed"] == 0 and np.array_equal(out["n_finite"], _expected_counts(t, m))
    q = np.asarray(probs)
    some = out["n_finite"] > 0
    bound = _noise_bound(sd, pred)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ref = {"lower": np.nanquantile(noisy, q, axis=0, method="lower"), "upper": np.nanquantile(noisy, q, axis=0, method="higher")}
        sd_max, v_max = np.nanmax(np.where(np.isnan(pred), np.nan, sd), axis=0), np.nanmax(np.abs(pred), axis=0)
    worst, worst_sd = 0.0, 0.0
    small_v = some & (np.nan_to_num(v_max) <= np.nan_to_num(sd_max))               # there the EPS |v| term is beside the point
    for name in ("lower", "upper"):
        assert np.isnan(out[name][:, ~some]).all()
        d = np.abs(out[name] - ref[name])
        worst = max(worst, float(np.max(d[:, some] / bound[some])))
        if small_v.any():
            worst_sd = max(worst_sd, float(np.max(d[:, small_v] / (EPS * sd_max[small_v]))))
    print(f"noise {label}: worst |device - restated| = {worst:.3g} of the bound 64 EPS sd + 2 EPS |v|; "
          f"{worst_sd:.3g} EPS sd over the {int(small_v.sum())} cells with |v| <= sd")
    assert worst <= 1.0
    return out, worst_sd


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fixed", "est_sigma", "noise_model"])
@pytest.mark.parametrize("n", [65, 2049])
def test_the_noise_term_is_its_numpy_restatement(pkg, planted_engines, n, kind):
    E = planted_engines(n) if kind == "fixed" else planted_engines(n, gate=6, noise=NOISE if kind == "noise_model" else None)
    probs = PROB_SETS["sixteen"]
    which, th = E["sets"][1]
    if kind != "fixed":
        _assert_predicts_the_planted_bits(E)
    plain = E["eng"].predictive_summary(which, probs=probs)
    for seed in NOISE_SEEDS:
        for goff in NOISE_OFFSETS:
            _check_noisy(pkg, E, kind, which, th, 264, probs, seed, goff, f"{kind} n={n} seed={seed:#x} offset={goff}")
    w0, th0 = E["sets"][0]
    _check_noisy(pkg, E, kind, w0, th0, 120, probs, NOISE_SEEDS[0], NOISE_OFFSETS[2], f"{kind} n={n} data design, the other set")
    assert _same_bits(plain, E["eng"].predictive_summary(which, probs=probs))     # noise=False after noise=True: the noiseless bits


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2049])
def test_staging_groups_do_not_change_a_noisy_bit(pkg, planted_engines, n):
    E = planted_engines(n)
    probs = PROB_SETS["sixteen"]
    which, th = E["sets"][1]
    for cells in (264, 120):
        kw = _design_kw(cells, n)[3]
        seed, goff = NOISE_SEEDS[1], NOISE_OFFSETS[2]
        one, _ = _check_noisy(pkg, E, "fixed", which, th, cells, probs, seed, goff, f"ungrouped n={n} cells={cells}")
        need = _bytes_of_one_experiment(pkg, E["eng"], which=which, probs=probs, **kw)
        grouped, _ = _check_noisy(pkg, E, "fixed", which, th, cells, probs, seed, goff, f"one experiment per group n={n} cells={cells}",
                                  max_staging_bytes=need)
        assert _same_bits(one, grouped)
        with pytest.raises(pkg.SmcError, match=rf"needs {need} B"):
            E["eng"].predictive_summary(which, probs=probs, noise=True, seed=seed, max_staging_bytes=need - 1, **kw)


def _every_noisy_value(eng, which, n, seed, goff, t, cond):
    """With n - 1 a power of two, q = r / (n - 1) is exact and picks rank r: every noisy value of every cell, sorted, in n / 16 calls."""
    assert (n - 1) & (n - 2) == 0
    rows = []
    for r0 in range(0, n, 16):
        q = np.arange(r0, min(r0 + 16, n)) / (n - 1)
        out = eng.predictive_summary(which, probs=q, noise=True, seed=seed, global_offset=goff, t=t, cond=cond)
        assert np.array_equal(_bits(out["lower"]), _bits(out["upper"])) and np.all(out["n_finite"] == n)
        rows.append(out["lower"])
    return np.concatenate(rows).reshape(n, -1)


@pytest.mark.gpu
def test_every_particle_and_cell_has_a_draw_of_its_own(pkg, planted_engines):
    n = 65
    row = np.array([1.25] * 7 + [0.25])                                           # identical particles, the gate open everywhere
    E = planted_engines(n)
    which = E["sets"][1][0]
    t = np.tile([0.0, 1.0, 2.0], (2, 1))
    cond = np.ones((2, 1))
    cells = t.size * PV.N_OBS
    sd = np.tile(SIGMA * np.asarray(OBS_SCALE), t.size)                          # per cell
    seed, goff = NOISE_SEEDS[0], NOISE_OFFSETS[1]
    v = np.tile(PV.outputs(row[None])[0], t.size)                                # per cell: 1.25, output 7 the table's 5e-324
    tol = 64 * EPS * sd + 2 * EPS * v
    try:
        E["eng"].upload_particles(which, np.tile(row, (n, 1)))
        got = _every_noisy_value(E["eng"], which, n, seed, goff, t, cond)
        shifted = _every_noisy_value(E["eng"], which, n, seed, goff + 1, t, cond)
    finally:
        E["eng"].upload_particles(which, E["sets"][1][1])
    z = PR.pred_noise_z(seed, goff, n + 1, np.arange(cells))                     # particles goff .. goff + n
    assert np.all(np.abs(got - np.sort(v + sd * z[:n], axis=0)) <= tol)
    # distinct draws: no two cells hold the same multiset - neither two outputs of a time nor two times of an output
    zs = (got - v) / sd
    apart = np.abs(zs[:, :, None] - zs[:, None, :]).max(axis=0) + np.eye(cells)
    print(f"standardised sorted draws of two cells differ by at least {apart.min():.3g}")
    assert apart.min() > 1e-3
    # global_offset + 1: the same draws one particle on - the first leaves, particle goff + n joins
    assert np.all(np.abs(shifted - np.sort(v + sd * z[1:], axis=0)) <= tol)
    assert np.abs(shifted - got).max() > 1e-3 * sd.min()


@pytest.mark.gpu
def test_the_bdf_prediction_kernel_feeds_the_same_summary(pkg, planted_engines):
    E = planted_engines(65, method="BDF")
    _assert_predicts_the_planted_bits(E)
    for cells in (264, 120):
        _check_planted_summaries(pkg, E, PROB_SETS["sixteen"], cells)
    which, th = E["sets"][1]
    _check_noisy(pkg, E, "fixed", which, th, 264, PROB_SETS["sixteen"], NOISE_SEEDS[0], NOISE_OFFSETS[2], "fixed n=65 BDF")
