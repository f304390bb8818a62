"""CPU tests of the rejection threshold of a Michaelis-Menten proposal (csrc/smc_internal.h: mm_reject_threshold, through the
C ABI: smc_mm_reject_threshold).  The propose kernel writes it once per particle and sweep; an item of a later pass of the solve
queue adds up the sums of squared residuals its siblings have published and is cancelled before its first attempt when they reach it
(mm_kernels.hip: MMOps::start_values).  That is only sound if the accept kernel - whose expression is restated here in NumPy
float64, operation by operation, in its order - then rejects the proposal whatever the unfinished solves return."""
import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

N_DRAWS = 4000


def _T(pkg, lk1, gamma, rr, sigma, n_ex, n_t, pratio=1.0, in_support=1):
    return float(pkg.lib().smc_mm_reject_threshold(float(lk1), float(gamma), float(rr), float(sigma), int(n_ex), int(n_t), float(pratio),
                                                   int(in_support)))


def _look_sum(S, finished):
    """What the look adds up: the finished sums in experiment order, one rounded addition each, from 0.0."""
    fin = np.float64(0.0)
    for k in range(len(S)):
        if finished[k]:
            fin = fin + np.float64(S[k])
    return float(fin)


def _claimed(fin, T):
    """The look's comparison."""
    return fin >= T and fin <= np.finfo(np.float64).max


def _accept_pp(S, lk1, gamma, sigma, n_t, pratio, ratio_mode):
    """mm_finish_kernel's pp: lk2 = sum_k (c0 - S_k / (2 s2)) from 0.0 in experiment order, exp((lk2 - lk1) * gamma) [* pratio]."""
    sigma, lk1, gamma = np.float64(sigma), np.float64(lk1), np.float64(gamma)
    s2 = sigma * sigma
    c0 = (np.float64(-0.5) * np.float64(n_t)) * np.log(np.float64(2.0) * np.float64(3.141592653589793) * s2)
    lk2 = np.float64(0.0)
    for k in range(len(S)):
        lk2 = lk2 + (c0 - np.float64(S[k]) / (np.float64(2.0) * s2))
    px = lk2 - lk1
    with np.errstate(over="ignore", under="ignore"):
        pp = np.exp(px * gamma)
    if ratio_mode:
        pp = pp * np.float64(pratio)
    return float(pp)


def _draw(rs):
    """One proposal over the ranges a run sees: gamma from 1e-4 to 1, sigma around the data's noise and far from it, lk1 the
    likelihood of a current point that fits from well (posterior) to not at all (prior)."""
    n_ex, n_t = int(rs.randint(1, 9)), int(rs.randint(5, 41))
    sigma = float(np.exp(rs.uniform(np.log(5e-3), np.log(0.5))))
    sigma_cur = sigma * float(np.exp(rs.uniform(-0.5, 0.5)))
    gamma = float(np.exp(rs.uniform(np.log(1e-4), 0.0)))
    rr = float(rs.uniform(0.0, 1.0)) if rs.rand() < 0.9 else float(np.exp(rs.uniform(-700.0, 0.0)))
    rr = rr if rr > 0.0 else 0.5
    ratio_mode = bool(rs.rand() < 0.5)
    pratio = float(np.exp(rs.uniform(np.log(1e-3), np.log(1e3)))) if ratio_mode else 1.0
    # chi-square-like for a fitting point, up to 1e6 times that for a prior draw
    S_cur = n_ex * n_t * sigma_cur ** 2 * float(np.exp(rs.uniform(-1.0, np.log(1e6))))
    lk1 = n_ex * (-0.5 * n_t) * math.log(2.0 * math.pi * sigma_cur ** 2) - S_cur / (2.0 * sigma_cur ** 2)
    return dict(n_ex=n_ex, n_t=n_t, sigma=sigma, gamma=gamma, rr=rr, ratio_mode=ratio_mode, pratio=pratio, lk1=lk1)


@pytest.fixture(scope="module")
def draws(pkg):
    rs = np.random.RandomState(20240611)
    out = []
    for _ in range(N_DRAWS):
        d = _draw(rs)
        d["T"] = _T(pkg, d["lk1"], d["gamma"], d["rr"], d["sigma"], d["n_ex"], d["n_t"], d["pratio"])
        out.append(d)
    return out


def test_threshold_exists_unless_its_terms_cancel(draws):
    """In the notation of the function's comment: a finite, positive T where B >= 1e-3 scale; T = 0 where B is negative beyond the
    margin (the proposal is rejected with no residual at all: the draws let sigma jump by up to exp(0.5) from a current point that
    may fit perfectly, so a few per cent of them are); +inf, the doubtful case, only in the thin band between.  A factor of two
    either side of the limits is left to rounding."""
    n_finite = 0
    for d in draws:
        c0 = (-0.5 * d["n_t"]) * math.log(2.0 * math.pi * d["sigma"] ** 2)
        E = math.log(d["rr"]) - math.log(d["pratio"])
        B = d["n_ex"] * c0 - d["lk1"] - E / d["gamma"]
        scale = d["n_ex"] * abs(c0) + abs(d["lk1"]) + (1.0 + abs(E)) / d["gamma"]
        if B >= 2e-3 * scale:
            assert math.isfinite(d["T"]) and d["T"] > 0.0, d
        elif 1e-9 * scale <= B <= 0.5e-3 * scale:
            assert d["T"] == math.inf, d
        elif B <= -1e-9 * scale:
            assert d["T"] == 0.0, d
        n_finite += math.isfinite(d["T"])
    assert n_finite >= 0.99 * len(draws)


def test_random_finished_subsets(draws):
    """Whenever the finished sums reach T the accept expression gives pp < rr - with the unfinished sums at 0 and at random positive
    values."""
    rs = np.random.RandomState(7)
    n_claimed = 0
    for d in draws:
        T, n_ex = d["T"], d["n_ex"]
        if not math.isfinite(T):
            continue
        finished = rs.rand(n_ex) < 0.6
        if not finished.any():
            finished[rs.randint(n_ex)] = True
        w = rs.uniform(0.05, 1.0, n_ex) * finished
        # totals from well below the threshold to far above it, many of them within a few ulps of it
        f = rs.choice([0.3, 0.999999, 1.0, 1.0 + 4e-16, 1.000001, 1.5, 30.0])
        S = T * f * w / w.sum()
        if T == 0.0:                           # rejected with no residual at all: nothing finished, or anything
            S = w * rs.choice([0.0, 1e-300, 1e-3])
        fin = _look_sum(S, finished)
        if not _claimed(fin, T):
            continue
        n_claimed += 1
        for unfinished in (0.0, None):
            S_all = S.copy()
            rest = ~finished
            S_all[rest] = 0.0 if unfinished is not None else max(T, 1e-3) * np.exp(rs.uniform(-20.0, 5.0, rest.sum()))
            pp = _accept_pp(S_all, d["lk1"], d["gamma"], d["sigma"], d["n_t"], d["pratio"], d["ratio_mode"])
            assert pp < d["rr"], (d, S_all, pp)
    assert n_claimed > N_DRAWS // 3


def test_adversarial_placement(draws):
    """The finished sum exactly at T, one ulp above and one ulp below: at and above T the claim must be true, below T it is simply
    not made."""
    for d in draws:
        T, n_ex = d["T"], d["n_ex"]
        if not math.isfinite(T):
            continue
        for k in {0, n_ex - 1}:                # one finished experiment, the first or the last term of the accept kernel's sum
            for fin in (T, np.nextafter(T, np.inf), np.nextafter(T, 0.0)) if T > 0.0 else (0.0, 5e-324):
                S = np.zeros(n_ex)
                finished = np.zeros(n_ex, dtype=bool)
                S[k], finished[k] = fin, True
                assert _look_sum(S, finished) == fin
                if fin < T:
                    assert not _claimed(fin, T)
                    continue
                assert _claimed(fin, T)
                pp = _accept_pp(S, d["lk1"], d["gamma"], d["sigma"], d["n_t"], d["pratio"], d["ratio_mode"])
                assert pp < d["rr"], (d, k, fin, pp)
        # ... and spread evenly over all experiments (every term of the sum rounds)
        S = np.full(n_ex, T / n_ex)
        fin = _look_sum(S, np.ones(n_ex, dtype=bool))
        if _claimed(fin, T):
            assert _accept_pp(S, d["lk1"], d["gamma"], d["sigma"], d["n_t"], d["pratio"], d["ratio_mode"]) < d["rr"]


def test_tightness(draws):
    """T is no less than the real-number threshold 2 sigma^2 (n_ex c0 - lk1 - (ln rr - ln pratio) / gamma) and at most (1 + 1e-6)
    times it: the margin cannot silently grow.  (T = 0 stands for every threshold <= 0: sums of squares are not negative.)"""
    getcontext().prec = 60
    pi = Decimal("3.14159265358979323846264338327950288419716939937510582097494")
    n_checked = 0
    for d in draws:
        T = d["T"]
        if not math.isfinite(T):
            continue
        n_checked += 1
        s2 = Decimal(d["sigma"]) ** 2
        c0 = Decimal(-d["n_t"]) / 2 * (2 * pi * s2).ln()
        E = Decimal(d["rr"]).ln() - Decimal(d["pratio"]).ln()
        T_real = 2 * s2 * (d["n_ex"] * c0 - Decimal(d["lk1"]) - E / Decimal(d["gamma"]))
        if T == 0.0:
            assert T_real < 0, (d, float(T_real))
            continue
        assert T_real > 0
        assert Decimal(T) >= T_real, d
        assert Decimal(T) <= T_real * (1 + Decimal("1e-6")), (d, float(T_real))
    assert n_checked >= 0.99 * len(draws)


@pytest.mark.parametrize("change", [
    dict(rr=0.0), dict(rr=-0.25), dict(rr=1.5), dict(rr=math.nan),
    dict(sigma=0.0), dict(sigma=-0.02), dict(sigma=math.nan), dict(sigma=math.inf),
    dict(pratio=0.0), dict(pratio=-1.0), dict(pratio=math.inf), dict(pratio=math.nan),
    dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=math.nan), dict(gamma=math.inf),
    dict(lk1=math.nan), dict(lk1=-math.inf), dict(lk1=math.inf),
    dict(in_support=0), dict(n_ex=0), dict(n_t=0),
])
def test_doubtful_inputs_never_cancel(pkg, change):
    a = dict(lk1=-350.0, gamma=0.01, rr=0.4, sigma=0.02, n_ex=6, n_t=40, pratio=1.0, in_support=1)
    assert math.isfinite(_T(pkg, **a)) and _T(pkg, **a) > 0.0
    a.update(change)
    assert _T(pkg, **a) == math.inf


def test_cancelling_terms_never_cancel(pkg):
    """lk1 so high that the proposal is rejected with no residual at all: T = 0; the neighbourhood where the terms of a positive
    threshold cancel: no threshold."""
    n_ex, n_t, sigma = 6, 40, 0.02
    top = n_ex * (-0.5 * n_t) * math.log(2.0 * math.pi * sigma ** 2)
    for lk1 in (top + 50.0, top + 1e-3):
        assert _T(pkg, lk1, 1.0, 0.999999, sigma, n_ex, n_t) == 0.0
    for lk1 in (top, top - 1e-3, top - 0.5):
        assert _T(pkg, lk1, 1.0, 0.999999, sigma, n_ex, n_t) == math.inf
    assert 0.0 < _T(pkg, top - 5.0, 1.0, 0.999999, sigma, n_ex, n_t) < math.inf
