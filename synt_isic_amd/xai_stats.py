"""The classical two-sample statistics of ``statistical_validation_comprehensive`` (xai/XAI.py:1708-2005) in numpy and
``math`` -- the product does not depend on scipy (as with ``xai.select_regions``).  Every function gives what the scipy call
of the reference gives (tests/test_xai_stats_cpu.py: statistics to 1e-12, p-values to 1e-10 relative):

* ``descriptive``        -- :1744-1759, with the biased skewness and excess kurtosis ``scipy.stats.skew`` / ``kurtosis`` default to
* ``ttest_ind``          -- ``stats.ttest_ind`` (Student) and ``equal_var=False`` (Welch)
* ``mannwhitneyu``       -- ``stats.mannwhitneyu(alternative='two-sided')`` with the ``auto`` rule: the exact null distribution
                            when min(n1, n2) <= 8 and there are no ties, else the normal approximation (tie and continuity corrected)
* ``ranksums``           -- ``stats.ranksums``
* ``cohens_d`` / ``glass_delta`` -- :1815-1842
* ``levene``             -- ``stats.levene`` (median centring)
* ``f_test``             -- :1950-1952

p-values come from one regularised incomplete beta function (Lentz's continued fraction) and ``math.erfc``.  An upper tail is
the complementary beta function I_{1-x}(b, a), never ``1 - cdf``: both tails keep their relative accuracy.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np


# ---- regularised incomplete beta -------------------------------------------------------------------------------------------
def _betacf(a: float, b: float, x: float) -> float:
    """continued fraction of I_x(a, b) (modified Lentz; converges fast for x < (a + 1) / (a + b + 2))"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 500):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            break
    return h


def betainc_pair(a: float, b: float, x: float, y: float) -> Tuple[float, float]:
    """(I_x(a, b), I_y(b, a)) for x + y = 1: the regularised incomplete beta function and its complement.  The caller passes
    both x and y = 1 - x, each formed without cancellation; whichever of the two values is the small one comes straight from
    the continued fraction."""
    a, b, x, y = float(a), float(b), float(x), float(y)
    if math.isnan(x) or math.isnan(y) or math.isnan(a) or math.isnan(b):
        return math.nan, math.nan
    if x <= 0.0:
        return 0.0, 1.0
    if y <= 0.0:
        return 1.0, 0.0
    bt = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(y))
    if x < (a + 1.0) / (a + b + 2.0):
        v = bt * _betacf(a, b, x) / a
        return v, 1.0 - v
    v = bt * _betacf(b, a, y) / b
    return 1.0 - v, v


def t_two_sided_p(t: float, df: float) -> float:
    """2 * P(T_df >= |t|) = I_{df / (df + t^2)}(df / 2, 1 / 2)"""
    t, df = float(t), float(df)
    if math.isnan(t) or math.isnan(df):
        return math.nan
    if math.isinf(t):
        return 0.0
    t2 = t * t
    return betainc_pair(0.5 * df, 0.5, df / (df + t2), t2 / (df + t2))[0]


def f_cdf_sf(f: float, d1: float, d2: float) -> Tuple[float, float]:
    """(P(F <= f), P(F > f)) of the F distribution with (d1, d2) degrees of freedom"""
    f = float(f)
    if math.isnan(f):
        return math.nan, math.nan
    if math.isinf(f):
        return 1.0, 0.0
    den = d1 * f + d2
    return betainc_pair(0.5 * d1, 0.5 * d2, d1 * f / den, d2 / den)


def norm_sf(z: float) -> float:
    return 0.5 * math.erfc(float(z) / math.sqrt(2.0))


# ---- pieces ----------------------------------------------------------------------------------------------------------------
def _arr(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).reshape(-1)


def rankdata(x: np.ndarray) -> np.ndarray:
    """average ranks, 1-based (``scipy.stats.rankdata``)"""
    x = _arr(x)
    order = np.argsort(x, kind="mergesort")
    xs = x[order]
    first = np.r_[True, xs[1:] != xs[:-1]]
    start = np.flatnonzero(first)
    counts = np.diff(np.r_[start, xs.size])
    avg = start + (counts + 1) / 2.0                       # mean of start+1 .. start+count
    ranks = np.empty(x.size, dtype=np.float64)
    ranks[order] = np.repeat(avg, counts)
    return ranks


def _tie_counts(x: np.ndarray) -> np.ndarray:
    return np.unique(x, return_counts=True)[1].astype(np.float64)


def skewness(x) -> float:
    """biased: m3 / m2^1.5 (``scipy.stats.skew`` default); NaN for a constant sample"""
    x = _arr(x)
    mean = x.mean()
    d = x - mean
    m2, m3 = np.mean(d * d), np.mean(d * d * d)
    if m2 <= (np.finfo(np.float64).resolution * mean) ** 2:
        return float("nan")
    return float(m3 / m2 ** 1.5)


def kurtosis(x) -> float:
    """biased excess kurtosis: m4 / m2^2 - 3 (``scipy.stats.kurtosis`` default); NaN for a constant sample"""
    x = _arr(x)
    mean = x.mean()
    d = x - mean
    m2, m4 = np.mean(d * d), np.mean(d ** 4)
    if m2 <= (np.finfo(np.float64).resolution * mean) ** 2:
        return float("nan")
    return float(m4 / m2 ** 2.0 - 3.0)


def descriptive(data, name: str) -> Dict:
    """``compute_descriptive_stats`` (XAI.py:1744-1759)"""
    data = _arr(data)
    q25, q75 = np.percentile(data, 25), np.percentile(data, 75)
    return {"name": name, "n": len(data), "mean": np.mean(data), "median": np.median(data), "std": np.std(data, ddof=1),
            "var": np.var(data, ddof=1), "min": np.min(data), "max": np.max(data), "q25": q25, "q75": q75, "iqr": q75 - q25,
            "skewness": skewness(data), "kurtosis": kurtosis(data)}


def ttest_ind(a, b, equal_var: bool = True) -> Tuple[float, float]:
    """(t, two-sided p): Student's t-test with the pooled variance, or Welch's with the Welch-Satterthwaite df"""
    a, b = _arr(a), _arr(b)
    n1, n2 = a.size, b.size
    with np.errstate(all="ignore"):
        v1, v2 = np.var(a, ddof=1), np.var(b, ddof=1)
        if equal_var:
            df = np.float64(n1 + n2 - 2)
            svar = ((n1 - 1) * v1 + (n2 - 1) * v2) / df
            denom = np.sqrt(svar * (1.0 / n1 + 1.0 / n2))
        else:
            vn1, vn2 = v1 / n1, v2 / n2
            df = (vn1 + vn2) ** 2 / (vn1 ** 2 / (n1 - 1) + vn2 ** 2 / (n2 - 1))
            df = np.where(np.isnan(df), 1.0, df)[()]
            denom = np.sqrt(vn1 + vn2)
        t = np.float64(np.mean(a) - np.mean(b)) / denom
    return float(t), t_two_sided_p(t, df)


def _mwu_exact_sf(k: int, n1: int, n2: int) -> float:
    """P(U >= k) under the null without ties: the number of ways u inversions arise among C(n1 + n2, n1) arrangements
    (the coefficients of the Gaussian binomial), in exact integers"""
    top = n1 * n2
    ways = [1] + [0] * top                       # generating function prod_{i=1..n1} (1 - q^(n2+i)) / (1 - q^i)
    for i in range(1, n1 + 1):
        for u in range(top, n2 + i - 1, -1):     # times (1 - q^(n2+i))
            ways[u] -= ways[u - n2 - i]
        for u in range(i, top + 1):              # divided by (1 - q^i)
            ways[u] += ways[u - i]
    total = math.comb(n1 + n2, n1)
    k = max(0, int(k))
    return sum(ways[k:]) / total if k <= top else 0.0


def mannwhitneyu(a, b) -> Tuple[float, float, str]:
    """(U of the first sample, two-sided p, method) as ``scipy.stats.mannwhitneyu(a, b, alternative='two-sided')`` (method 'auto')"""
    a, b = _arr(a), _arr(b)
    n1, n2 = a.size, b.size
    both = np.concatenate([a, b])
    ranks = rankdata(both)
    u1 = float(ranks[:n1].sum() - n1 * (n1 + 1) / 2.0)
    u = max(u1, n1 * n2 - u1)
    t = _tie_counts(both)
    ties = bool(np.any(t > 1))
    if (n1 > 8 and n2 > 8) or ties:
        n = n1 + n2
        mu = n1 * n2 / 2.0
        tie_term = float((t ** 3 - t).sum())
        s = math.sqrt(n1 * n2 / 12.0 * ((n + 1) - tie_term / (n * (n - 1))))
        with np.errstate(all="ignore"):
            z = float((np.float64(u) - mu - 0.5) / np.float64(s))
        p = 2.0 * norm_sf(z)
        method = "asymptotic"
    else:
        p = 2.0 * _mwu_exact_sf(int(u), n1, n2)
        method = "exact"
    return u1, min(1.0, max(0.0, p)) if not math.isnan(p) else p, method


def ranksums(a, b) -> Tuple[float, float]:
    """(z, two-sided p) of ``scipy.stats.ranksums``: the rank sum of the first sample, normal approximation, no corrections"""
    a, b = _arr(a), _arr(b)
    n1, n2 = a.size, b.size
    ranks = rankdata(np.concatenate([a, b]))
    s = float(ranks[:n1].sum())
    expected = n1 * (n1 + n2 + 1) / 2.0
    z = (s - expected) / math.sqrt(n1 * n2 * (n1 + n2 + 1) / 12.0)
    return z, 2.0 * norm_sf(abs(z))


def cohens_d(a, b) -> Tuple[float, str]:
    """(d, 'negligible' | 'small' | 'medium' | 'large') of XAI.py:1815-1829; d = 0 when the pooled deviation is 0"""
    a, b = _arr(a), _arr(b)
    pooled = np.sqrt(((len(a) - 1) * np.var(a, ddof=1) + (len(b) - 1) * np.var(b, ddof=1)) / (len(a) + len(b) - 2))
    d = (np.mean(a) - np.mean(b)) / pooled if pooled > 0 else 0
    label = "negligible" if abs(d) < 0.2 else "small" if abs(d) < 0.5 else "medium" if abs(d) < 0.8 else "large"
    return d, label


def glass_delta(a, b):
    a, b = _arr(a), _arr(b)
    with np.errstate(all="ignore"):
        return (np.mean(a) - np.mean(b)) / np.std(b, ddof=1)


def levene(a, b) -> Tuple[float, float]:
    """(W, p) of ``scipy.stats.levene(a, b)`` (center='median'): one-way ANOVA of |x - median of its sample|"""
    groups = [_arr(a), _arr(b)]
    k = len(groups)
    z = [np.abs(g - np.median(g)) for g in groups]
    ni = np.array([g.size for g in groups], dtype=np.float64)
    zbari = np.array([zi.mean() for zi in z])
    ntot = ni.sum()
    zbar = np.sum(zbari * ni) / ntot
    numer = (ntot - k) * np.sum(ni * (zbari - zbar) ** 2)
    dvar = sum(np.sum((zi - zb) ** 2) for zi, zb in zip(z, zbari))
    with np.errstate(all="ignore"):
        w = np.float64(numer) / np.float64((k - 1) * dvar)
    return float(w), f_cdf_sf(w, k - 1, ntot - k)[1]


def f_test(a, b) -> Tuple[float, float]:
    """(F = var(a) / var(b), 2 * min(cdf, 1 - cdf)) of XAI.py:1950-1952"""
    a, b = _arr(a), _arr(b)
    with np.errstate(all="ignore"):
        f = np.var(a, ddof=1) / np.var(b, ddof=1)
    cdf, sf = f_cdf_sf(f, a.size - 1, b.size - 1)
    return float(f), 2.0 * min(cdf, sf)


def classical_tests(top_k, bottom_k, alpha: float) -> Dict:
    """The deterministic part of the reference's result (XAI.py:1761-1842, :1937-1959) with its keys: descriptive statistics,
    parametric and non-parametric tests, effect sizes and the variance tests."""
    top_k, bottom_k = _arr(top_k), _arr(bottom_k)
    t, tp = ttest_ind(top_k, bottom_k)
    wt, wp = ttest_ind(top_k, bottom_k, equal_var=False)
    u, up, _ = mannwhitneyu(top_k, bottom_k)
    rz, rp = ranksums(top_k, bottom_k)
    d, label = cohens_d(top_k, bottom_k)
    lw, lp = levene(top_k, bottom_k)
    f, fp = f_test(top_k, bottom_k)
    return {
        "descriptive_statistics": {"top_k": descriptive(top_k, "Top-k"), "bottom_k": descriptive(bottom_k, "Bottom-k")},
        "parametric_tests": {
            "t_test": {"statistic": t, "p_value": tp, "significant": tp < alpha, "description": "Independent samples t-test"},
            "welch_t_test": {"statistic": wt, "p_value": wp, "significant": wp < alpha,
                             "description": "Welch's t-test (unequal variances)"},
        },
        "nonparametric_tests": {
            "mann_whitney_u": {"statistic": u, "p_value": up, "significant": up < alpha, "description": "Mann-Whitney U test"},
            "wilcoxon_rank_sum": {"statistic": rz, "p_value": rp, "significant": rp < alpha,
                                  "description": "Wilcoxon rank-sum test"},
        },
        "effect_sizes": {
            "cohens_d": {"value": d, "interpretation": label, "description": "Cohen's d (standardized mean difference)"},
            "glass_delta": {"value": glass_delta(top_k, bottom_k), "description": "Glass's delta (using control group std)"},
        },
        "variance_tests": {
            "levene": {"statistic": lw, "p_value": lp, "equal_variances": lp > alpha,
                       "description": "Levene's test for equal variances"},
            "f_test": {"statistic": f, "p_value": fp, "equal_variances": fp > alpha, "description": "F-test for equal variances"},
        },
    }
