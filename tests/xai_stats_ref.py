"""Reference side of the statistics stage (synt_isic_amd.xai_stats, sisic_resample_diffs): the scipy calls of
xai/XAI.py:1708-2005 for the recorded fixture, and the resampling contract of include/sisic.h restated in numpy over
tests/philox_ref.py -- written from the contract text, not from the kernel."""
import itertools

import numpy as np

import philox_ref

# the six-against-six input of the pipeline's default size (6 key frames x 1 intervention type per region)
TOP6 = np.array([0.31, 0.12, 0.44, 0.05, 0.27, 0.38])
BOTTOM6 = np.array([0.02, 0.21, -0.04, 0.15, 0.09, 0.33])
EXACT_PERM_P = 126 / 924            # |d| >= |observed| over all C(12, 6) relabellings = 0.13636...
OBSERVED_DIFF = 0.135

KEYS = ("t_stat", "t_p", "welch_stat", "welch_p", "mwu_stat", "mwu_p", "ranksums_stat", "ranksums_p", "levene_stat",
        "levene_p", "f_stat", "f_p", "skew_a", "kurt_a", "skew_b", "kurt_b")
STAT_KEYS = tuple(k for k in KEYS if not k.endswith("_p"))
P_KEYS = tuple(k for k in KEYS if k.endswith("_p"))


def case_inputs():
    """{name: (a, b)}: (6,6) without ties (the exact Mann-Whitney branch), (6,6) with ties, (2,2), (3,8), (9,12), (42,42)"""
    rng = np.random.default_rng(20240607)
    cases = {"n6_6": (TOP6.copy(), BOTTOM6.copy()),
             "n6_6_ties": (np.array([0.3, 0.1, 0.4, 0.1, 0.3, 0.4]), np.array([0.0, 0.2, 0.1, 0.2, 0.1, 0.3]))}
    for n1, n2 in ((2, 2), (3, 8), (9, 12), (42, 42)):
        cases[f"n{n1}_{n2}"] = (rng.normal(0.25, 0.15, n1), rng.normal(0.1, 0.1 + 0.002 * n2, n2))
    return cases


def scipy_values(a, b) -> np.ndarray:
    """float64 [len(KEYS)]: what the reference's scipy calls return for (a, b)"""
    from scipy import stats
    t = stats.ttest_ind(a, b)
    w = stats.ttest_ind(a, b, equal_var=False)
    u = stats.mannwhitneyu(a, b, alternative="two-sided")
    r = stats.ranksums(a, b)
    lv = stats.levene(a, b)
    f = np.var(a, ddof=1) / np.var(b, ddof=1)
    cdf = stats.f.cdf(f, len(a) - 1, len(b) - 1)
    fp = 2 * min(cdf, 1 - cdf)
    return np.array([t[0], t[1], w[0], w[1], u[0], u[1], r[0], r[1], lv[0], lv[1], f, fp, stats.skew(a), stats.kurtosis(a),
                     stats.skew(b), stats.kurtosis(b)], dtype=np.float64)


def have_scipy() -> bool:
    try:
        import scipy.stats  # noqa: F401
        return True
    except Exception:
        return False


def load_fixture(path):
    z = np.load(path)
    return {name: (z[name + "_a"], z[name + "_b"], dict(zip(KEYS, z[name + "_vals"]))) for name in case_inputs()}


# ---- the resampling contract ------------------------------------------------------------------------------------------------
def resample_words(seed: int, tag: int, n_resamples: int, n: int) -> np.ndarray:
    """uint64 [n_resamples, n]: row r = the first n words of the block stream (seed, step = r, tag) = noise_bits(n, step r)"""
    nq = (n + 3) // 4
    ctr = np.zeros((n_resamples * nq, 4), dtype=np.uint32)
    ctr[:, 0] = np.tile(np.arange(nq, dtype=np.uint32), n_resamples)
    ctr[:, 1] = np.repeat(np.arange(n_resamples, dtype=np.uint32), nq)
    ctr[:, 2] = np.uint32(tag)
    seed = int(seed)
    w = philox_ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(n_resamples, nq * 4)
    return w[:, :n].astype(np.uint64)


def bootstrap_diffs(top, bottom, seed: int, n_resamples: int) -> np.ndarray:
    """tag 3: s1 = sum_j top[(w[j] * n_top) >> 32], s2 = sum_j bottom[(w[n_top + j] * n_bottom) >> 32], sequential in j, double"""
    top, bottom = np.asarray(top, np.float64), np.asarray(bottom, np.float64)
    n1, n2 = top.size, bottom.size
    w = resample_words(seed, 3, n_resamples, n1 + n2)
    s1 = np.zeros(n_resamples)
    for j in range(n1):
        s1 = s1 + top[((w[:, j] * np.uint64(n1)) >> np.uint64(32)).astype(np.int64)]
    s2 = np.zeros(n_resamples)
    for j in range(n2):
        s2 = s2 + bottom[((w[:, n1 + j] * np.uint64(n2)) >> np.uint64(32)).astype(np.int64)]
    return s1 / n1 - s2 / n2


def permutation_diffs(top, bottom, seed: int, n_resamples: int) -> np.ndarray:
    """tag 4: selection sampling -- element i joins the n_top-subset when (w[i] * (N - i)) >> 32 < need"""
    top, bottom = np.asarray(top, np.float64), np.asarray(bottom, np.float64)
    n1, n2 = top.size, bottom.size
    n = n1 + n2
    comb = np.concatenate([top, bottom])
    w = resample_words(seed, 4, n_resamples, n)
    need = np.full(n_resamples, n1, dtype=np.int64)
    s1 = np.zeros(n_resamples)
    s2 = np.zeros(n_resamples)
    for i in range(n):
        take = ((w[:, i] * np.uint64(n - i)) >> np.uint64(32)).astype(np.int64) < need
        s1 = np.where(take, s1 + comb[i], s1)
        s2 = np.where(take, s2, s2 + comb[i])
        need = need - take
    assert np.all(need == 0)
    return s1 / n1 - s2 / n2


def exact_permutation_p(top, bottom) -> float:
    """mean(|d| >= |observed|) over every n_top-subset of the pooled values"""
    top, bottom = np.asarray(top, np.float64), np.asarray(bottom, np.float64)
    comb = np.concatenate([top, bottom])
    n1, n = top.size, comb.size
    obs = abs(top.mean() - bottom.mean())
    hits = total = 0
    for s in itertools.combinations(range(n), n1):
        inside = np.zeros(n, dtype=bool)
        inside[list(s)] = True
        hits += abs(comb[inside].mean() - comb[~inside].mean()) >= obs
        total += 1
    return hits / total
