"""The statistics stage without a GPU: synt_isic_amd.xai_stats against scipy, and the resampling contract of
sisic_resample_diffs as a distribution.

Classical tests: the expected values were recorded with scipy 1.15.3 into tests/golden/xai_stats.npz
(tests/golden/make_xai_stats.py) and are compared live as well where scipy is installed.  Statistics to 1e-12 relative,
p-values to 1e-10 relative for p >= 1e-12: a textbook continued fraction agrees with scipy's ``t.sf`` to 1.1e-12 over 20 000
draws with df 2 .. 200 and t <= 8 and with ``f.cdf`` to 5e-14, and the bound is about 100 times that.

Resampling: the contract (include/sisic.h) restated in numpy over tests/philox_ref.py gives, for the six-against-six input and
seeds 0 and 12345, a 10 000-sample permutation p within 4 standard errors sqrt(p (1 - p) / 10000) of the exact p over all 924
subsets, and a mean of 1 000 bootstrap differences within 4 standard errors of the observed difference."""
import os
import subprocess
import sys

import numpy as np
import pytest

import xai_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(ref.case_inputs())


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return ref.load_fixture(os.path.join(golden_dir, "xai_stats.npz"))


def _ours(a, b):
    from synt_isic_amd import xai_stats as xs
    t, w, u, r, lv, f = (xs.ttest_ind(a, b), xs.ttest_ind(a, b, equal_var=False), xs.mannwhitneyu(a, b), xs.ranksums(a, b),
                         xs.levene(a, b), xs.f_test(a, b))
    vals = [t[0], t[1], w[0], w[1], u[0], u[1], r[0], r[1], lv[0], lv[1], f[0], f[1], xs.skewness(a), xs.kurtosis(a),
            xs.skewness(b), xs.kurtosis(b)]
    return dict(zip(ref.KEYS, vals)), u[2]


def _compare(got, want, what):
    for k in ref.STAT_KEYS:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), f"{what}: {k} = {got[k]!r}, scipy {want[k]!r}"
    for k in ref.P_KEYS:
        if want[k] < 1e-12:            # below the range the relative bound covers (Levene on two pairs: no spread within a sample)
            assert 0.0 <= got[k] < 1e-12, f"{what}: {k} = {got[k]!r}, scipy {want[k]!r}"
            continue
        assert abs(got[k] - want[k]) <= 1e-10 * want[k], f"{what}: {k} = {got[k]!r}, scipy {want[k]!r}"


@pytest.mark.parametrize("case", CASES)
def test_classical_tests_match_scipy(fixture, case):
    a, b, want = fixture[case]
    a0, b0 = ref.case_inputs()[case]
    assert np.array_equal(a, a0) and np.array_equal(b, b0), "the fixture was recorded for other inputs: regenerate it"
    got, method = _ours(a, b)
    ties = np.unique(np.concatenate([a, b])).size < a.size + b.size
    assert method == ("exact" if min(a.size, b.size) <= 8 and not ties else "asymptotic")
    _compare(got, want, f"{case} (fixture)")
    if ref.have_scipy():
        _compare(got, dict(zip(ref.KEYS, ref.scipy_values(a, b))), f"{case} (live scipy)")


def test_cases_cover_both_mann_whitney_branches(fixture):
    methods = {case: _ours(*fixture[case][:2])[1] for case in CASES}
    assert methods["n6_6"] == "exact" and methods["n6_6_ties"] == "asymptotic" and methods["n2_2"] == "exact"
    assert methods["n3_8"] == "exact" and methods["n9_12"] == "asymptotic" and methods["n42_42"] == "asymptotic"


def test_classical_dictionary_and_descriptives(fixture):
    """the keys of XAI.py:1744-1842 / :1937-1959, Cohen's four-way label and Glass's delta"""
    from synt_isic_amd import xai_stats as xs
    a, b, want = fixture["n6_6"]
    res = xs.classical_tests(a, b, 0.1)
    assert set(res) == {"descriptive_statistics", "parametric_tests", "nonparametric_tests", "effect_sizes", "variance_tests"}
    d = res["descriptive_statistics"]["top_k"]
    assert set(d) == {"name", "n", "mean", "median", "std", "var", "min", "max", "q25", "q75", "iqr", "skewness", "kurtosis"}
    assert d["name"] == "Top-k" and d["n"] == 6 and d["mean"] == np.mean(a) and d["std"] == np.std(a, ddof=1)
    assert d["iqr"] == np.percentile(a, 75) - np.percentile(a, 25)
    assert res["parametric_tests"]["t_test"]["p_value"] == xs.ttest_ind(a, b)[1]
    assert res["parametric_tests"]["t_test"]["significant"] == (want["t_p"] < 0.1)
    assert set(res["nonparametric_tests"]) == {"mann_whitney_u", "wilcoxon_rank_sum"}
    assert res["variance_tests"]["levene"]["equal_variances"] == (want["levene_p"] > 0.1)
    pooled = np.sqrt((5 * np.var(a, ddof=1) + 5 * np.var(b, ddof=1)) / 10)
    assert res["effect_sizes"]["cohens_d"]["value"] == (np.mean(a) - np.mean(b)) / pooled
    assert res["effect_sizes"]["glass_delta"]["value"] == (np.mean(a) - np.mean(b)) / np.std(b, ddof=1)
    base = np.array([0.0, 1.0, 2.0, 3.0])
    for shift, label in ((0.1, "negligible"), (0.5, "small"), (0.9, "medium"), (1.5, "large")):      # pooled deviation 1.29
        assert xs.cohens_d(base + shift, base)[1] == label
    assert xs.cohens_d(np.ones(3), np.ones(3)) == (0, "negligible")


def test_upper_tails_keep_their_relative_accuracy():
    """a far tail is the complementary beta function, not 1 - cdf: it stays positive and smooth where 1 - cdf is 0"""
    from synt_isic_amd import xai_stats as xs
    cdf, sf = xs.f_cdf_sf(1e9, 3, 40)
    assert cdf == 1.0 and 0.0 < sf < 1e-30
    lo, hi = xs.f_cdf_sf(1e-9, 3, 40)
    assert 0.0 < lo < 1e-12 and hi == 1.0 - lo
    assert 0.0 < xs.t_two_sided_p(60.0, 10) < 1e-13
    assert xs.t_two_sided_p(0.0, 7) == 1.0


def test_xai_stats_does_not_import_scipy():
    code = ("import sys; import synt_isic_amd.xai_stats as xs; import numpy as np; "
            "xs.classical_tests(np.arange(6.0) ** 1.5, np.arange(7.0), 0.1); "
            "bad = [m for m in sys.modules if m == 'scipy' or m.startswith('scipy.')]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    src = open(os.path.join(ROOT, "synt_isic_amd", "xai_stats.py")).read()
    assert "import scipy" not in src and "from scipy" not in src and "import torch" not in src


# ---- the resampling contract ------------------------------------------------------------------------------------------------
def test_exact_permutation_p():
    assert abs(ref.exact_permutation_p(ref.TOP6, ref.BOTTOM6) - ref.EXACT_PERM_P) < 1e-15
    assert abs(ref.EXACT_PERM_P - 0.13636) < 1e-5
    assert abs((ref.TOP6.mean() - ref.BOTTOM6.mean()) - ref.OBSERVED_DIFF) < 1e-15


def test_resample_words_are_the_noise_bits():
    import philox_ref
    w = ref.resample_words(5, 3, 4, 13)
    for r in range(4):
        assert np.array_equal(w[r].astype(np.uint32), philox_ref.noise_bits(5, r, 3, 13)[:13])


@pytest.mark.parametrize("seed", [0, 12345])
def test_permutation_p_within_four_standard_errors(seed):
    d = ref.permutation_diffs(ref.TOP6, ref.BOTTOM6, seed, 10000)
    p = np.mean(np.abs(d) >= abs(ref.TOP6.mean() - ref.BOTTOM6.mean()))
    se = np.sqrt(ref.EXACT_PERM_P * (1 - ref.EXACT_PERM_P) / 10000)
    print(f"seed {seed}: permutation p = {p}, exact {ref.EXACT_PERM_P:.5f}, z = {(p - ref.EXACT_PERM_P) / se:+.2f}")
    assert abs(p - ref.EXACT_PERM_P) <= 4 * se


@pytest.mark.parametrize("seed", [0, 12345])
def test_bootstrap_mean_within_four_standard_errors(seed):
    d = ref.bootstrap_diffs(ref.TOP6, ref.BOTTOM6, seed, 1000)
    # a bootstrap mean of n draws has variance var_biased / n; the two samples are drawn independently
    se = np.sqrt((ref.TOP6.var() / 6 + ref.BOTTOM6.var() / 6) / 1000)
    obs = ref.TOP6.mean() - ref.BOTTOM6.mean()
    print(f"seed {seed}: bootstrap mean = {d.mean()}, observed {obs}, z = {(d.mean() - obs) / se:+.2f}")
    assert abs(d.mean() - obs) <= 4 * se
