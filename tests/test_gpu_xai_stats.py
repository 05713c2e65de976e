"""sisic_resample_diffs and ``xai.statistical_validation`` on the GPU.

The kernel is BIT-EQUAL to the numpy restatement of its contract (tests/xai_stats_ref.py over tests/philox_ref.py): the words are
integers, the index maps are integer multiplies, and every sum is sequential in index order in double without contraction, so
there is nothing to round differently.  Sizes: ordinary ones, (5,9) with a partial last Philox block, (300,217) = 130 blocks per
resample; counts (1000, 10000) = 4 + 40 workgroups with partial last ones, and (7, 13).  The permutation p of the
six-against-six input is within 4 standard errors sqrt(p (1 - p) / 10000) of the exact p over all 924 subsets."""
import numpy as np
import pytest
import torch

import xai_stats_ref as ref

from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [(1, 1), (2, 3), (6, 6), (42, 42), (5, 9), (300, 217)]


def _samples(n_top, n_bottom):
    if (n_top, n_bottom) == (6, 6):
        return ref.TOP6.copy(), ref.BOTTOM6.copy()
    rng = np.random.default_rng(1000 * n_top + n_bottom)
    return rng.normal(0.2, 0.3, n_top), rng.normal(0.0, 0.2, n_bottom)


@pytest.mark.parametrize("counts", [(1000, 10000), (7, 13)])
@pytest.mark.parametrize("sizes", SIZES)
def test_resample_diffs_bit_equal_to_the_contract(sizes, counts):
    from synt_isic_amd import ops
    top, bottom = _samples(*sizes)
    for seed in (0, 12345):
        boot, perm = ops.resample_diffs(top, bottom, seed, counts[0], counts[1], DEV)
        assert boot.dtype == torch.float64 and tuple(boot.shape) == (counts[0],) and tuple(perm.shape) == (counts[1],)
        want_b = ref.bootstrap_diffs(top, bottom, seed, counts[0])
        want_p = ref.permutation_diffs(top, bottom, seed, counts[1])
        got_b, got_p = boot.cpu().numpy(), perm.cpu().numpy()
        assert np.array_equal(got_b, want_b), f"{sizes} seed {seed}: {np.sum(got_b != want_b)} bootstrap values differ"
        assert np.array_equal(got_p, want_p), f"{sizes} seed {seed}: {np.sum(got_p != want_p)} permutation values differ"
    if sizes[0] + sizes[1] > 2:
        assert np.unique(got_p).size > 1 and np.unique(got_b).size > 1


def test_one_output_left_out():
    from synt_isic_amd import ops
    top, bottom = _samples(5, 9)
    boot, perm = ops.resample_diffs(top, bottom, 12345, 7, 13, DEV)
    none, perm_only = ops.resample_diffs(top, bottom, 12345, 0, 13, DEV)
    boot_only, none2 = ops.resample_diffs(top, bottom, 12345, 7, 0, DEV)
    assert none is None and none2 is None
    assert torch.equal(perm_only, perm) and torch.equal(boot_only, boot)


def test_bad_sizes_are_refused_with_a_message():
    from synt_isic_amd import _lib, ops
    with pytest.raises(_lib.SisicError, match="resample_diffs") as e:
        ops.resample_diffs(np.zeros(2000), np.zeros(2097), 0, 7, 13, DEV)
    assert e.value.code == _lib.SISIC_EINVAL and "4096" in str(e.value)
    with pytest.raises(_lib.SisicError, match="resample_diffs") as e:
        ops.resample_diffs(np.zeros(0), np.zeros(5), 0, 7, 13, DEV)
    assert e.value.code == _lib.SISIC_EINVAL
    boot, perm = ops.resample_diffs(np.arange(2000.0), np.arange(2096.0), 0, 3, 3, DEV)       # N = 4096 is taken
    assert np.array_equal(perm.cpu().numpy(), ref.permutation_diffs(np.arange(2000.0), np.arange(2096.0), 0, 3))
    assert np.array_equal(boot.cpu().numpy(), ref.bootstrap_diffs(np.arange(2000.0), np.arange(2096.0), 0, 3))


REFERENCE_KEYS = {"descriptive_statistics", "parametric_tests", "nonparametric_tests", "effect_sizes", "bootstrap_analysis",
                  "permutation_analysis", "normality_tests", "variance_tests", "significance_consensus", "overall_conclusion",
                  "metadata"}


def _same(a, b, path=""):
    """two result dictionaries hold the same values (numpy arrays included); the wall-clock stamp aside"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            if k != "analysis_timestamp":
                _same(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b, equal_nan=True), path
    elif isinstance(a, float) and np.isnan(a):
        assert np.isnan(b), path
    else:
        assert a == b, path


@pytest.mark.parametrize("seed", [0, 12345])
def test_statistical_validation(seed):
    from synt_isic_amd import xai, xai_stats
    res = xai.statistical_validation(ref.TOP6, ref.BOTTOM6, seed=seed)
    assert set(res) == REFERENCE_KEYS
    p = res["permutation_analysis"]["p_value"]
    se = np.sqrt(ref.EXACT_PERM_P * (1 - ref.EXACT_PERM_P) / 10000)
    print(f"seed {seed}: permutation p = {p}, exact {ref.EXACT_PERM_P:.5f}, z = {(p - ref.EXACT_PERM_P) / se:+.2f}")
    assert abs(p - ref.EXACT_PERM_P) <= 4 * se
    want_d = ref.permutation_diffs(ref.TOP6, ref.BOTTOM6, seed, 10000)
    assert p == np.mean(np.abs(want_d) >= abs(ref.TOP6.mean() - ref.BOTTOM6.mean()))
    host = xai_stats.classical_tests(ref.TOP6, ref.BOTTOM6, 0.1)
    for k in host:
        _same(res[k], host[k], k)

    boot = res["bootstrap_analysis"]
    assert set(boot) == {"bootstrap_diffs", "mean_diff", "ci_lower", "ci_upper", "ci_contains_zero", "confidence_level"}
    diffs = ref.bootstrap_diffs(ref.TOP6, ref.BOTTOM6, seed, 1000)
    assert np.array_equal(boot["bootstrap_diffs"], diffs)
    level = 1 - 0.1                                                   # the reference's two percentile levels (XAI.py:1860-1861)
    assert boot["ci_lower"] == np.percentile(diffs, (1 - level) / 2 * 100)
    assert boot["ci_upper"] == np.percentile(diffs, (1 + level) / 2 * 100)
    assert boot["ci_contains_zero"] == bool(boot["ci_lower"] <= 0 <= boot["ci_upper"]) and boot["confidence_level"] == 0.9
    perm = res["permutation_analysis"]
    assert set(perm) == {"observed_difference", "permuted_differences", "p_value", "significant", "n_permutations"}
    assert perm["n_permutations"] == 10000 and perm["significant"] == (p < 0.1)
    assert perm["observed_difference"] == ref.TOP6.mean() - ref.BOTTOM6.mean()
    for test in ("shapiro_wilk", "kolmogorov_smirnov"):
        for side in ("top_k", "bottom_k"):
            assert res["normality_tests"][test][side]["skipped"] is True and res["normality_tests"][test][side]["reason"]
    cons = res["significance_consensus"]
    assert cons == {
        "parametric_significant": any(t["significant"] for t in res["parametric_tests"].values()),
        "nonparametric_significant": any(t["significant"] for t in res["nonparametric_tests"].values()),
        "bootstrap_significant": not boot["ci_contains_zero"], "permutation_significant": perm["significant"]}
    concl = res["overall_conclusion"]
    assert concl["significant_tests_count"] == sum(cons.values()) and concl["total_tests_count"] == 4
    assert concl["significant"] == (sum(cons.values()) >= 3) and concl["alpha_level"] == 0.1
    assert concl["recommendation"] == ("significant" if concl["significant"] else "not_significant")
    assert res["metadata"]["seed"] == seed and res["metadata"]["n_bootstrap_samples"] == 1000
    assert set(res["metadata"]) == {"analysis_timestamp", "n_bootstrap_samples", "n_permutations", "alpha_level", "seed"}

    _same(res, xai.statistical_validation(ref.TOP6, ref.BOTTOM6, seed=seed))
    other = xai.statistical_validation(ref.TOP6, ref.BOTTOM6, seed=seed + 1)
    assert not np.array_equal(other["bootstrap_analysis"]["bootstrap_diffs"], diffs)


def test_statistical_validation_insufficient_data():
    from synt_isic_amd import xai
    for top, bottom in (([0.1], [0.2, 0.3]), ([0.1, 0.2], [0.3]), ([], [])):
        with pytest.raises(ValueError, match="Insufficient data"):
            xai.statistical_validation(top, bottom)
