"""The host side of synt_isic_amd/evaluate.py without a GPU: the Frechet distance against closed forms, FeatureStats.merge against
the statistics of the whole, the unbiased MMD^2 and precision / recall against the restatement tests/eval_ref.py, the seeded
subset draw, three planted errors, and the conditioning conditions of every input set of tests/test_gpu_eval.py.

Planted errors, each measured against the bar the GPU suite holds that quantity to (the test asserts a factor >= 10):
    covariance divided by n (n = 300)                        relative error 3.3e-03 against bar 1.0e-05:    333 x
    MMD^2 with the diagonal left in                          against the bound propagated from bar 1.0e-05:      1.1e+03 x
    uncentred Gram-form distances, common offset 50          against bar 1.0e-05 of the centred matrix:         3.4e+03 x
"""
import numpy as np
import pytest
import torch

import eval_ref as er
from synt_isic_amd import evaluate as ev

F64_TOL = 1e-10          # float64 round-off of O(d^3) linear algebra at d <= 512, relative to the quantity's scale


def _stats(F):
    n, mu, cov = er.feature_stats(F)
    return ev.FeatureStats(n, mu, cov)


# ---- frechet_distance ------------------------------------------------------------------------------------------------------------
def test_frechet_closed_form_commuting_diagonal():
    """two Gaussians with diagonal covariances: |mu_a - mu_b|^2 + sum_i (sqrt(a_i) - sqrt(b_i))^2"""
    rng = np.random.default_rng(0)
    d = 16
    va, vb = rng.uniform(0.1, 4.0, d), rng.uniform(0.1, 4.0, d)
    va[3] = 0.0                                                   # a direction one set does not vary in
    mu_a, mu_b = rng.standard_normal(d), rng.standard_normal(d)
    want = ((mu_a - mu_b) ** 2).sum() + ((np.sqrt(va) - np.sqrt(vb)) ** 2).sum()
    got = ev.frechet_distance(ev.FeatureStats(100, mu_a, np.diag(va)), ev.FeatureStats(80, mu_b, np.diag(vb)))
    assert abs(got - want) <= F64_TOL * want
    # the same two in a rotated basis: still commuting, no longer diagonal
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    got = ev.frechet_distance(ev.FeatureStats(100, q @ mu_a, q @ np.diag(va) @ q.T), ev.FeatureStats(80, q @ mu_b, q @ np.diag(vb) @ q.T))
    assert abs(got - want) <= 1e-9 * want
    assert abs(er.frechet(mu_a, np.diag(va), mu_b, np.diag(vb)) - want) <= F64_TOL * want      # the restatement knows it too


def test_frechet_zero_symmetric_and_rank_deficient():
    rng = np.random.default_rng(1)
    a, b = _stats(rng.standard_normal((40, 64)) + 3.0), _stats(1.3 * rng.standard_normal((40, 64)) + 3.2)     # n = 40 < d = 64
    scale = np.trace(a.cov) + np.trace(b.cov)
    assert abs(ev.frechet_distance(a, a)) <= 1e-7 * scale       # sqrt loses half the digits at the 24 zero eigenvalues
    ab, ba = ev.frechet_distance(a, b), ev.frechet_distance(b, a)
    assert np.isfinite(ab) and ab > 0 and abs(ab - ba) <= 1e-7 * scale      # the same half of the digits
    assert abs(ab - er.frechet(a.mean, a.cov, b.mean, b.cov)) <= 1e-7 * scale


# ---- FeatureStats ------------------------------------------------------------------------------------------------------------------
def test_merge_of_three_ragged_shards_is_the_whole():
    rng = np.random.default_rng(2)
    F = rng.standard_normal((157, 24)) * rng.uniform(0.5, 3, 24) + 50.0
    whole = _stats(F)
    merged = ev.FeatureStats.merge(ev.FeatureStats.merge(_stats(F[:11]), _stats(F[11:90])), _stats(F[90:]))
    assert merged.n == 157
    assert np.abs(merged.mean - whole.mean).max() <= 1e-13 * np.abs(whole.mean).max()
    assert np.abs(merged.cov - whole.cov).max() <= 1e-11 * np.abs(whole.cov).max()
    back = ev.FeatureStats.from_state_dict(merged.state_dict())
    assert back.n == 157 and np.array_equal(back.mean, merged.mean) and np.array_equal(back.cov, merged.cov)


# ---- kernel distance ---------------------------------------------------------------------------------------------------------------
def test_mmd2_from_sums_is_the_restatement_and_straddles_zero():
    rng = np.random.default_rng(3)
    X, Y = rng.standard_normal((30, 8)) + 1.0, 1.2 * rng.standard_normal((25, 8)) + 1.1
    kxx, kyy, kxy = er.poly3(X, X), er.poly3(Y, Y), er.poly3(X, Y)
    got = ev.mmd2_unbiased(kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum(), 30, 25)
    want = er.mmd2(X, Y)
    assert abs(got - want) <= 1e-12 * kxx.max()
    # both sets from ONE distribution: the unbiased estimate has mean zero, so over many draws it takes both signs and its mean is
    # within three standard errors of zero
    est = []
    for _ in range(200):
        Z = rng.standard_normal((40, 8))
        est.append(er.mmd2(Z[:20], Z[20:]))
    est = np.array(est)
    assert (est > 0).any() and (est < 0).any()
    assert abs(est.mean()) <= 3 * est.std() / np.sqrt(len(est))


def test_subset_draw_is_a_pure_function_of_its_arguments():
    a, b = ev.subset_indices(7, 300, 200, 50, 5), ev.subset_indices(7, 300, 200, 50, 5)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    c = ev.subset_indices(8, 300, 200, 50, 5)
    assert not all(np.array_equal(x[0], y[0]) for x, y in zip(a, c))
    for ia, ib in a:
        assert len(set(ia.tolist())) == 50 and len(set(ib.tolist())) == 50 and ia.max() < 300 and ib.max() < 200
    with pytest.raises(ValueError):
        ev.subset_indices(0, 300, 200, 201, 1)


# ---- precision / recall --------------------------------------------------------------------------------------------------------------
def test_precision_recall_two_cluster_toy():
    """real: two far clusters of 30; generated: the first cluster's points moved by a hundredth of their spacing -> every
    generated point lies in its source's ball (precision 1), every real point of the first cluster in its twin's and none of the
    second in any (recall 1/2)"""
    rng = np.random.default_rng(4)
    real = np.concatenate([rng.standard_normal((30, 4)), rng.standard_normal((30, 4)) + 100.0])
    gen = real[:30] + 0.01 * rng.standard_normal((30, 4))
    want = er.precision_recall(gen, real, 3)
    got = ev.precision_recall_from_distances(er.sqdist(gen, gen), er.sqdist(real, real), er.sqdist(gen, real), 3)
    assert got == want
    assert got == (1.0, 0.5)


# ---- planted errors ------------------------------------------------------------------------------------------------------------------
def test_planted_errors_land_ten_times_over_the_gpu_bars():
    gen, real, _ = er.feature_sets(*er.PR_CASES[0])
    n, mu, cov = er.feature_stats(gen)
    # 1. covariance divided by n: against bar(e32) of the covariance, e32 = fp32 torch on the same centred inputs
    c32 = torch.from_numpy(gen) - torch.from_numpy(mu.astype(np.float32))
    e32 = er.rel_err((c32.T @ c32) / (n - 1), torch.from_numpy(cov))
    f_cov = er.rel_err(torch.from_numpy(cov * (n - 1) / n), torch.from_numpy(cov)) / er.bar(e32)
    # 2. MMD^2 with the diagonal left in: against the bound propagated from bar(e32) of the kernel matrices
    kxx, kyy, kxy = er.poly3(gen, gen), er.poly3(real, real), er.poly3(gen, real)
    e32 = er.rel_err(er.gram(gen, real, "poly3", dtype=torch.float32), torch.from_numpy(kxy))
    bound, _ = er.mmd2_bound(gen, real, er.bar(e32))
    f_mmd = abs(er.mmd2_from_kernels(kxx, kyy, kxy, diagonal_left_in=True) - er.mmd2_from_kernels(kxx, kyy, kxy)) / bound
    # 3. uncentred Gram-form distances: against bar(e32) of the centred distance matrix
    a, b = er.tight_feature_sets(200, 150, 512)
    D = er.sqdist(a, b)
    centre = b.astype(np.float64).mean(0).astype(np.float32)
    e32 = er.rel_err(torch.from_numpy(er.sqdist_gram_form(a, b, np.float32, centre)), torch.from_numpy(D))
    f_dist = er.rel_err(torch.from_numpy(er.sqdist_gram_form(a, b, np.float32, None)), torch.from_numpy(D)) / er.bar(e32)
    print(f"planted errors over their bars: covariance / n {f_cov:.3g} x, diagonal left in {f_mmd:.3g} x, uncentred {f_dist:.3g} x")
    assert f_cov >= 10 and f_mmd >= 10 and f_dist >= 10


# ---- the GPU suite's inputs meet their conditions ----------------------------------------------------------------------------------------
def test_gpu_inputs_meet_their_conditioning_conditions():
    for case in er.PR_CASES:
        gen, real, _ = er.feature_sets(*case)
        assert er.pr_margin_ok(gen, real, 3), case
        assert gen.min() > 0 and real.min() > 0 and abs(gen.mean() - er.OFFSET) < 1 and abs(real.mean() - er.OFFSET) < 1
        p, r = er.precision_recall(gen, real, 3)
        assert 0 < p < 1 and 0 < r < 1, (p, r)                  # a set where neither number is trivially 0 or 1
    A, B = er.neighbour_sets(*er.NN_CASE, er.NN_CANDIDATES + 1)
    assert A.shape == er.NN_CASE[::2] and er.neighbour_gaps_ok(A, B, er.NN_CANDIDATES + 1)
    for planted in ("exact", "near", None):
        gen, real, _ = er.image_sets(planted=planted)
        G, R = gen.reshape(len(gen), -1).astype(np.float64), real.reshape(len(real), -1).astype(np.float64)
        assert er.neighbour_gaps_ok(G, R, 6, allow_zero=True) and er.neighbour_gaps_ok(R, R, 6, exclude_self=True)
        if planted:
            d, i = er.knn(G, R, 1)
            assert i[er.PLANT_SLOT, 0] == er.PLANT_SRC and (d[er.PLANT_SLOT, 0] == 0) == (planted == "exact")
