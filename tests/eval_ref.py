"""Float64 numpy restatement of the evaluation metrics of synt_isic_amd/evaluate.py, written from the three papers (imported by
test_eval_cpu.py and test_gpu_eval.py, as clf_train_ref / xai_stats_ref are by theirs), and the seeded inputs of both suites.

    feature_stats        mean and covariance (divisor n - 1)
    frechet              Heusel et al. 2017, eq. 6: |mu_a - mu_b|^2 + tr(S_a + S_b - 2 (S_a S_b)^(1/2)); the trace of the root from
                         the eigenvalues of the product S_a S_b (numpy.linalg.eigvals on the unsymmetric product: another route
                         than the library's two symmetric decompositions)
    poly3, mmd2          Binkowski et al. 2018: k(x, y) = (x.y / d + 1)^3, the unbiased MMD^2 estimate written as three double loops'
                         worth of sums
    sqdist               sum_c (a_c - b_c)^2, subtracting first
    precision_recall     Kynkaanniemi et al. 2019, eq. 1-2, by brute force
    knn, rows_topk       brute-force neighbours by a stable argsort (ties to the lower index)
    gram                 the library's three epilogues in torch, float64 or float32 (the fp32 yardstick of ``bar``)
    rel_err, bar         clf_train_ref's: max|x - x64| / max|x64| <= max(1e-5, 16 e32)

Inputs.  ``feature_sets`` draws features that are positive with a large common mean (50), as pooled ReLU features are, from a
latent of few dimensions, so neighbour distances spread over orders of magnitude instead of concentrating.  The GPU tests need
their references well conditioned -- a neighbour list or a membership decision that hangs on the seventh digit tests the
rounding, not the code -- so every input set is drawn by seed until its float64 reference meets its condition
(``neighbour_gaps_ok``, ``pr_margin_ok``); test_eval_cpu.py asserts the conditions again, without a GPU.
"""
import numpy as np
import torch

from clf_train_ref import bar, rel_err  # noqa: F401

GAP = 1e-3            # the conditioning conditions: relative gap between consecutive neighbours, relative margin of a decision
OFFSET = 50.0


# ---- the metrics -------------------------------------------------------------------------------------------------------------
def feature_stats(F):
    F = np.asarray(F, np.float64)
    mu = F.mean(0)
    c = F - mu
    return F.shape[0], mu, c.T @ c / (F.shape[0] - 1)


def frechet(mu_a, cov_a, mu_b, cov_b):
    lam = np.linalg.eigvals(cov_a @ cov_b)
    root_trace = np.sqrt(np.maximum(lam.real, 0.0)).sum()
    return float(((mu_a - mu_b) ** 2).sum() + np.trace(cov_a) + np.trace(cov_b) - 2.0 * root_trace)


def poly3(X, Y):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return (X @ Y.T / X.shape[1] + 1.0) ** 3


def mmd2_from_kernels(kxx, kyy, kxy, diagonal_left_in=False):
    n, m = kxy.shape
    if diagonal_left_in:                       # the planted error: the biased V-statistic's sums under the unbiased divisors
        return float(kxx.sum() / (n * (n - 1)) + kyy.sum() / (m * (m - 1)) - 2.0 * kxy.mean())
    return float((kxx.sum() - np.trace(kxx)) / (n * (n - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2.0 * kxy.mean())


def mmd2(X, Y):
    return mmd2_from_kernels(poly3(X, X), poly3(Y, Y), poly3(X, Y))


def sqdist(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        out[i] = ((A[i][None, :] - B) ** 2).sum(1)
    return out


def sqdist_gram_form(A, B, dtype=np.float32, centre=None):
    """|a|^2 + |b|^2 - 2 a.b in ``dtype``, the operands centred on ``centre`` first (None: not at all -- the planted error)"""
    A, B = np.asarray(A, dtype), np.asarray(B, dtype)
    if centre is not None:
        A, B = A - np.asarray(centre, dtype), B - np.asarray(centre, dtype)
    return np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * (A @ B.T), 0)


def kth_radius2(D, k):
    """squared distance to the k-th nearest other point, from a square matrix"""
    D = np.array(D, np.float64)
    np.fill_diagonal(D, np.inf)
    return np.sort(D, axis=1)[:, k - 1]


def pr_decisions(G, R, k):
    """(q_g [n], q_r [m]): min_j D[i,j] / radius_j^2 - 1 -- generated i lies in the real manifold iff q_g[i] <= 0, and so on"""
    d_gr = sqdist(G, R)
    rad_g, rad_r = kth_radius2(sqdist(G, G), k), kth_radius2(sqdist(R, R), k)
    return (d_gr / rad_r[None, :]).min(1) - 1.0, (d_gr.T / rad_g[None, :]).min(1) - 1.0


def precision_recall(G, R, k=3):
    q_g, q_r = pr_decisions(G, R, k)
    return float((q_g <= 0).mean()), float((q_r <= 0).mean())


def rows_topk(D, k, col_offset=None, skip_diagonal=False):
    """(values, columns) of the k smallest of D[i,j] - col_offset[j] per row in D's dtype, by a stable argsort"""
    X = np.array(D)
    if col_offset is not None:
        X = X - np.asarray(col_offset, X.dtype)[None, :]
    if skip_diagonal:
        r = np.arange(min(X.shape))
        X[r, r] = np.inf
    order = np.argsort(X, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(X, order, 1), order.astype(np.int32)


def knn(A, B, k, exclude_self=False):
    """(sqdist float64 [n,k], index [n,k]) by brute force in float64"""
    D = sqdist(A, B)
    return rows_topk(D, k, skip_diagonal=exclude_self)


def pair_sqdist(A, B, idx):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return ((A[:, None, :] - B[np.asarray(idx, np.int64)]) ** 2).sum(-1)


def gram(A, B, mode, shift_a=None, shift_b=None, dtype=torch.float64, contract_rows=False):
    """the library's sisic_gram in torch at ``dtype``: the same fp32 inputs, shifted, multiplied and finished in that dtype"""
    a = torch.as_tensor(A).to(dtype)
    b = a if B is None else torch.as_tensor(B).to(dtype)
    if shift_a is not None:
        a = a - torch.as_tensor(shift_a).to(dtype)
    if contract_rows:
        return a.T @ a
    if shift_b is not None:
        b = b - torch.as_tensor(shift_b).to(dtype)
    s = a @ b.T
    if mode == "dot":
        return s
    if mode == "sqdist":
        return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * s).clamp(min=0)
    return (s / a.shape[1] + 1) ** 3


# ---- conditions --------------------------------------------------------------------------------------------------------------
def neighbour_gaps_ok(A, B, first, exclude_self=False, allow_zero=False):
    """every row's consecutive float64 neighbour distances among the first ``first`` differ by more than GAP of the larger one
    (allow_zero: an exact copy's distance 0 is a neighbour like any other -- its gap to the next is the next distance)"""
    D = sqdist(A, B)
    if exclude_self:
        np.fill_diagonal(D, np.inf)
    s = np.sort(D, axis=1)[:, :first]
    if not allow_zero and not (s[:, 0] > 0).all():
        return False
    return bool(((s[:, 1:] - s[:, :-1]) > GAP * s[:, 1:]).all())


def pr_margin_ok(G, R, k):
    q_g, q_r = pr_decisions(G, R, k)
    return bool((np.abs(q_g) > GAP).all() and (np.abs(q_r) > GAP).all())


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _low_rank(rng, n, d, W, scale, shift):
    z = scale * rng.standard_normal((n, W.shape[0])) + shift
    return (OFFSET + z @ W + 0.05 * rng.standard_normal((n, d))).astype(np.float32)


def _draw_feature_sets(n, m, d, seed, r=5):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((r, d)) / np.sqrt(r)
    real = _low_rank(rng, m, d, W, 1.0, 0.0)
    gen = _low_rank(rng, n, d, W, 0.7, 0.6)        # a narrower, displaced distribution: precision and recall both strictly inside (0, 1)
    return gen, real


def feature_sets(n, m, d, k=3, seed0=0):
    """(generated [n,d], real [m,d], seed) fp32, positive with a common mean of 50: the first seed from ``seed0`` on whose float64
    reference meets ``pr_margin_ok(k)``"""
    for seed in range(seed0, seed0 + 200):
        gen, real = _draw_feature_sets(n, m, d, seed)
        if pr_margin_ok(gen, real, k):
            return gen, real, seed
    raise AssertionError("no seed gives a well-conditioned reference")


def neighbour_sets(n, m, d, first, seed=0):
    """(A [n,d], B [m,d]) fp32 of the same kind for the neighbour tests: 4 n rows are drawn and the first n kept whose own
    float64 neighbour list in B meets ``neighbour_gaps_ok(first)`` (a condition on one row at a time, so rows are chosen, not seeds)"""
    pool, real = _draw_feature_sets(4 * n, m, d, 500 + seed)
    keep = [i for i in range(pool.shape[0]) if neighbour_gaps_ok(pool[i:i + 1], real, first)][:n]
    assert len(keep) == n, "too few well-conditioned rows"
    return pool[keep], real


PR_CASES = [(300, 200, 64), (120, 90, 512)]          # (generated, real, d) of the statistics / distance tests
NN_CASE = (200, 150, 512)                            # feature-space neighbours
NN_K, NN_CANDIDATES = 3, 7                           # k and min(8, k + 4)
IMG_CASE = (24, 16, 32)                              # generated, real, side: pixel space and evaluate_generated
PLANT_SLOT, PLANT_SRC = 7, 5                         # real image 5 planted at generated slot 7


def image_sets(seed0=0, planted="exact"):
    """(generated uint8 [24,32,32,3], real uint8 [16,32,32,3], seed): smooth random images (a few low-frequency patterns under
    each, so distances spread), real image PLANT_SRC copied to generated slot PLANT_SLOT -- ``exact``ly, ``near``ly (+-1 in
    1 % of the bytes) or not at all (None); the first seed whose float64 neighbour references (generated -> real among the first
    6, real -> other real among the first 6) meet ``neighbour_gaps_ok``"""
    n, m, side = IMG_CASE
    d = side * side * 3
    for seed in range(seed0, seed0 + 200):
        rng = np.random.default_rng(1000 + seed)
        basis = rng.standard_normal((6, d))
        def draw(count):
            z = rng.standard_normal((count, 6)) * np.array([40, 30, 25, 20, 15, 10.0])
            return np.clip(np.rint(128 + z @ basis / 2 + 6 * rng.standard_normal((count, d))), 0, 255).astype(np.uint8)
        real, gen = draw(m), draw(n)
        if planted is not None:
            gen[PLANT_SLOT] = real[PLANT_SRC]
            if planted == "near":
                where = rng.choice(d, size=d // 100, replace=False)
                row = gen[PLANT_SLOT].astype(np.int64)
                row[where] += np.where(row[where] >= 255, -1, np.where(row[where] <= 0, 1, rng.choice([-1, 1], size=where.size)))
                gen[PLANT_SLOT] = row.astype(np.uint8)
        G, R = gen.astype(np.float64), real.astype(np.float64)
        if neighbour_gaps_ok(G, R, 6, allow_zero=True) and neighbour_gaps_ok(R, R, 6, exclude_self=True):
            return gen.reshape(n, side, side, 3), real.reshape(m, side, side, 3), seed
    raise AssertionError("no seed gives a well-conditioned reference")


def gram_inputs(n, m, d, seed):
    """fp32 operands and shifts of the ops.gram tests: A ~ N(0, 1), B ~ N(0.5, 1), shifts ~ N(0, 0.1)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g), torch.randn(m, d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1,
            torch.randn(d, generator=g) * 0.1)


# ---- bounds propagated from ``bar`` --------------------------------------------------------------------------------------------
# The library's mean, covariance and kernel matrices are held to ``bar``: an error of at most eps = bar(e32) times the largest
# entry, anywhere.  What that allows in a scalar computed FROM them is measured, not guessed: the restatement is evaluated on
# inputs perturbed by +-eps * max|x| in every entry (random signs: the size the bar allows, in no particular direction), the largest
# change over a few draws is what a library inside its bar may move the scalar by, and the bound is 16 times that -- the project's
# margin over a measured error (clf_train_ref.GRAD_MARGIN).
PROPAGATION_DRAWS = 4


def _jitter(rng, x, eps, symmetric=False):
    sign = rng.choice([-1.0, 1.0], size=x.shape)
    if symmetric:
        sign = np.triu(sign) + np.triu(sign, 1).T
    return x + eps * np.abs(x).max() * sign


def frechet_bound(stats_a, stats_b, eps, seed=0):
    """(bound, measured): 16 x the largest change of ``frechet`` under eps-perturbed means and covariances of both sets"""
    (_, mu_a, cov_a), (_, mu_b, cov_b) = stats_a, stats_b
    base = frechet(mu_a, cov_a, mu_b, cov_b)
    rng = np.random.default_rng(seed)
    worst = max(abs(frechet(_jitter(rng, mu_a, eps), _jitter(rng, cov_a, eps, True), _jitter(rng, mu_b, eps),
                            _jitter(rng, cov_b, eps, True)) - base) for _ in range(PROPAGATION_DRAWS))
    return 16.0 * worst, worst


def mmd2_bound(X, Y, eps, seed=0):
    """(bound, measured): 16 x the largest change of the MMD^2 estimate under eps-perturbed kernel matrices"""
    kxx, kyy, kxy = poly3(X, X), poly3(Y, Y), poly3(X, Y)
    base = mmd2_from_kernels(kxx, kyy, kxy)
    rng = np.random.default_rng(seed)
    worst = max(abs(mmd2_from_kernels(_jitter(rng, kxx, eps, True), _jitter(rng, kyy, eps, True), _jitter(rng, kxy, eps)) - base)
                for _ in range(PROPAGATION_DRAWS))
    return 16.0 * worst, worst


def tight_feature_sets(n, m, d, seed=0, spread=0.1):
    """features with the common offset of 50 and a spread of 0.1 around it, as pooled features of similar images have: the
    inputs of the planted uncentred-distance error"""
    rng = np.random.default_rng(900 + seed)
    W = rng.standard_normal((5, d)) / np.sqrt(5)
    a = (OFFSET + spread * (rng.standard_normal((n, 5)) @ W)).astype(np.float32)
    b = (OFFSET + spread * (rng.standard_normal((m, 5)) @ W)).astype(np.float32)
    return a, b
