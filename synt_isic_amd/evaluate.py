"""Evaluation of a generated set against the real images: how close the two are, and whether the model copied its training data.

* ``extract_features``      -- the classifier's pooled 512-d features of uint8 or float images
* ``FeatureStats``          -- count, mean and covariance of a feature set; ``merge`` combines shards on the host
* ``frechet_distance``      -- the Frechet distance of two Gaussians fitted to the features (Heusel et al. 2017)
* ``kernel_distance``       -- the unbiased MMD^2 with the cubic polynomial kernel (Binkowski et al. 2018, "KID")
* ``precision_recall``      -- improved precision and recall (Kynkaanniemi et al. 2019)
* ``nearest_neighbours``    -- exact k nearest rows of one set in another
* ``memorisation_audit``    -- per generated image the nearest real image, in pixels and in features, with a calibrated copy ratio
* ``evaluate_generated``    -- all of it in one dict

The pairwise arithmetic -- Gram matrices, covariances, kernel matrices, neighbour search -- runs in libsisic_hip.so
(``ops.gram`` on the f32 matrix pipe, ``ops.col_means``, ``ops.rows_topk``, ``ops.pair_sqdist``, ``ops.matrix_sum``); what is left
on the host is O(d^3) linear algebra and bookkeeping in numpy float64, in pure functions that run without a GPU
(``frechet_distance``, ``FeatureStats.merge``, ``mmd2_unbiased``, ``subset_indices``, ``precision_recall_from_distances``).
Nothing here depends on scipy.

Which number to read.  The Frechet distance of two sample sets is biased upwards by a term that grows as the sets shrink, and
a covariance of 512 dimensions estimated from 500 images is rank-deficient: at the reference's <= 500 real images per class
its value says more about n than about the model.  The kernel distance is unbiased at any n, so at <= 500 real images it is the
number to compare settings by.  Neither is comparable with Inception-FID or KID figures from the literature: the features
are this project's ResNet18's, not Inception's.

Centring.  Every squared distance formed as ``|a|^2 + |b|^2 - 2 a.b`` loses the digits the three terms have in common, and
pooled ReLU features share a large positive mean: the library subtracts the real set's mean from both operands while it stages
them (``shift_a`` / ``shift_b`` of ``ops.gram``), which changes no distance and removes the common part.  Even so the Gram form
cannot resolve a distance much smaller than the norms -- exactly the case of a copied image -- so ``nearest_neighbours`` only
takes its candidates from it and ranks them by ``ops.pair_sqdist``, which subtracts first and sums in double.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

FEATURE_DIM = 512
DIST_BYTES_CAP = 256 << 20      # bytes of one distance matrix in nearest_neighbours: the rows of A are walked in chunks under it
MAX_K = 8                       # ops.rows_topk keeps at most 8 per row


# ---- host side: pure numpy float64 ------------------------------------------------------------------------------------------------
@dataclass
class FeatureStats:
    """Count, mean (float64 [d]) and covariance (float64 [d,d], divisor n - 1) of a feature set."""
    n: int
    mean: np.ndarray
    cov: np.ndarray

    @staticmethod
    def from_features(features) -> "FeatureStats":
        """Statistics of any [n,d] array (a torch tensor on the GPU, or anything ``numpy.asarray`` takes, which is uploaded):
        ``ops.col_means`` for the mean, ``ops.gram(contract_rows=True)`` centred on the fp32-rounded mean for the scatter matrix;
        the rounding of the mean is taken out again in float64 (sum (x-s)(x-s)^T = sum (x-mu)(x-mu)^T + n (mu-s)(mu-s)^T)."""
        import torch
        from . import ops
        F = _as_device_matrix(features)
        n, d = int(F.shape[0]), int(F.shape[1])
        if n < 2:
            raise ValueError(f"a covariance needs at least 2 rows, got {n}")
        mean_dev = ops.col_means(F)
        shift = mean_dev.to(torch.float32)
        scatter = ops.gram(F, shift_a=shift, contract_rows=True)
        mean = mean_dev.cpu().numpy()
        delta = mean - shift.cpu().numpy().astype(np.float64)
        s = scatter.cpu().numpy().astype(np.float64) - n * np.outer(delta, delta)
        return FeatureStats(n, mean, (s + s.T) / (2.0 * (n - 1)))

    @staticmethod
    def merge(a: "FeatureStats", b: "FeatureStats") -> "FeatureStats":
        """The statistics of the union of two disjoint sets from their statistics alone (Chan, Golub and LeVeque 1979), in float64:
        shards of a sharded generation combine without gathering features."""
        if a.mean.shape != b.mean.shape:
            raise ValueError(f"feature dimensions differ: {a.mean.shape} and {b.mean.shape}")
        n = a.n + b.n
        delta = np.asarray(b.mean, np.float64) - np.asarray(a.mean, np.float64)
        mean = a.mean + delta * (b.n / n)
        m2 = a.cov * (a.n - 1) + b.cov * (b.n - 1) + np.outer(delta, delta) * (a.n * b.n / n)
        return FeatureStats(n, mean, m2 / (n - 1))

    def state_dict(self) -> Dict[str, np.ndarray]:
        """arrays ``numpy.savez`` takes: the real set's statistics are computed once and kept"""
        return {"n": np.asarray(self.n, np.int64), "mean": np.asarray(self.mean, np.float64), "cov": np.asarray(self.cov, np.float64)}

    @staticmethod
    def from_state_dict(sd) -> "FeatureStats":
        mean, cov = np.asarray(sd["mean"], np.float64), np.asarray(sd["cov"], np.float64)
        if mean.ndim != 1 or cov.shape != (mean.shape[0], mean.shape[0]):
            raise ValueError(f"mean {mean.shape} and cov {cov.shape} do not belong together")
        return FeatureStats(int(sd["n"]), mean, cov)


def frechet_distance(a: FeatureStats, b: FeatureStats) -> float:
    """``|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 sum_i sqrt(max(l_i, 0))``, l the eigenvalues of ``S_a^(1/2) S_b S_a^(1/2)`` (which
    are those of ``S_a S_b``), from ``numpy.linalg.eigh`` twice: symmetric throughout, so it is defined and real when the
    covariances are rank-deficient (n < d, the normal case at 500 real images).  Biased upwards at small n: see the module text."""
    sa, sb = np.asarray(a.cov, np.float64), np.asarray(b.cov, np.float64)
    w, v = np.linalg.eigh((sa + sa.T) / 2)
    root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
    m = root @ ((sb + sb.T) / 2) @ root
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    diff = np.asarray(a.mean, np.float64) - np.asarray(b.mean, np.float64)
    return float(diff @ diff + np.trace(sa) + np.trace(sb) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def mmd2_unbiased(sum_xx_offdiag: float, sum_yy_offdiag: float, sum_xy: float, n: int, m: int) -> float:
    """The unbiased MMD^2 estimate from three kernel-matrix sums: k(x,x') over i != j, k(y,y') over i != j, k(x,y) over all."""
    if n < 2 or m < 2:
        raise ValueError(f"the unbiased estimate needs at least 2 samples per set, got {n} and {m}")
    return float(sum_xx_offdiag / (n * (n - 1.0)) + sum_yy_offdiag / (m * (m - 1.0)) - 2.0 * sum_xy / (float(n) * m))


def subset_indices(seed: int, n: int, m: int, subset_size: int, n_subsets: int):
    """The subsets ``kernel_distance`` draws: for each of ``n_subsets`` a pair of sorted index arrays of length ``subset_size``
    drawn without replacement from range(n) and range(m).  A pure function of its arguments (numpy's PCG64 seeded with ``seed``)."""
    if not 2 <= subset_size <= min(n, m):
        raise ValueError(f"subset_size {subset_size} must lie in [2, min(n, m) = {min(n, m)}]")
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    out = []
    for _ in range(int(n_subsets)):
        ia = np.sort(rng.choice(n, size=subset_size, replace=False))
        ib = np.sort(rng.choice(m, size=subset_size, replace=False))
        out.append((ia.astype(np.int64), ib.astype(np.int64)))
    return out


def precision_recall_from_distances(d_gg, d_rr, d_gr, k: int = 3) -> Tuple[float, float]:
    """Improved precision and recall from squared-distance matrices (generated x generated, real x real, generated x real).
    The radius of a point is the distance to its k-th nearest neighbour within its own set, itself excluded; precision is
    the share of generated points inside some real point's ball, recall the share of real points inside some generated ball."""
    d_gg, d_rr, d_gr = (np.asarray(x) for x in (d_gg, d_rr, d_gr))
    rad_g, rad_r = _kth_excluding_self(d_gg, k), _kth_excluding_self(d_rr, k)
    precision = float(((d_gr - rad_r[None, :]).min(axis=1) <= 0).mean())
    recall = float(((d_gr.T - rad_g[None, :]).min(axis=1) <= 0).mean())
    return precision, recall


def _kth_excluding_self(d: np.ndarray, k: int) -> np.ndarray:
    n = d.shape[0]
    if d.shape != (n, n) or not 1 <= k <= n - 1:
        raise ValueError(f"a [n,n] matrix with 1 <= k <= n - 1 is needed, got {d.shape} and k = {k}")
    off = d[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    return np.partition(off, k - 1, axis=1)[:, k - 1]


# ---- device side ------------------------------------------------------------------------------------------------------------------
def _as_device_matrix(x, device=None):
    """fp32 [n,d] on the GPU: a torch tensor there as it is (rows may be strided), anything else uploaded"""
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    if x.dim() != 2:
        raise ValueError(f"features must be [n,d], got {tuple(x.shape)}")
    if not x.is_cuda:
        x = x.to(device if device is not None else "cuda")
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


def _images_of(images):
    """the tensor or array behind a DeviceDataset, a SampleResult or a bare array"""
    return getattr(images, "images", images)


def _u8_rows(images, device):
    """uint8 [N,H,W,3] images as fp32 rows [N, H*W*3] of their byte values on ``device``"""
    import torch
    t = _images_of(images)
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"images must be uint8 [N,H,W,3], got {t.dtype} {tuple(t.shape)}")
    return t.to(device).reshape(t.shape[0], -1).to(torch.float32)


def extract_features(clf, images, batch: Optional[int] = None):
    """fp32 [N,512] on the classifier's device: ``clf.features`` of uint8 [N,H,W,3] images (a ``DeviceDataset``, its ``.images``,
    ``SampleResult.images`` or numpy; scaled to [-1,1] as the samplers' latents are) or of float [N,3,H,W] in [-1,1].  ``batch``
    images are converted and run at a time (default ``clf.max_forward_batch``)."""
    import torch
    from . import ops
    t = _images_of(images)
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dim() != 4:
        raise ValueError(f"images must be uint8 [N,H,W,3] or float [N,3,H,W], got {tuple(t.shape)}")
    u8 = t.dtype == torch.uint8
    if u8 and t.shape[3] != 3 or not u8 and (t.shape[1] != 3 or not t.dtype.is_floating_point):
        raise ValueError(f"images must be uint8 [N,H,W,3] or float [N,3,H,W], got {t.dtype} {tuple(t.shape)}")
    step = int(batch) if batch else int(clf.max_forward_batch)
    dev = clf.device
    out = ops.empty((t.shape[0], FEATURE_DIM), dtype=torch.float32, device=dev)
    for lo in range(0, t.shape[0], step):
        x = t[lo:lo + step].to(dev)
        if u8:
            x = x.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0
        out[lo:lo + step].copy_(clf.features(x))
    return out


def kernel_distance(Fa, Fb, subset_size: Optional[int] = None, n_subsets: int = 100, seed: int = 0):
    """The kernel distance of two feature sets: the unbiased MMD^2 estimate with k(x,y) = (x.y / d + 1)^3, the three kernel
    matrices from ``ops.gram(mode='poly3')`` and their sums from ``ops.matrix_sum``.  Returns ``(mean, std)`` over ``n_subsets``
    subsets of ``subset_size`` rows of each set (``subset_indices(seed, ...)``); ``subset_size=None``: the single estimate over the
    full sets, std None.  Unbiased at any n: at <= 500 real images this is the number to read, not the Frechet distance."""
    import torch
    from . import ops
    A = _as_device_matrix(Fa)
    B = _as_device_matrix(Fb, A.device)
    n, m = int(A.shape[0]), int(B.shape[0])

    def sums(a, b):
        return torch.cat([ops.matrix_sum(ops.gram(a, mode="poly3"), exclude_diagonal=True),
                          ops.matrix_sum(ops.gram(b, mode="poly3"), exclude_diagonal=True),
                          ops.matrix_sum(ops.gram(a, b, mode="poly3"))])

    if subset_size is None:
        s = sums(A, B).cpu().numpy()
        return mmd2_unbiased(s[0], s[1], s[2], n, m), None
    rows = []
    for ia, ib in subset_indices(seed, n, m, int(subset_size), n_subsets):
        rows.append(sums(A[torch.from_numpy(ia).to(A.device)], B[torch.from_numpy(ib).to(A.device)]))
    s = torch.stack(rows).cpu().numpy()
    est = np.array([mmd2_unbiased(r[0], r[1], r[2], int(subset_size), int(subset_size)) for r in s])
    return float(est.mean()), float(est.std())


def precision_recall(Fa_generated, Fb_real, k: int = 3) -> Tuple[float, float]:
    """Improved precision and recall of the generated features against the real ones.  Each set's radii are its own k-th
    neighbour distances (``ops.gram(mode='sqdist')`` within the set, ``ops.rows_topk(skip_diagonal=True)``); a point lies in
    the other set's manifold when ``min_j (D[i,j] - radius_j^2) <= 0`` (``ops.rows_topk(col_offset=radii^2, k=1)``).  All
    distances are formed after centring both sets on the real set's mean."""
    import torch
    from . import ops
    G = _as_device_matrix(Fa_generated)
    R = _as_device_matrix(Fb_real, G.device)
    if not 1 <= k <= MAX_K or k > min(G.shape[0], R.shape[0]) - 1:
        raise ValueError(f"k = {k} must lie in [1, {MAX_K}] and below both set sizes ({G.shape[0]}, {R.shape[0]})")
    shift = ops.col_means(R).to(torch.float32)
    rad_g = ops.rows_topk(ops.gram(G, mode="sqdist", shift_a=shift, shift_b=shift), k, skip_diagonal=True)[0][:, k - 1].contiguous()
    rad_r = ops.rows_topk(ops.gram(R, mode="sqdist", shift_a=shift, shift_b=shift), k, skip_diagonal=True)[0][:, k - 1].contiguous()
    in_real = ops.rows_topk(ops.gram(G, R, mode="sqdist", shift_a=shift, shift_b=shift), 1, col_offset=rad_r)[0]
    in_gen = ops.rows_topk(ops.gram(R, G, mode="sqdist", shift_a=shift, shift_b=shift), 1, col_offset=rad_g)[0]
    inside = torch.stack([(in_real <= 0).sum(), (in_gen <= 0).sum()]).cpu().numpy()        # counts: the shares are formed on the host
    return int(inside[0]) / int(G.shape[0]), int(inside[1]) / int(R.shape[0])


def nearest_neighbours(A, B, k: int = 1, candidates: Optional[int] = None, exclude_self: bool = False):
    """The ``k`` nearest rows of ``B`` for every row of ``A``: ``(sqdist fp32 [n,k], index int32 [n,k])``, ascending, ties to the
    lower index.  ``candidates`` (default ``min(8, k + 4)``) per row come from the Gram-form distances
    (``ops.gram(mode='sqdist')`` on operands centred on B's mean, ``ops.rows_topk``); ``ops.pair_sqdist`` then gives their exact
    distances and the best ``k`` are kept -- the Gram form loses its digits exactly where a copy would sit.  The rows of A are
    walked in chunks so that one distance matrix stays under ``DIST_BYTES_CAP`` bytes.  ``exclude_self``: A is B and row i is not
    its own neighbour (one chunk: the matrix must fit under the cap)."""
    import torch
    from . import ops
    A = _as_device_matrix(A)
    B = A if exclude_self else _as_device_matrix(B, A.device)
    n, m = int(A.shape[0]), int(B.shape[0])
    avail = m - (1 if exclude_self else 0)
    if not 1 <= k <= MAX_K or k > avail:
        raise ValueError(f"k = {k} must lie in [1, {MAX_K}] and not above the {avail} candidates rows")
    cand = min(MAX_K, k + 4) if candidates is None else int(candidates)
    cand = min(cand, avail)
    if cand < k:
        raise ValueError(f"candidates = {cand} below k = {k}")
    rows = max(1, DIST_BYTES_CAP // (4 * m))
    if exclude_self and rows < n:
        raise ValueError(f"exclude_self needs the whole [{n},{n}] distance matrix under {DIST_BYTES_CAP} bytes")
    shift = ops.col_means(B).to(torch.float32)
    dist = ops.empty((n, k), dtype=torch.float32, device=A.device)
    index = ops.empty((n, k), dtype=torch.int32, device=A.device)
    for lo in range(0, n, rows):
        a = A[lo:lo + rows]
        _, idx = ops.rows_topk(ops.gram(a, B, mode="sqdist", shift_a=shift, shift_b=shift), cand, skip_diagonal=exclude_self)
        exact = ops.pair_sqdist(a, B, idx)
        # rank the candidates by (exact distance, index): order by index first, then a stable sort by distance
        by_idx = torch.sort(idx, dim=1, stable=True)
        order = torch.sort(torch.gather(exact, 1, by_idx.indices), dim=1, stable=True)
        dist[lo:lo + rows].copy_(order.values[:, :k])
        index[lo:lo + rows].copy_(torch.gather(by_idx.values, 1, order.indices)[:, :k])
    return dist, index


@dataclass
class NeighbourReport:
    """One space's (pixels or features) nearest real rows of every generated row; arrays on the host.
    ``ratio[i] = distance[i,0] / real_gap[index[i,0]]``: the distance to the nearest real row over that real row's own distance
    to its nearest other real row -- near or above 1 for a sample as far from the data as the data is from itself, near 0 for
    a copy."""
    sqdist: np.ndarray        # float32 [n,k]
    index: np.ndarray         # int32 [n,k]
    distance: np.ndarray      # float64 [n,k], sqrt(sqdist)
    rms: np.ndarray           # float64 [n,k], sqrt(sqdist / d): per coordinate (pixels: per channel value, in grey levels)
    real_gap: np.ndarray      # float64 [m], every real row's distance to its nearest other real row
    ratio: np.ndarray         # float64 [n]

    def indices_below(self, threshold: float) -> np.ndarray:
        """generated rows whose ratio is below ``threshold`` (the function reports; the bar is the caller's)"""
        return np.nonzero(self.ratio < threshold)[0]


@dataclass
class AuditResult:
    pixels: NeighbourReport
    features: Optional[NeighbourReport]

    def indices_below(self, threshold: float, space: str = "pixels") -> np.ndarray:
        rep = self.pixels if space == "pixels" else self.features
        if rep is None:
            raise ValueError("the audit ran without a classifier: there is no feature-space report")
        return rep.indices_below(threshold)


def _neighbour_report(G, R, k: int) -> NeighbourReport:
    d2, idx = nearest_neighbours(G, R, k)
    gap2, _ = nearest_neighbours(R, R, 1, exclude_self=True)
    d2, idx, gap2 = d2.cpu().numpy(), idx.cpu().numpy(), gap2.cpu().numpy()
    distance = np.sqrt(d2.astype(np.float64))
    real_gap = np.sqrt(gap2[:, 0].astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = distance[:, 0] / real_gap[idx[:, 0]]
    return NeighbourReport(d2, idx, distance, np.sqrt(d2.astype(np.float64) / G.shape[1]), real_gap, ratio)


def memorisation_audit(generated_u8, real_u8, clf=None, k: int = 1, device=None,
                       features: Optional[tuple] = None) -> AuditResult:
    """Per generated image its ``k`` nearest real images in pixel space (distance over the uint8 values as floats, also as RMS
    per channel value) and, given ``clf``, in the classifier's feature space, each with the calibrated copy ratio of
    ``NeighbourReport``.  ``features``: (generated, real) feature matrices already extracted.  The function reports -- it sets
    no pass or fail bar: ``result.indices_below(threshold)`` lists the rows under a bar of the caller's choosing."""
    import torch
    if device is None:
        g = _images_of(generated_u8)
        device = clf.device if clf is not None else (g.device if isinstance(g, torch.Tensor) and g.is_cuda else "cuda")
    G, R = _u8_rows(generated_u8, device), _u8_rows(real_u8, device)
    if G.shape[1] != R.shape[1]:
        raise ValueError(f"generated and real images differ in size: {G.shape[1]} and {R.shape[1]} values per image")
    pixels = _neighbour_report(G, R, k)
    feats = None
    if features is None and clf is not None:
        features = (extract_features(clf, generated_u8), extract_features(clf, real_u8))
    if features is not None:
        feats = _neighbour_report(_as_device_matrix(features[0]), _as_device_matrix(features[1]), k)
    return AuditResult(pixels, feats)


def evaluate_generated(clf, generated, real, k: int = 3, kid_subset: Optional[int] = None, seed: int = 0) -> dict:
    """Everything above for uint8 image sets ``generated`` and ``real``: ``n_generated``, ``n_real``, ``feature_dim``,
    ``frechet_distance``, ``kernel_distance`` and ``kernel_distance_std`` (None without ``kid_subset``), ``precision``, ``recall``,
    ``stats_generated`` / ``stats_real`` (``FeatureStats``) and ``audit`` (``AuditResult``) with its headline numbers
    ``pixel_ratio_min``, ``pixel_rms_min``, ``feature_ratio_min``."""
    Fg, Fr = extract_features(clf, generated), extract_features(clf, real)
    sg, sr = FeatureStats.from_features(Fg), FeatureStats.from_features(Fr)
    kid, kid_std = kernel_distance(Fg, Fr, subset_size=kid_subset, seed=seed)
    precision, recall = precision_recall(Fg, Fr, k=k)
    audit = memorisation_audit(generated, real, clf=clf, k=1, features=(Fg, Fr))
    return {"n_generated": sg.n, "n_real": sr.n, "feature_dim": int(Fg.shape[1]),
            "frechet_distance": frechet_distance(sg, sr), "kernel_distance": kid, "kernel_distance_std": kid_std,
            "precision": precision, "recall": recall, "k": int(k), "stats_generated": sg, "stats_real": sr, "audit": audit,
            "pixel_ratio_min": float(np.min(audit.pixels.ratio)), "pixel_rms_min": float(np.min(audit.pixels.rms[:, 0])),
            "feature_ratio_min": float(np.min(audit.features.ratio))}
