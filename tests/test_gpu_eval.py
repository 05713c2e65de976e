"""The evaluation metrics on the GPU against tests/eval_ref.py: the pooled features, the five pairwise entry points one by one,
then FeatureStats, the Frechet and kernel distances, precision / recall, nearest neighbours, the memorisation audit and
evaluate_generated on top of them, and every entry point on a held side stream.

Bounds.  Matrices (Gram, distance, kernel, covariance, mean) are held to clf_train_ref's ``bar``: max|x - x64| / max|x64| <=
max(1e-5, 16 e32), e32 the error of fp32 torch computing the same formula on the same fp32 inputs.  Scalars computed FROM such
matrices (the Frechet distance, the kernel distance) are held to a bound propagated from that bar (eval_ref.frechet_bound /
mmd2_bound): the restatement is evaluated on inputs perturbed by +-bar * max|x| in every entry, the largest change over four
draws is what a library inside its bar may move the scalar by, and the bound is 16 times that.  Measured on the two input sets
(generated, real, d) = (300, 200, 64) and (120, 90, 512); eps is the bar of the matrices the scalar is computed from, 1.0e-05
for the statistics and 2.5e-05 / 2.3e-05 for the kernel matrices (16 x fp32 torch's 1.6e-06 / 1.4e-06):
    Frechet distance   value 2.67e+01 / 2.61e+02, change under perturbation 4.6e-03 / 2.1e-01  -> bounds 7.4e-02 / 3.4e+00;
                       the library is 3.5e-07 / 1.8e-03 from the restatement
    kernel distance    value 6.76e+06 / 7.29e+06, change under perturbation 7.1e+03 / 1.5e+04  -> bounds 1.1e+05 / 2.4e+05;
                       the library is 1.1e+02 / 2.1e+02 from the restatement
(the kernel values themselves are (50^2 + 1)^3 = 1.6e+10 on features with a common mean of 50: the distance is a difference of
means of such numbers).  Exact quantities -- neighbour indices, precision and recall, rows_topk -- are compared with ==; their
inputs are chosen so that the float64 reference is well conditioned (eval_ref, asserted in test_eval_cpu.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_ref as er
import stream_probe as sp
from poison import guard_bands, poison_allocations  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
CLF_TOL = 2e-4            # tests/test_gpu_classifier.py: logits against the float64 oracle


def _close(got, ref, tol, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    bound = tol * max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert got.shape == ref.shape and err <= bound, f"{what}: err {err:.3e} > {bound:.3e} (shape {tuple(got.shape)})"


def _inside_bar(got, ref64, ref32, what):
    e32 = er.rel_err(ref32, ref64)
    err = er.rel_err(got, ref64)
    print(f"{what}: rel err {err:.3e}, fp32 torch {e32:.3e}, bar {er.bar(e32):.3e}")
    assert tuple(got.shape) == tuple(ref64.shape) and err <= er.bar(e32), f"{what}: {err:.3e} > {er.bar(e32):.3e}"


def _dev(x):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(DEV)


# ---- 1. pooled features ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feat_sd():
    """a 512-class head that is the identity: the logits ARE the pooled features"""
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    sd = synthetic_resnet18_state_dict(num_classes=512)
    sd["model.fc.weight"] = torch.eye(512)
    sd["model.fc.bias"] = torch.zeros(512)
    return sd


@pytest.fixture(scope="module")
def feat_clf(feat_sd):
    from synt_isic_amd.classifier import HipMelanomaClassifier
    m = HipMelanomaClassifier(num_classes=512, pretrained=False)
    m.load_state_dict(dict(feat_sd))
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def clf():
    from synt_isic_amd.classifier import HipMelanomaClassifier
    from synt_isic_amd.weights import synthetic_resnet18_state_dict
    m = HipMelanomaClassifier(num_classes=7, pretrained=False)
    m.load_state_dict(dict(synthetic_resnet18_state_dict()))
    return m.to(DEV).eval()


def _x(B, H, W, seed):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 0.8


@pytest.mark.parametrize("B,H,W", [(3, 32, 32), (2, 64, 64)])
def test_features_are_the_identity_heads_logits(feat_clf, feat_sd, B, H, W):
    from oracle import resnet18 as ores
    x = _x(B, H, W, 40 + H)
    got = feat_clf.features(x)
    assert got.shape == (B, 512) and got.dtype == torch.float32 and got.device.type == "cuda"
    _close(got, feat_clf.forward(x), CLF_TOL, "features vs the identity head's logits")
    _close(got, ores.resnet18_features(feat_sd, ores.preprocess_for_classifier(x)), CLF_TOL, "features vs the oracle")
    pre = ores.preprocess_for_classifier(x)
    _close(feat_clf.features(pre, preprocessed=True), ores.resnet18_features(feat_sd, pre), CLF_TOL, "preprocessed input")


def test_feature_rows_do_not_depend_on_the_chunking(feat_clf, monkeypatch):
    x = _x(5, 32, 32, 41)
    whole = feat_clf.features(x)
    monkeypatch.setattr(feat_clf, "max_forward_batch", 2)
    assert torch.equal(feat_clf.features(x), whole)
    assert torch.equal(feat_clf.features(x[3:4]), whole[3:4])


# ---- 2. ops.gram ---------------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 1, 1), (33, 65, 7), (128, 128, 512), (130, 257, 515), (64, 500, 12288)]


@pytest.mark.parametrize("n,m,d", GRAM_SHAPES)
def test_gram_three_modes_with_and_without_shifts(n, m, d):
    from synt_isic_amd import ops
    A, B, sa, sb = er.gram_inputs(n, m, d, 100 + n)
    dA, dB, dsa, dsb = _dev(A), _dev(B), _dev(sa), _dev(sb)
    for mode in ("dot", "sqdist", "poly3"):
        for shifted in (False, True):
            kw = dict(shift_a=sa, shift_b=sb) if shifted else {}
            got = ops.gram(dA, dB, mode=mode, shift_a=dsa if shifted else None, shift_b=dsb if shifted else None)
            _inside_bar(got, er.gram(A, B, mode, **kw), er.gram(A, B, mode, dtype=torch.float32, **kw),
                        f"gram {mode} {n}x{m}x{d} shifted={shifted}")
            assert torch.equal(ops.gram(dA, dB, mode=mode, shift_a=dsa if shifted else None, shift_b=dsb if shifted else None), got)
    # b omitted: the set against itself, shift_b still B's own
    _inside_bar(ops.gram(dA, mode="sqdist", shift_a=dsa, shift_b=dsa), er.gram(A, None, "sqdist", sa, sa),
                er.gram(A, None, "sqdist", sa, sa, dtype=torch.float32), f"gram sqdist {n}x{n}x{d} on itself")


@pytest.mark.parametrize("n,d", [(37, 5), (300, 64), (130, 515)])
def test_gram_contract_rows(n, d):
    from synt_isic_amd import ops
    A = torch.randn(n, d, generator=torch.Generator().manual_seed(200 + n)) + 3.0
    for shift in (None, A.double().mean(0).float()):
        got = ops.gram(_dev(A), shift_a=None if shift is None else _dev(shift), contract_rows=True)
        _inside_bar(got, er.gram(A, None, "dot", shift, contract_rows=True),
                    er.gram(A, None, "dot", shift, dtype=torch.float32, contract_rows=True), f"gram contract_rows {n}x{d}")
        assert torch.equal(ops.gram(_dev(A), shift_a=None if shift is None else _dev(shift), contract_rows=True), got)


def test_gram_leading_dimensions_and_refusals():
    from synt_isic_amd import _lib, ops
    A, B, sa, sb = er.gram_inputs(70, 45, 19, 300)
    wide_a, wide_b = torch.full((70, 32), float("nan")), torch.full((45, 27), float("nan"))
    wide_a[:, 3:22], wide_b[:, :19] = A, B
    da, db = _dev(wide_a)[:, 3:22], _dev(wide_b)[:, :19]            # rows 32 and 27 floats apart, the first not 16-byte aligned
    assert da.stride(0) == 32 and db.stride(0) == 27
    for mode in ("dot", "sqdist", "poly3"):
        got = ops.gram(da, db, mode=mode, shift_a=_dev(sa), shift_b=_dev(sb))
        assert torch.equal(got, ops.gram(_dev(A), _dev(B), mode=mode, shift_a=_dev(sa), shift_b=_dev(sb))), mode
    assert torch.equal(ops.gram(da, shift_a=_dev(sa), contract_rows=True), ops.gram(_dev(A), shift_a=_dev(sa), contract_rows=True))
    # the C entry refuses what the wrapper cannot express
    out = torch.zeros(4, 4, device=DEV)
    x = torch.zeros(4, 4, device=DEV)

    def rc(**kw):
        f = dict(a=x.data_ptr(), out=out.data_ptr(), lda=4, ldb=4, ldo=4, n=4, m=4, d=4, mode=0,
                 stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
        f.update(kw)
        return _lib.load().sisic_gram(ops.context(x.device), C.byref(_lib.GramArgs(**f))), _lib.load().sisic_last_error()

    assert rc()[0] == _lib.SISIC_OK
    for kw, needle in ((dict(mode=3), b"mode"), (dict(lda=3), b"lda"), (dict(ldo=3), b"ldo"), (dict(n=0), b"n 0"),
                       (dict(contract_rows=1, b=x.data_ptr()), b"contract_rows"), (dict(contract_rows=1, mode=1), b"contract_rows")):
        code, msg = rc(**kw)
        assert code == _lib.SISIC_EINVAL and needle in msg, (kw, code, msg)
    with pytest.raises(ValueError):
        ops.gram(x, mode="cosine")


# ---- 3. ops.rows_topk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [9, 1000])
def test_rows_topk_is_the_stable_argsort(m):
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(400 + m)
    n = 9 if m == 9 else 70
    D = (torch.randn(n, m, generator=g) * 3).round()                 # integers in about [-9, 9]: every row repeats values
    D[0] = 2.0                                                       # a constant row: the columns come back in order
    off = torch.randint(-2, 3, (m,), generator=g).float()
    for k in (1, 3, 8):
        for use_off in (False, True):
            for skip in (False, True):
                val, idx = ops.rows_topk(_dev(D), k, col_offset=_dev(off) if use_off else None, skip_diagonal=skip)
                rv, ri = er.rows_topk(D.numpy(), k, off.numpy() if use_off else None, skip)
                assert val.shape == (n, k) and idx.dtype == torch.int32
                assert torch.equal(idx.cpu(), torch.from_numpy(ri)), (m, k, use_off, skip)
                assert torch.equal(val.cpu(), torch.from_numpy(rv)), (m, k, use_off, skip)
    wide = _dev(torch.cat([D, torch.full((n, 5), -100.0)], 1))[:, :m]       # ld > m: what lies behind the row is not read
    assert torch.equal(ops.rows_topk(wide, 3)[1].cpu(), torch.from_numpy(er.rows_topk(D.numpy(), 3)[1]))


def test_rows_topk_refusals():
    from synt_isic_amd import _lib, ops
    D = torch.zeros(9, 9, device=DEV)
    for m, k, skip in ((9, 9, False), (9, 0, False), (7, 8, False), (8, 8, True)):       # k > 8, k < 1, k > m, k > m - skip_diagonal
        with pytest.raises(_lib.SisicError) as e:
            ops.rows_topk(D[:, :m], k, skip_diagonal=skip)
        assert e.value.code == _lib.SISIC_EINVAL and f"k = {k}" in str(e.value) and f"m = {m}" in str(e.value), str(e.value)
    val, idx = ops.rows_topk(D[:, :8], 7, skip_diagonal=True)       # k = m - skip_diagonal is the most that is there
    assert torch.equal(idx[0].cpu(), torch.arange(1, 8, dtype=torch.int32))


# ---- 4. ops.pair_sqdist ------------------------------------------------------------------------------------------------------------------
def _ulps(got, want64):
    """distance of fp32 ``got`` from the float64 value rounded to fp32, in units of that fp32's spacing"""
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))


@pytest.mark.parametrize("d", [7, 512, 12288])
def test_pair_sqdist_is_float64_rounded_once(d):
    from synt_isic_amd import ops
    g = torch.Generator().manual_seed(500 + d)
    A, B = torch.randn(21, d, generator=g) + 50.0, torch.randn(33, d, generator=g) + 50.0
    A[4] = B[9]                                                     # identical rows: exactly 0
    idx = torch.randint(0, 33, (21, 5), generator=g).to(torch.int32)
    idx[4, 2] = 9
    got = ops.pair_sqdist(_dev(A), _dev(B), _dev(idx)).cpu().numpy()
    want = er.pair_sqdist(A.numpy(), B.numpy(), idx.numpy())
    assert got.shape == (21, 5) and got[4, 2] == 0.0
    assert _ulps(got, want).max() <= 1.0, _ulps(got, want).max()     # 1 ulp for the order of the double sum
    assert np.array_equal(ops.pair_sqdist(_dev(A), _dev(B), _dev(idx)).cpu().numpy(), got)
    bad = idx.clone()
    bad[0, 0], bad[1, 1] = 33, -1                                    # outside B: NaN, nothing read
    out = ops.pair_sqdist(_dev(A), _dev(B), _dev(bad)).cpu().numpy()
    assert np.isnan(out[0, 0]) and np.isnan(out[1, 1]) and np.array_equal(out[2:], got[2:])


# ---- 5. ops.col_means, ops.matrix_sum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 5), (300, 77), (1000, 512)])
def test_col_means(n, d):
    from synt_isic_amd import ops
    X = torch.randn(n, d, generator=torch.Generator().manual_seed(600 + n)) + 50.0
    got = ops.col_means(_dev(X))
    want = X.double().mean(0)
    assert got.dtype == torch.float64 and got.shape == (d,)
    assert ((got.cpu() - want).abs() / want.abs()).max().item() <= 1e-12
    assert torch.equal(ops.col_means(_dev(X)), got)
    wide = _dev(torch.cat([X, torch.full((n, 3), float("nan"))], 1))[:, :d]
    assert torch.equal(ops.col_means(wide), got)


@pytest.mark.parametrize("n,m", [(1, 1), (1, 40), (100, 333), (333, 100), (1100, 1100)])
def test_matrix_sum(n, m):
    from synt_isic_amd import ops
    M = torch.randn(n, m, generator=torch.Generator().manual_seed(700 + n + m)) + 2.0
    full = M.double().sum()
    for excl, want in ((False, full), (True, full - M.double().diagonal().sum())):       # the diagonal of a non-square matrix too
        got = ops.matrix_sum(_dev(M), exclude_diagonal=excl)
        assert got.dtype == torch.float64 and got.shape == (1,)
        scale = M.double().abs().sum().item()
        assert abs(got.item() - want.item()) <= 1e-12 * scale, (n, m, excl)
        assert torch.equal(ops.matrix_sum(_dev(M), exclude_diagonal=excl), got)
    wide = _dev(torch.cat([M, torch.full((n, 3), float("nan"))], 1))[:, :m]
    assert torch.equal(ops.matrix_sum(wide), ops.matrix_sum(_dev(M)))


# ---- 6. statistics and the three distances -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=er.PR_CASES, ids=lambda c: "x".join(map(str, c)))
def sets(request):
    gen, real, _ = er.feature_sets(*request.param)
    return gen, real, er.feature_stats(gen), er.feature_stats(real)


def _bar_of_stats(F, stats64):
    """bar(e32) of the mean and of the covariance: fp32 torch computing both on the same inputs (centred before the product)"""
    _, mu, cov = stats64
    f = torch.from_numpy(F)
    mu32 = f.mean(0)
    c = f - mu32
    return er.bar(er.rel_err(mu32, torch.from_numpy(mu))), er.bar(er.rel_err(c.T @ c / (F.shape[0] - 1), torch.from_numpy(cov)))


def test_feature_stats_inside_bar(sets):
    from synt_isic_amd import evaluate as ev
    for F, ref in ((sets[0], sets[2]), (sets[1], sets[3])):
        got = ev.FeatureStats.from_features(_dev(F))
        bar_mu, bar_cov = _bar_of_stats(F, ref)
        e_mu = er.rel_err(torch.from_numpy(got.mean), torch.from_numpy(ref[1]))
        e_cov = er.rel_err(torch.from_numpy(got.cov), torch.from_numpy(ref[2]))
        print(f"stats {F.shape}: mean {e_mu:.3e} (bar {bar_mu:.3e}), covariance {e_cov:.3e} (bar {bar_cov:.3e})")
        assert got.n == ref[0] and got.mean.dtype == np.float64 and got.cov.shape == ref[2].shape
        assert e_mu <= bar_mu and e_cov <= bar_cov
        assert np.array_equal(got.cov, got.cov.T)
    # numpy in, the same statistics out; two shards merged on the host are the whole
    F = sets[0]
    whole = ev.FeatureStats.from_features(F)
    parts = ev.FeatureStats.merge(ev.FeatureStats.from_features(F[:101]), ev.FeatureStats.from_features(F[101:]))
    assert parts.n == whole.n and er.rel_err(torch.from_numpy(parts.cov), torch.from_numpy(whole.cov)) <= 2 * _bar_of_stats(F, sets[2])[1]


def test_frechet_distance_inside_the_propagated_bound(sets):
    from synt_isic_amd import evaluate as ev
    gen, real, sg, sr = sets
    eps = max(max(_bar_of_stats(gen, sg)), max(_bar_of_stats(real, sr)))
    bound, measured = er.frechet_bound(sg, sr, eps)
    want = er.frechet(sg[1], sg[2], sr[1], sr[2])
    got = ev.frechet_distance(ev.FeatureStats.from_features(_dev(gen)), ev.FeatureStats.from_features(_dev(real)))
    print(f"frechet {gen.shape}: {got:.9e} vs {want:.9e}, |diff| {abs(got - want):.3e}; eps {eps:.2e}, restatement moves "
          f"{measured:.3e} under perturbation, bound {bound:.3e}")
    assert np.isfinite(got) and abs(got - want) <= bound


def test_kernel_distance_inside_the_propagated_bound(sets):
    from synt_isic_amd import evaluate as ev
    gen, real, _, _ = sets
    kxy = er.poly3(gen, real)
    eps = er.bar(er.rel_err(er.gram(gen, real, "poly3", dtype=torch.float32), torch.from_numpy(kxy)))
    bound, measured = er.mmd2_bound(gen, real, eps)
    want = er.mmd2(gen, real)
    got, std = ev.kernel_distance(_dev(gen), _dev(real))
    print(f"kernel distance {gen.shape}: {got:.9e} vs {want:.9e}, |diff| {abs(got - want):.3e}; eps {eps:.2e}, restatement moves "
          f"{measured:.3e} under perturbation, bound {bound:.3e}")
    assert std is None and abs(got - want) <= bound
    # subsets: the mean and std over the seeded draws, each estimate inside its own bound
    size, count = 60, 4
    draws = ev.subset_indices(3, len(gen), len(real), size, count)
    each = np.array([er.mmd2(gen[ia], real[ib]) for ia, ib in draws])
    worst = max(er.mmd2_bound(gen[ia], real[ib], eps)[0] for ia, ib in draws)
    mean, std = ev.kernel_distance(_dev(gen), _dev(real), subset_size=size, n_subsets=count, seed=3)
    assert abs(mean - each.mean()) <= worst and abs(std - each.std()) <= 2 * worst
    assert (mean, std) == ev.kernel_distance(_dev(gen), _dev(real), subset_size=size, n_subsets=count, seed=3)


def test_precision_recall_equal_the_restatement(sets):
    from synt_isic_amd import evaluate as ev
    gen, real, _, _ = sets
    want = er.precision_recall(gen, real, 3)
    got = ev.precision_recall(_dev(gen), _dev(real), k=3)
    print(f"precision / recall {gen.shape}: {got} vs {want}")
    assert got == want and 0 < got[0] < 1 and 0 < got[1] < 1


# ---- 7. nearest neighbours -----------------------------------------------------------------------------------------------------------------
def _neighbours_equal(got_d, got_i, A, B, k, exclude_self=False):
    want_d, want_i = er.knn(A, B, k, exclude_self)
    assert np.array_equal(got_i.cpu().numpy(), want_i)
    assert _ulps(got_d.cpu().numpy(), want_d).max() <= 1.0


def test_nearest_neighbours_feature_space(monkeypatch):
    from synt_isic_amd import evaluate as ev
    A, B = er.neighbour_sets(*er.NN_CASE, er.NN_CANDIDATES + 1)
    d, i = ev.nearest_neighbours(_dev(A), _dev(B), k=er.NN_K)
    assert d.shape == (200, er.NN_K) and i.dtype == torch.int32
    _neighbours_equal(d, i, A, B, er.NN_K)
    monkeypatch.setattr(ev, "DIST_BYTES_CAP", 4 * 150 * 64)          # 64 rows per chunk: three full chunks and a ragged one
    d2, i2 = ev.nearest_neighbours(_dev(A), _dev(B), k=er.NN_K)
    assert torch.equal(d2, d) and torch.equal(i2, i)


@pytest.mark.parametrize("planted", ["exact", "near"])
def test_nearest_neighbours_pixel_space_and_the_planted_copy(planted):
    from synt_isic_amd import evaluate as ev
    gen, real, _ = er.image_sets(planted=planted)
    G, R = gen.reshape(len(gen), -1).astype(np.float32), real.reshape(len(real), -1).astype(np.float32)
    d, i = ev.nearest_neighbours(_dev(G), _dev(R), k=2)
    _neighbours_equal(d, i, G, R, 2)
    d_self, i_self = ev.nearest_neighbours(_dev(R), _dev(R), k=1, exclude_self=True)
    _neighbours_equal(d_self, i_self, R, R, 1, exclude_self=True)
    audit = ev.memorisation_audit(gen, _dev(real))
    px = audit.pixels
    assert audit.features is None and px.index[er.PLANT_SLOT, 0] == er.PLANT_SRC
    others = np.delete(px.ratio, er.PLANT_SLOT)
    print(f"{planted} copy: ratio {px.ratio[er.PLANT_SLOT]:.3e}, rms {px.rms[er.PLANT_SLOT, 0]:.3e}; the others' ratios >= {others.min():.3f}")
    if planted == "exact":
        assert px.sqdist[er.PLANT_SLOT, 0] == 0.0 and px.ratio[er.PLANT_SLOT] == 0.0 and px.rms[er.PLANT_SLOT, 0] == 0.0
    else:
        assert 0 < px.rms[er.PLANT_SLOT, 0] <= 0.1 + 1e-6               # +-1 in 1 % of the bytes: sqrt(0.01) grey levels
        assert px.ratio[er.PLANT_SLOT] < 0.05 * others.min()
    threshold = 0.5 * others.min()                                   # between the two groups
    assert audit.indices_below(threshold).tolist() == [er.PLANT_SLOT]


# ---- 8. evaluate_generated -------------------------------------------------------------------------------------------------------------------
def test_evaluate_generated(clf):
    from synt_isic_amd import evaluate as ev
    from synt_isic_amd.data import DeviceDataset
    gen, real, _ = er.image_sets(planted="near")
    res = ev.evaluate_generated(clf, _dev(gen), DeviceDataset(real, DEV), k=3)
    assert res["n_generated"] == 24 and res["n_real"] == 16 and res["feature_dim"] == 512 and res["kernel_distance_std"] is None
    for key in ("frechet_distance", "kernel_distance", "precision", "recall", "pixel_ratio_min", "pixel_rms_min", "feature_ratio_min"):
        assert np.isfinite(res[key]), key
    assert 0 <= res["precision"] <= 1 and 0 <= res["recall"] <= 1
    assert res["stats_generated"].cov.shape == (512, 512) and np.isfinite(res["stats_real"].cov).all()
    audit = res["audit"]
    others = np.delete(audit.pixels.ratio, er.PLANT_SLOT)
    assert audit.indices_below(0.5 * others.min()).tolist() == [er.PLANT_SLOT]
    assert audit.features is not None and audit.features.index.shape == (24, 1) and np.isfinite(audit.features.ratio).all()
    assert audit.features.index[er.PLANT_SLOT, 0] == er.PLANT_SRC       # nearly the same image: nearly the same features
    # features of the uint8 images are the features of their [-1, 1] form
    F = ev.extract_features(clf, gen, batch=7)
    x = _dev(gen).permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0
    assert torch.equal(F, ev.extract_features(clf, x)) and torch.equal(F, clf.features(x))
    with_subsets = ev.evaluate_generated(clf, _dev(gen), _dev(real), k=3, kid_subset=10, seed=1)
    assert np.isfinite(with_subsets["kernel_distance"]) and with_subsets["kernel_distance_std"] >= 0


# ---- 9. a held side stream ---------------------------------------------------------------------------------------------------------------------
def _rand(shape, seed, offset=0.0):
    return _dev(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + offset)


def _stream_cases(feat_clf):
    from synt_isic_amd import ops
    idx = lambda seed: _dev(torch.randint(0, 40, (50, 4), generator=torch.Generator().manual_seed(seed)).to(torch.int32))  # noqa: E731
    return {
        "sisic_resnet_features": (lambda x: feat_clf.features(x), lambda s: [_rand((2, 3, 32, 32), s)]),
        "sisic_col_means": (ops.col_means, lambda s: [_rand((300, 70), s, 5.0)]),
        "sisic_gram": (lambda a, b, sh: (ops.gram(a, b, mode="sqdist", shift_a=sh, shift_b=sh), ops.gram(a, mode="poly3"),
                                         ops.gram(a, shift_a=sh, contract_rows=True)),
                       lambda s: [_rand((150, 70), s), _rand((130, 70), s + 1), _rand((70,), s + 2)]),
        "sisic_rows_topk": (lambda d, off: ops.rows_topk(d, 3, col_offset=off, skip_diagonal=True),
                            lambda s: [_rand((60, 200), s), _rand((200,), s + 1)]),
        "sisic_pair_sqdist": (ops.pair_sqdist, lambda s: [_rand((50, 300), s), _rand((40, 300), s + 1), idx(s + 2)]),
        "sisic_matrix_sum": (lambda m: (ops.matrix_sum(m), ops.matrix_sum(m, True)), lambda s: [_rand((200, 300), s)]),
    }


@pytest.mark.parametrize("entry", ["sisic_resnet_features", "sisic_col_means", "sisic_gram", "sisic_rows_topk", "sisic_pair_sqdist",
                                   "sisic_matrix_sum"])
def test_side_stream_gives_the_default_stream_bits(feat_clf, entry):
    fn, make = _stream_cases(feat_clf)[entry]
    baseline, held, until_return = sp.run_held(fn, lambda: make(10), lambda: make(20), entry)
    assert sp.same(baseline, held)
    assert until_return, f"{entry} waited for its stream"
