"""The training loader's host side, and its arithmetic contract, without a GPU: tests/augment_ref.py (the numpy restatement of
sisic_augment) against the PIL-generated fixture and against PIL itself, the parameter draws of synt_isic_amd.data, the colour
correction, the epoch permutations and the ISIC reader.  Equality with PIL is exact: integer resampling, float32 blends
truncated to uint8, a fixed-point nearest rotation -- there is no tolerance to choose."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

import augment_ref as R

SIZE_KEYS = ("16x16", "32x32", "24x40")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    with np.load(os.path.join(golden_dir, "augment.npz")) as z:
        return {k: z[k] for k in z.files}


def test_record_layout():
    from synt_isic_amd import _lib, ops, data
    assert ctypes.sizeof(_lib.AugmentParams) == 96
    assert ops.AUGMENT_DTYPE.itemsize == 96 and ops.AUGMENT_DTYPE == R.AUGMENT_DTYPE and data.AUGMENT_DTYPE is ops.AUGMENT_DTYPE
    for name, _ in _lib.AugmentParams._fields_:
        assert getattr(_lib.AugmentParams, name).offset == ops.AUGMENT_DTYPE.fields[name][1], name
    assert "sisic_augment" in _lib.SIGNATURES and "sisic_augment_u8" in _lib.SIGNATURES


def test_fixture_covers_the_groups(fixture):
    for key in SIZE_KEYS:
        H, W = (int(v) for v in key.split("x"))
        assert fixture["img_" + key].shape == (2, H, W, 3) and fixture["rec_" + key].dtype == R.AUGMENT_DTYPE
        groups, recs = fixture["group_" + key], fixture["rec_" + key]
        assert (groups == 0).sum() == 27 and (groups == 2).sum() == 8 and (groups == 1).sum() == (0 if key == "32x32" else 6)
        assert fixture["u8_" + key].shape == (len(recs), H, W, 3) and fixture["f32_" + key].shape == (8, 3, H, W)
        alone = recs[groups == 0]
        assert alone["rotate"].sum() == 7 and alone["hflip"].sum() == 2 and alone["vflip"].sum() == 2
        assert ((alone["crop_w"] < W) | (alone["crop_h"] < H)).sum() == 4
        assert ((alone["crop_w"] < W) & (alone["crop_h"] == H)).sum() == 1 and ((alone["crop_w"] == W) & (alone["crop_h"] < H)).sum() == 1
        if key != "32x32":
            assert sorted(tuple(o) for o in recs[groups == 1]["order"]) == sorted(itertools.permutations(range(3)))
        # a rotation by 15 degrees fills the corners with 0
        r15 = fixture["u8_" + key][np.nonzero((groups == 0) & (recs["rotate"] == 1))[0][0]]
        assert (r15[0, 0] == 0).all() and (r15[-1, -1] == 0).all()


@pytest.mark.parametrize("key", SIZE_KEYS)
def test_restatement_reproduces_fixture(fixture, key):
    imgs, recs, want = fixture["img_" + key], fixture["rec_" + key], fixture["u8_" + key]
    for i, rec in enumerate(recs):
        got = R.augment_u8(imgs, rec)
        assert np.array_equal(got, want[i]), f"{key} record {i} (group {fixture['group_' + key][i]}): {(got != want[i]).sum()} bytes differ"
        if rec["rotate"]:
            assert list(rec["rot"]) == R.rotation_fixed(float(fixture["angle_" + key][i]), *imgs.shape[1:3])
    full = want[fixture["group_" + key] == 2]
    assert np.array_equal(np.stack([R.normalize(u) for u in full]).view(np.uint32), fixture["f32_" + key].view(np.uint32))
    assert np.array_equal(fixture["norm_lut"][full].transpose(0, 3, 1, 2).view(np.uint32), fixture["f32_" + key].view(np.uint32))


@pytest.mark.parametrize("key", SIZE_KEYS)
def test_restatement_reproduces_pil(fixture, key):
    pytest.importorskip("PIL")
    imgs, recs = fixture["img_" + key], fixture["rec_" + key]
    for i, rec in enumerate(recs):
        pil = R.pil_augment(imgs, rec, float(fixture["angle_" + key][i]))
        assert np.array_equal(pil, fixture["u8_" + key][i]), f"{key} record {i}: the installed PIL differs from the fixture"
        assert np.array_equal(R.augment_u8(imgs, rec), pil)


def test_restatement_reproduces_pil_on_drawn_records():
    """records as draw_augment_params makes them (its own rotation matrices included), through PIL at 32x32 and 24x40"""
    pytest.importorskip("PIL")
    from synt_isic_amd import data
    rng = np.random.default_rng(7)
    for H, W in ((32, 32), (24, 40)):
        imgs = rng.integers(0, 256, size=(40, H, W, 3), dtype=np.uint8)
        recs = data.draw_augment_params(np.arange(40), 3, 11, H, W)
        u = np.stack([data._generator(11, 3, i).random(32) for i in range(40)])
        angles = -15.0 + 30.0 * u[:, 29]
        assert 0 < recs["rotate"].sum() < 40
        for rec, angle in zip(recs, angles):
            assert np.array_equal(R.augment_u8(imgs, rec), R.pil_augment(imgs, rec, angle))


# ---- parameter draws ----------------------------------------------------------------------------------------------------------
def test_draws_depend_on_seed_epoch_index_alone():
    from synt_isic_amd import data
    a = data.draw_augment_params(np.arange(16), 2, 5, 128, 128)
    b = np.concatenate([data.draw_augment_params([i], 2, 5, 128, 128) for i in reversed(range(16))])[::-1]
    assert a.tobytes() == b.tobytes()
    c = data.draw_augment_params([3, 9, 3], 2, 5, 128, 128)
    assert c[0] == a[3] and c[1] == a[9] and c[2] == a[3]
    other_epoch = data.draw_augment_params(np.arange(16), 3, 5, 128, 128)
    other_seed = data.draw_augment_params(np.arange(16), 2, 6, 128, 128)
    for other in (other_epoch, other_seed):
        assert (other["src"] == a["src"]).all()
        assert sum(x.tobytes() != y.tobytes() for x, y in zip(a, other)) == 16


def test_draws_are_valid_and_follow_the_distributions():
    from synt_isic_amd import data, ops
    n, H, W = 2000, 128, 128
    p, fallback = data.draw_augment_params(np.arange(n), 0, 1, H, W, return_fallback=True)
    ops.validate_augment_params(p, n, H, W)
    assert (p["crop_x"] >= 0).all() and (p["crop_y"] >= 0).all() and (p["crop_w"] > 0).all() and (p["crop_h"] > 0).all()
    assert (p["crop_x"] + p["crop_w"] <= W).all() and (p["crop_y"] + p["crop_h"] <= H).all()
    assert (np.sort(p["order"], axis=1) == np.arange(3)).all()
    for op, v in enumerate((0.3, 0.3, 0.2)):
        f = p["factor"][:, op]
        assert (f >= np.float32(1 - v)).all() and (f <= np.float32(1 + v)).all() and f.std() > 0.4 * v
    # crop area: w and h are each rounded by at most 1/2, so the share moves by at most (w + h + 0.5) / 2 / (H W) < 1 / min(H, W)
    share = p["crop_w"].astype(float) * p["crop_h"] / (H * W)
    slack = 1.0 / min(H, W)
    drawn = ~fallback
    print(f"fallback crops: {fallback.sum()} of {n}; drawn area share {share[drawn].min():.4f} .. {share[drawn].max():.4f}")
    assert (share[drawn] >= 0.9 - slack).all() and (share[drawn] <= 1.0 + slack).all()
    assert (p["crop_w"][fallback] == W).all() and (p["crop_h"][fallback] == H).all()      # 128x128 lies inside the ratio range
    assert 0 < fallback.sum() < n // 2
    aspect = p["crop_w"][drawn] / p["crop_h"][drawn]
    assert (aspect > 0.74).all() and (aspect < 1.35).all()
    # shares of 1/2: binomial 4-sigma bands
    band = 4 * math.sqrt(0.25 / n)
    for name in ("rotate", "hflip", "vflip"):
        assert abs(p[name].mean() - 0.5) <= band, (name, p[name].mean())
    rot = p[p["rotate"] == 1]["rot"]
    cos15 = math.cos(math.radians(15.0))
    assert (rot[:, 0] <= 65536).all() and (rot[:, 0] >= math.floor(cos15 * 65536)).all() and (rot[:, 0] == rot[:, 4]).all()
    assert (np.abs(rot[:, 1] + rot[:, 3]) <= 1).all() and (np.abs(rot[:, 1]) <= math.ceil(math.sin(math.radians(15.0)) * 65536)).all()
    assert (p[p["rotate"] == 0]["rot"] == 0).all() and (p["reserved"] == 0).all()
    assert len({tuple(o) for o in p["order"]}) == 6


def test_draw_options_and_fallback_crop():
    from synt_isic_amd import data
    p = data.draw_augment_params(np.arange(64), 0, 0, 32, 32, brightness=0.0, p_rotate=0.0, hflip=False, vflip=False)
    assert (p["rotate"] == 0).all() and (p["hflip"] == 0).all() and (p["vflip"] == 0).all()
    assert ((p["order"] == 0).sum(axis=1) == 0).all() and ((p["order"] == -1).sum(axis=1) == 1).all()
    q = data.draw_augment_params(np.arange(64), 0, 0, 32, 32)
    assert (q["factor"][:, 1:] == p["factor"][:, 1:]).all() and (q["crop_w"] == p["crop_w"]).all()      # the draws do not shift
    # 16 x 64: in_ratio 4 > 4/3, every attempt fails, the fallback is the central h x round(h * 4/3) crop
    f, fb = data.draw_augment_params(np.arange(8), 0, 0, 16, 64, return_fallback=True)
    assert fb.all() and (f["crop_h"] == 16).all() and (f["crop_w"] == 21).all() and (f["crop_x"] == (64 - 21) // 2).all()
    ident = data.identity_params([2, 0], 24, 40)
    assert list(ident["src"]) == [2, 0] and (ident["order"] == -1).all() and (ident["crop_w"] == 40).all() and (ident["crop_h"] == 24).all()
    imgs = np.random.default_rng(0).integers(0, 256, size=(3, 24, 40, 3), dtype=np.uint8)
    assert np.array_equal(R.augment_u8(imgs, ident[0]), imgs[2])


def test_record_validation():
    from synt_isic_amd import _lib, ops
    good = R.make_record(1, 32, 32, box=(2, 3, 30, 29))
    ops.validate_augment_params(np.array([good, good]), 2, 32, 32)
    for field, value, size in (("src", 2, (32, 32)), ("src", -1, (32, 32)), ("crop_w", 33, (32, 32)), ("crop_w", 0, (32, 32)),
                               ("crop_x", 3, (32, 32)), ("crop_y", -1, (32, 32)), ("crop_h", 30, (32, 32)), ("src", 0, (32, 36))):
        bad = np.array([good, good])
        bad[field][1] = value
        with pytest.raises(_lib.SisicError) as e:
            ops.validate_augment_params(bad, 2, *size)
        assert e.value.code == _lib.SISIC_EINVAL and "augment" in str(e.value)
    bad = np.array([good])
    bad["order"][0] = (0, 3, 1)
    with pytest.raises(_lib.SisicError):
        ops.validate_augment_params(bad, 2, 32, 32)


# ---- colour correction, epochs, the ISIC reader --------------------------------------------------------------------------------
def test_enhance_color_matches_the_formula():
    from synt_isic_amd import data
    img = np.random.default_rng(3).integers(0, 256, size=(24, 40, 3), dtype=np.uint8)
    assert sorted(data.CLASS_COLOR_PARAMS) == list(range(7))
    for class_id, cp in data.CLASS_COLOR_PARAMS.items():
        x = img.astype(np.float32) / 255.0
        want = np.empty_like(x)
        for c in range(3):
            mean_c = np.mean(x, axis=(0, 1))[c]
            want[..., c] = np.clip(x[..., c] + (cp["target"][c] - mean_c) * cp["gain"][c] + cp["brightness"], 0, 1)
        got = data.enhance_color(img, class_id)
        assert got.dtype == np.uint8 and np.array_equal(got, (want * 255).astype(np.uint8))
        assert not np.array_equal(got, img)


@pytest.mark.parametrize("n,batch,drop_last", [(8, 2, False), (11, 4, False), (11, 4, True), (5, 8, False), (5, 8, True)])
def test_epoch_batches_cover_every_index_once(n, batch, drop_last):
    from synt_isic_amd import data
    seen = []
    for epoch in range(3):
        batches = data.epoch_batches(n, batch, epoch, seed=9, shuffle=True, drop_last=drop_last)
        assert len(batches) == (n // batch if drop_last else -(-n // batch))
        assert all(len(b) == batch for b in batches[:-1]) and (not batches or len(batches[-1]) == (batch if drop_last or n % batch == 0 else n % batch))
        flat = np.concatenate(batches) if batches else np.array([], dtype=int)
        assert len(set(flat.tolist())) == len(flat) and set(flat.tolist()) <= set(range(n))
        if not drop_last:
            assert sorted(flat.tolist()) == list(range(n))
        else:
            assert len(flat) == n - n % batch
        seen.append(flat.tolist())
        assert seen[-1] == np.concatenate(data.epoch_batches(n, batch, epoch, 9, True, drop_last) or [np.array([], dtype=int)]).tolist()
    if n >= 8:
        assert seen[0] != seen[1]
    plain = data.epoch_batches(n, batch, 0, 9, shuffle=False, drop_last=False)
    assert np.concatenate(plain).tolist() == list(range(n))


def test_load_isic_reads_the_reference_layout(tmp_path):
    pytest.importorskip("pandas")
    Image = pytest.importorskip("PIL.Image")
    from synt_isic_amd import data
    rng = np.random.default_rng(5)
    classes = ["MEL", "NV", "BCC", "AKIEC", "BKL", "DF", "VASC"]
    labels = [1, 1, 0, 1, 2, 1, 1, 1]
    lines = ["image," + ",".join(classes)]
    for k, lab in enumerate(labels):
        name = f"ISIC_{k:07d}"
        lines.append(name + "," + ",".join("1.0" if c == lab else "0.0" for c in range(7)))
        if k != 3:                                   # listed in the CSV, absent from the folder
            Image.fromarray(rng.integers(0, 256, size=(20 + k, 30, 3), dtype=np.uint8)).save(tmp_path / (name + ".jpg"), quality=95)
    (tmp_path / "truth.csv").write_text("\n".join(lines) + "\n")
    imgs = data.DeviceDataset.load_isic(str(tmp_path), str(tmp_path / "truth.csv"), class_id=1, image_size=16, max_samples=500)
    assert imgs.shape == (5, 16, 16, 3) and imgs.dtype == np.uint8
    names = sorted(f"ISIC_{k:07d}" for k, lab in enumerate(labels) if lab == 1 and k != 3)
    want = {n: data.enhance_color(np.asarray(Image.open(tmp_path / (n + ".jpg")).convert("RGB").resize((16, 16))), 1) for n in names}
    assert sorted(im.tobytes() for im in imgs) == sorted(w.tobytes() for w in want.values())
    capped = data.DeviceDataset.load_isic(str(tmp_path), str(tmp_path / "truth.csv"), class_id=1, image_size=16, max_samples=3)
    assert capped.shape[0] == 3
    again = data.DeviceDataset.load_isic(str(tmp_path), str(tmp_path / "truth.csv"), class_id=1, image_size=16, max_samples=3)
    assert np.array_equal(capped, again)
    with pytest.raises(ValueError):
        data.DeviceDataset.load_isic(str(tmp_path), str(tmp_path / "truth.csv"), class_id=6, image_size=16)
