"""Host side of the counterfactual-intervention stage (synt_isic_amd.xai): region selection against scipy.ndimage, the
key-frame rule, the C ABI names.  No GPU.

``select_regions`` must give scipy.ndimage's masks pixel for pixel without importing scipy.  The expected masks were
recorded with scipy into tests/golden/xai_regions.npz (tests/golden/make_xai_regions.py); every case is compared with the
fixture, and with live scipy as well where it is installed.  The float statistics are numpy reductions of (attribution,
mask): they are compared exactly with the same reductions over the fixture's mask, and with the recorded values to 1e-6
relative (the summation order inside numpy is not something this project fixes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import xai_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return xai_ref.load_region_fixture(os.path.join(golden_dir, "xai_regions.npz"))


def _have_scipy() -> bool:
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except Exception:
        return False


def test_fixture_does_real_work(fixture):
    """the recorded masks are not trivial: at connectivity 8 every cleaned mask is non-empty (169 to 8223 pixels), and the
    clean-up changes the thresholded mask"""
    changed = 0
    for case, (mask, _, selected, _) in fixture.items():
        assert mask.sum() == selected
        if case[5]:
            if case[4] == 8:
                assert 169 <= selected <= 8223, case
            raw = fixture[case[:5] + (False,)][0]
            changed += int(not np.array_equal(raw, mask))
    assert changed >= 90          # 96 cleaned cases


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("pool", [1, 9, 15])
def test_select_regions_matches_scipy(fixture, seed, H, pool):
    from synt_isic_amd import xai
    attr = xai_ref.region_input(seed, H, pool)
    live = _have_scipy()
    for rt in ("top", "bottom"):
        for conn in (4, 8):
            for cleanup in (True, False):
                what = f"seed {seed} {H}x{H} pool {pool} {rt} connectivity {conn} cleanup {cleanup}"
                want_mask, want_thr, want_sel, want_f = fixture[(seed, H, pool, rt, conn, cleanup)]
                got = xai.select_regions(attr, k_percent=10, region_type=rt, morphology_cleanup=cleanup, connectivity=conn)
                assert set(got) == {"mask", "threshold", "statistics", "metadata"}
                assert got["mask"].dtype == bool and got["mask"].shape == (H, H)
                assert np.array_equal(got["mask"], want_mask), f"{what}: {np.sum(got['mask'] != want_mask)} pixels differ"
                assert got["threshold"] == want_thr, what
                st = got["statistics"]
                ref = xai_ref.region_statistics(attr, want_mask, want_thr)
                assert set(st) == set(ref)
                for k, v in ref.items():
                    assert st[k] == v, f"{what}: statistics[{k}] = {st[k]} != {v}"
                assert st["selected_pixels"] == want_sel and st["total_pixels"] == H * H
                np.testing.assert_allclose([float(st[k]) for k in xai_ref.FLOAT_STATS], want_f, rtol=1e-6, atol=0, err_msg=what)
                assert got["metadata"] == {"region_type": rt, "morphology_cleanup": cleanup, "connectivity": conn,
                                           "original_shape": (1, 3, H, H)}
                if live:
                    m2, t2 = xai_ref.regions_scipy(attr, 10, rt, cleanup, conn)
                    assert np.array_equal(got["mask"], m2) and got["threshold"] == t2, f"{what}: differs from live scipy"


def test_select_regions_input_forms():
    from synt_isic_amd import xai
    attr = xai_ref.region_input(1, 64, 9)
    a = xai.select_regions(attr)                                   # [1,3,H,W] tensor: L2 norm over the channels
    b = xai.select_regions(attr[0].numpy())                        # [3,H,W] numpy
    c = xai.select_regions(np.linalg.norm(attr[0].numpy(), axis=0))     # [H,W]: |.|
    d = xai.select_regions(-np.linalg.norm(attr[0].numpy(), axis=0))
    assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["mask"], c["mask"]) and np.array_equal(a["mask"], d["mask"])
    assert a["statistics"]["target_percentage"] == 10 and a["metadata"]["region_type"] == "top"
    with pytest.raises(ValueError):
        xai.select_regions(attr, region_type="middle")
    empty = xai.select_regions(np.zeros((64, 64), dtype=np.float32) + np.eye(64, dtype=np.float32), k_percent=1)
    assert empty["mask"].sum() == 0 and empty["statistics"]["mean_attribution_selected"] == 0     # the diagonal does not survive the opening


@pytest.mark.parametrize("n,want", [(1, [0]), (3, [0, 1, 2]), (6, [0, 3, 2, 4, 5]), (50, [0, 25, 46, 47, 48, 49])])
def test_key_steps(n, want):
    from synt_isic_amd import xai
    assert xai.key_steps(n) == want == xai_ref.key_steps(n)


def test_xai_does_not_import_scipy():
    code = ("import sys; import synt_isic_amd.xai as x; import numpy as np; "
            "x.select_regions(np.random.default_rng(0).random((3, 32, 32)).astype('float32')); "
            "bad = [m for m in sys.modules if m == 'scipy' or m.startswith('scipy.')]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    src = open(os.path.join(ROOT, "synt_isic_amd", "xai.py")).read()
    assert "import scipy" not in src and "from scipy" not in src


def test_new_entries_are_bound():
    import ctypes
    from synt_isic_amd import _lib, ops
    assert "sisic_intervene" in _lib.SIGNATURES and "sisic_cfi_metrics" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.InterventionJob) == 20
    assert list(ops.INTERVENTION_TYPES) == list(xai_ref.TYPES) and list(ops.INTERVENTION_TYPES.values()) == list(range(7))
    assert _lib.ABI_VERSION == 3
