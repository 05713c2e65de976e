"""Dynamic thresholding of x0 without a GPU: the contract's spelling of the quantile against torch's own, the numpy model of the
kernel's selection against sorting, the composed step against the clamped one at sample_max_value = 1, planted errors, and the
refusals and records of the Python interface (tests/threshold_ref.py)."""
import numpy as np
import pytest
import torch

import pred_ref
import threshold_ref as tr

SHAPES = (1, 2, 27, 105, 192, 768, 12288, 49152)
RATIOS = (0.0, 0.5, 0.9, 0.995, 0.999, 1.0)
KINDS = ("draws", "eighths", "equal", "zeros", "inf", "nan")


def make_rows(n: int, seed: int = 0) -> torch.Tensor:
    """[6, n] fp32: ordinary draws; draws quantised to 1/8, so that ties straddle the lo / hi boundary; an all-equal row; +-0; a
    row holding inf; a row holding NaN"""
    g = torch.Generator().manual_seed(1000 * seed + n)
    rows = torch.randn((len(KINDS), n), generator=g) * 1.7
    rows[1] = torch.round(rows[1] * 8) / 8
    rows[2] = 1.375
    rows[3] = 0.0
    rows[3, ::2] = -0.0
    rows[4, n // 2] = float("inf")
    rows[5, n // 3] = float("nan")
    return rows


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    nan = torch.isnan(a.view(torch.float32)) & torch.isnan(b.view(torch.float32))
    return bool(((a == b) | nan).all())


@pytest.fixture(scope="module")
def rows_by_n():
    return {n: make_rows(n) for n in SHAPES}


@pytest.mark.parametrize("n", SHAPES)
def test_restatement_equals_torch(n, rows_by_n):
    """the spelled-out quantile, the clamp and the division equal torch.quantile, clamp and / on CPU torch, bit for bit"""
    x0 = rows_by_n[n]
    for ratio in RATIOS:
        for max_value in (1.0, 2.5):
            want_x0, want_s = tr.torch_threshold(x0, ratio, max_value)
            got_s = tr.threshold_s(x0, ratio, max_value)
            assert same_bits(got_s, want_s), (n, ratio, max_value, got_s, want_s)
            assert same_bits(tr.apply_s(x0, got_s), want_x0), (n, ratio, max_value)
            assert torch.isnan(got_s[5]) and torch.isnan(tr.apply_s(x0, got_s)[5]).all()      # a NaN anywhere: a NaN image


def test_regimes_occur(rows_by_n):
    """the inputs reach s clamped to 1, s inside (1, max) and s clamped to max: the comparison above is not all one branch"""
    seen = set()
    for n in SHAPES:
        for ratio in RATIOS:
            for v in tr.threshold_s(rows_by_n[n][:3], ratio, 2.5).tolist():
                seen.add("one" if v == 1.0 else "max" if v == 2.5 else "inside")
    assert seen == {"one", "inside", "max"}


@pytest.mark.parametrize("n", SHAPES)
def test_selection_model_equals_sorting(n, rows_by_n):
    """the kernel's algorithm -- the passes, the count, the successor rule -- finds the order statistics that sorting finds"""
    for row in rows_by_n[n][:5]:
        keys = tr.keys_of(row.numpy())
        order = np.sort(keys)
        for ratio in RATIOS:
            lo, hi, _ = tr.rank_of(ratio, n)
            a_lo, a_hi, cnt_le, has_nan = tr.radix_select_model(keys, lo, hi)
            assert (a_lo, a_hi) == (int(order[lo]), int(order[hi])) and not has_nan
            assert cnt_le == int((keys <= np.uint32(a_lo)).sum())
            got, want = tr.model_s(row.numpy(), ratio, 2.5), tr.clamp_s(tr.quantile_spelled(row.numpy(), ratio), 2.5)
            assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)
    assert np.isnan(tr.model_s(rows_by_n[n][5].numpy(), 0.5, 2.5))


def test_fma32_is_one_rounding():
    a, b, c = np.float32(1 + 2 ** -12), np.float32(1 + 2 ** -12), np.float32(-1.0)
    assert float(tr.fma32(a, b, c)) == 2 ** -11 + 2 ** -24                       # the product's low bits survive
    assert float(np.float32(np.float32(a * b) + c)) != float(tr.fma32(a, b, c))
    assert tr.fma32(np.float32(0.25), np.float32(np.inf), np.float32(1.0)) == np.inf
    assert np.isnan(tr.fma32(np.float32(0.0), np.float32(np.inf), np.float32(1.0)))


ROWS = {"ddpm": (0.6, 0.8, 0.45, 0.5, 0.25), "ddim": (0.6, 0.8, 0.9, 0.3, 0.25), "dpmsolver++": (0.6, 0.8, 0.9, 0.3, 0.25, -0.1)}


def _step_inputs(n=105, B=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    o, x, z, hist = (torch.randn((B, n), generator=g) for _ in range(4))
    return o * 1.5, x * 1.5, z, hist


@pytest.mark.parametrize("rule", sorted(ROWS))
@pytest.mark.parametrize("ptype", pred_ref.TYPES)
def test_max_one_is_the_static_clip(rule, ptype):
    """sample_max_value = 1 makes s exactly 1: the thresholded step is the step under clip = 1, bit for bit"""
    o, x, z, hist = _step_inputs()
    for clipped in ((False, True) if rule == "ddim" else (False,)):
        got, got_hist, s = tr.step_row(rule, o, x, z, hist, ROWS[rule], (0.995, 1.0), ptype, clipped)
        want, want_hist = pred_ref.step_row(rule, o, x, z, hist, ROWS[rule], 1.0, ptype, clipped)
        assert (s == 1.0).all() and same_bits(got, want)
        assert want_hist is None or same_bits(got_hist, want_hist)
        # and a maximum above 1 is another step
        other, _, s2 = tr.step_row(rule, o, x, z, hist, ROWS[rule], (0.995, 4.0), ptype, clipped)
        assert (s2 > 1.0).any() and not same_bits(other, want)


def test_planted_errors_change_bits():
    """each mistake an implementation could make moves the result on these inputs"""
    x0 = make_rows(105)[:2] * 1.0
    ratio, max_value = 0.9, 8.0
    right_s = tr.threshold_s(x0, ratio, max_value)
    right = tr.apply_s(x0, right_s)
    assert ((right_s > 1.0) & (right_s < max_value)).all()
    # the rank over n instead of n - 1
    assert not same_bits(tr.threshold_s(x0, ratio, max_value, rank_n=105 + 1), right_s)
    # one quantile over the whole batch
    whole = tr.threshold_s(x0.reshape(1, -1), ratio, max_value).expand(2)
    assert not same_bits(whole.contiguous(), right_s)
    # the division left out
    sv = right_s.reshape(-1, 1)
    assert not same_bits(torch.clamp(x0, -sv, sv), right)
    # abs left out
    assert not same_bits(tr.threshold_s(x0, ratio, max_value, use_abs=False), right_s)
    # the unfused interpolation, on an input where the two roundings show
    found = None
    for seed in range(400):
        row = make_rows(105, seed=seed)[0].numpy()
        if tr.quantile_spelled(row, 0.995) != tr.quantile_spelled(row, 0.995, interp=tr.unfused_interpolate):
            found = seed
            break
    assert found is not None, "no input separates the fused interpolation from the unfused one"
    row = make_rows(105, seed=found)[:1]
    _, want_s = tr.torch_threshold(row, 0.995, 100.0)
    assert same_bits(tr.threshold_s(row, 0.995, 100.0), want_s)
    assert not same_bits(tr.threshold_s(row, 0.995, 100.0, interp=tr.unfused_interpolate), want_s)


# ---- the Python interface: what needs no GPU ----------------------------------------------------------------------------------
def _mirrors():
    from synt_isic_amd.scheduler import HipDDIMScheduler, HipDDPMScheduler, HipDPMSolverMultistepScheduler
    return HipDDPMScheduler, HipDDIMScheduler, HipDPMSolverMultistepScheduler


def test_mirrors_take_the_published_arguments():
    """every mirror has set_thresholding under the published names and defaults; the DDPM mirror also takes them in its
    constructor.  The DDIM and DPM-Solver++ constructors keep refusing them (tests/test_ddim_cpu.py and tests/test_dpmpp_cpu.py
    assert that), as they keep refusing prediction_type="v_prediction"; their configs hold what their constructors take."""
    DDPM, DDIM, DPM = _mirrors()
    for cls in (DDPM, DDIM, DPM):
        sched = cls()
        assert sched.threshold is None
        sched.set_thresholding(True, dynamic_thresholding_ratio=0.9, sample_max_value=2.0)
        assert sched.threshold == (0.9, 2.0)
        sched.set_timesteps(10)                                        # a new run keeps the setting
        assert sched.threshold == (0.9, 2.0)
        again = cls(**vars(sched.config))                              # a config rebuilds its scheduler
        assert vars(again.config) == vars(sched.config)
        sched.set_thresholding()                                       # the published defaults: ratio 0.995, maximum 1
        assert sched.threshold == (0.995, 1.0)
        # off: the two companions are not judged, as in the published classes
        sched.set_thresholding(False, sample_max_value=0.5)
        assert sched.threshold is None
    off = DDPM()
    assert off.config.thresholding is False and off.config.dynamic_thresholding_ratio == 0.995 and off.config.sample_max_value == 1.0
    on = DDPM(thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=2.0)
    assert on.threshold == (0.9, 2.0) and on.config.thresholding is True
    assert DDPM(**vars(on.config)).threshold == (0.9, 2.0)
    off.set_thresholding(True, 0.9, 2.0)
    assert (off.config.thresholding, off.config.dynamic_thresholding_ratio, off.config.sample_max_value) == (True, 0.9, 2.0)
    assert DDPM(thresholding=False, sample_max_value=0.5).threshold is None
    for cls in (DDIM, DPM):
        assert not hasattr(cls().config, "thresholding")
        with pytest.raises(NotImplementedError, match="set_thresholding"):
            cls(thresholding=True)


BAD = [dict(dynamic_thresholding_ratio=-0.1), dict(dynamic_thresholding_ratio=1.5), dict(dynamic_thresholding_ratio=float("nan")),
       dict(dynamic_thresholding_ratio=float("inf")), dict(sample_max_value=0.5), dict(sample_max_value=float("nan")),
       dict(sample_max_value=float("inf"))]


@pytest.mark.parametrize("bad", BAD)
def test_refusals(bad):
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import check_thresholding
    with pytest.raises(ValueError):
        _mirrors()[0](thresholding=True, **bad)
    for cls in _mirrors():
        sched = cls()
        sched.set_thresholding(True, 0.9, 2.0)
        with pytest.raises(ValueError):
            sched.set_thresholding(True, **bad)
        assert sched.threshold == (0.9, 2.0)                           # the previous setting stays in force
    with pytest.raises(ValueError):
        check_thresholding(True, **bad)
    with pytest.raises(ValueError):
        ops.check_threshold((bad.get("dynamic_thresholding_ratio", 0.995), bad.get("sample_max_value", 1.0)))
    assert check_thresholding(False, **bad) is None


def test_image_size_refusal():
    """more than 2^24 elements per image: n - 1 would not be exact in fp32"""
    from synt_isic_amd import ops
    from synt_isic_amd.sampler import run_sampling_loop
    DDPM = _mirrors()[0]
    sched = DDPM(thresholding=True, sample_max_value=2.0)
    x = torch.zeros((1, 1, 4097, 4096))
    assert x[0].numel() > ops.THRESHOLD_MAX_PER_IMAGE
    with pytest.raises(ValueError, match="2\\*\\*24"):
        run_sampling_loop(None, sched, x, None)
    with pytest.raises(ValueError, match="2\\*\\*24"):
        run_sampling_loop(None, DDPM(), x, None, thresholding=True)
    with pytest.raises(ValueError, match="2\\*\\*24"):
        ops._step_context(x, "epsilon", (0.995, 2.0))


def test_generate_takes_the_arguments():
    """the public entry points name the three arguments, and the result has a place for the setting"""
    import inspect
    from synt_isic_amd.sampler import SampleResult, Sampler, run_sampling_loop
    for fn in (Sampler.generate, Sampler.generate_seeds, run_sampling_loop):
        params = inspect.signature(fn).parameters
        assert {"thresholding", "dynamic_thresholding_ratio", "sample_max_value"} <= set(params), fn
        assert params["dynamic_thresholding_ratio"].default == 0.995 and params["sample_max_value"].default == 1.0
    assert SampleResult(images=None, latents=None).thresholding is None
