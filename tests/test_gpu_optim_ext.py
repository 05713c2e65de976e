"""Global-norm clipping and the EMA of the weights: the two kernels on vectors of the test's own (sisic_grad_stats,
sisic_adam_ema), then through the model (HipAdam(max_grad_norm=, ema=), HipEMA, train_step_fused, train_class).

Vector sizes are where the kernels can go wrong: 1, 3 (no whole 16-byte vector), 255 and 1025 (either side of a block, a
scalar tail), 5 000 003 (more than 4096 blocks x 256 threads x 4 floats: a second grid-stride round, and a tail), and 1025 on
a base pointer one float past a 16-byte boundary (a scalar head of three).  Gradients are randn * 10^U(-8, 0), as in
test_gpu_optimizer.py.

The bars, and where they come from:
  * total_norm: 1 fp32 ulp from float32(sqrt(float64 sum of squares)).  A double sum of non-negative terms in any order is
    ~1e-13 relative from exact, far inside half an fp32 ulp (6e-8) except at a rounding boundary: hence 1 ulp, not 0.
  * clip_coef, the fused update against its torch fp32 restatement (optim_ext_ref.adam_update), the EMA: bit for bit.  Both
    sides perform the same fp32 operations in the same order on the same inputs.
  * parameters under active clipping: test_gpu_optimizer.py's yardstick, restated here -- at most ADAM_BAR times as far from a
    float64 torch.optim.Adam on the same clipped fp32 gradients as torch's own fp32 Adam is.
"""
import ctypes as C
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import optim_ext_ref as ref
from poison import guard_bands, poison_allocations, unwritten  # noqa: F401  (autouse: poisoned, guarded allocations -- tests/poison.py)

pytestmark = pytest.mark.gpu

DEV = "cuda"
ADAM_BAR = 2.0               # the project's bar for the Adam update's operation order (test_gpu_optimizer.py)
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
BIG = 5_000_003
CASES = [(1, 0), (3, 0), (255, 0), (1025, 0), (BIG, 0), (1025, 1)]
CASE_IDS = [f"n{n}" + ("+1float" if off else "") for n, off in CASES]


def _lib():
    from synt_isic_amd import _lib
    return _lib


def _ctx():
    from synt_isic_amd import ops
    return ops.context(torch.device(DEV))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(host: torch.Tensor, offset: int = 0) -> torch.Tensor:
    """``host`` on the device inside a poisoned, guarded allocation, ``offset`` floats past its 16-byte-aligned start"""
    from synt_isic_amd import ops
    base = ops.empty(host.numel() + offset, dtype=host.dtype, device=DEV)
    assert base.data_ptr() % 16 == 0
    view = base[offset:]
    view.copy_(host)
    return view


def _grad(n: int, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen) * torch.exp(torch.rand(n, generator=gen) * (-8.0 * math.log(10.0)))


def _grad_stats(g_dev: torch.Tensor, inv_scale: float, max_norm: float):
    """(total_norm fp32, clip_coef fp32, found_inf, the record's 12 bytes)"""
    from synt_isic_amd import ops
    lib = _lib()
    rec = ops.empty(3, dtype=torch.int32, device=DEV)
    lib.check(lib.load().sisic_grad_stats(_ctx(), g_dev.data_ptr(), g_dev.numel(), inv_scale, max_norm, rec.data_ptr(), _stream()))
    torch.cuda.synchronize()
    raw = rec.cpu().numpy().copy()
    f = raw.view(np.float32)
    return f[0], f[1], int(raw[2]), raw.tobytes(), rec


def _within_one_ulp(got: np.float32, want: np.float32) -> bool:
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))


# ================================================================ 1. the norm =========================================
@pytest.mark.parametrize("n,offset", CASES, ids=CASE_IDS)
def test_grad_stats_norm_and_coefficient(n, offset):
    g = _grad(n, 100 + n % 977 + offset)
    gd = _dev(g, offset)
    inv_scale, max_norm = float(np.float32(1.0 / 3.0)), 0.01
    norm, coef, flag, bits, _ = _grad_stats(gd, inv_scale, max_norm)
    norm64, norm32, _ = ref.clip_stats(g, inv_scale, max_norm)
    print(f"n={n} offset={offset}: norm {norm!r} against {norm32!r} (float64 {norm64!r}), coefficient {coef!r}")
    assert flag == 0
    assert _within_one_ulp(norm, norm32), (norm, norm32)
    assert coef.tobytes() == ref.clip_coef_of(norm, max_norm).tobytes(), (coef, ref.clip_coef_of(norm, max_norm))
    if n >= 255:
        assert coef < 1.0                                      # the norm is far above 0.01: the case exercises the clamp's other arm
    assert _grad_stats(gd, inv_scale, max_norm)[3] == bits     # a fixed summation order: the same bits again
    assert torch.equal(gd.cpu(), g)                            # the gradient is read only


@pytest.mark.parametrize("value", [math.inf, -math.inf, math.nan], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("n,offset,at", [(1025, 0, 0), (1025, 0, 1024), (1025, 1, 1), (BIG, 0, 4096 * 256 * 4 + 5),
                                         (BIG, 0, BIG - 1)],
                         ids=["first", "tail", "head", "second-round", "last"])
def test_grad_stats_flags_one_non_finite_element(n, offset, at, value):
    g = _grad(n, 7)
    g[at] = value
    norm, coef, flag, _, _ = _grad_stats(_dev(g, offset), 1.0, 1.0)
    assert flag == 1
    # torch's arithmetic, no special cases: an infinite norm clips to 0, a NaN norm gives a NaN coefficient
    assert (math.isnan(norm) and math.isnan(coef)) if math.isnan(value) else (math.isinf(norm) and coef == 0.0)
    clean = _grad(n, 7)
    assert _grad_stats(_dev(clean, offset), 1.0, 1.0)[2] == 0  # the flag is not sticky


def test_grad_stats_sums_in_double():
    """300 gradients of 1e18: their squares sum to 3e38, past fp32; the norm, 1.7e19, is an ordinary fp32 value."""
    g = _grad(1025, 8)
    g[400:700] = 1e18
    g[500:600] = -1e18
    norm, coef, flag, _, _ = _grad_stats(_dev(g), 1.0, 1.0)
    _, norm32, _ = ref.clip_stats(g, 1.0, 1.0)
    assert flag == 0 and math.isfinite(norm) and 1.7e19 < norm < 1.8e19
    assert _within_one_ulp(norm, norm32), (norm, norm32)
    assert coef.tobytes() == ref.clip_coef_of(norm, 1.0).tobytes() and 0.0 < coef < 1e-18


@pytest.mark.parametrize("max_norm", [math.inf, 0.0, -1.0])
def test_grad_stats_without_a_bound_reports_the_norm_only(max_norm):
    g = _grad(1025, 9)
    norm, coef, flag, _, _ = _grad_stats(_dev(g), 1.0, max_norm)
    assert flag == 0 and coef.tobytes() == np.float32(1.0).tobytes()
    assert _within_one_ulp(norm, ref.clip_stats(g, 1.0, 1.0)[1])


# ================================================================ 2. / 3. the fused update ============================
def _adam_ema(p, g, m, v, ema, step, inv_scale=1.0, stats=None, decay=0.0):
    lib = _lib()
    lib.check(lib.load().sisic_adam_ema(_ctx(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        ema.data_ptr() if ema is not None else None, p.numel(), ADAM["lr"], ADAM["beta1"],
                                        ADAM["beta2"], ADAM["eps"], step, inv_scale,
                                        stats.data_ptr() if stats is not None else None, decay, _stream()))


def _state(n, offset, seed):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen) * 0.05
    return [_dev(t, offset) for t in (p0, torch.zeros(n), torch.zeros(n))]


def _host_state(n, seed):
    """_state's values on the host, for ref.adam_update"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen) * 0.05, torch.zeros(n), torch.zeros(n)


def _same_bits(dev_tensors, host_tensors):
    return all(torch.equal(d.cpu(), h) for d, h in zip(dev_tensors, host_tensors))


@pytest.mark.parametrize("n,offset", CASES, ids=CASE_IDS)
def test_fused_update_equals_the_parent_kernel_on_the_clipped_gradient(n, offset):
    """sisic_adam_ema reading the coefficient c from the record, and the null-record, null-EMA route fed g' = (g * 1) * c formed
    in torch fp32, against the torch fp32 restatement of the update (ref.adam_update, one rounded operation per line -- the
    anchor that the deleted scalar adam_kernel was; that kernel gave the restatement's bits): p, m and v bit for bit over
    three steps."""
    pa, ma, va = _state(n, offset, 21)
    pb, mb, vb = _state(n, offset, 21)
    want = _host_state(n, 21)
    clipped = 0
    for step in (1, 2, 3):
        g = _grad(n, 30 + step)
        gd = _dev(g, offset)
        _, coef, _, _, rec = _grad_stats(gd, 1.0, 0.01)
        clipped += coef < 1.0
        _adam_ema(pa, gd, ma, va, None, step, stats=rec)
        g2 = _dev((g * torch.tensor(1.0)) * torch.tensor(float(coef)), offset)          # fp32 x fp32, rounded once each
        assert g2.dtype == torch.float32
        _adam_ema(pb, g2, mb, vb, None, step)
        torch.cuda.synchronize()
        ref.adam_update(*want[:1], g, *want[1:], step, 1.0, float(coef), **ADAM)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), f"step {step}"
        assert _same_bits((pa, ma, va), want), f"step {step}: not the restatement's bits"
        assert bool(torch.isfinite(pa).all())
    assert n < 255 or clipped == 3


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9999])
@pytest.mark.parametrize("n,offset", CASES, ids=CASE_IDS)
def test_fused_ema_equals_the_published_update(n, offset, decay):
    """ema = ema - (1 - decay) * (ema - p_new) on the p read back after each of three steps; p, m, v beside it equal the
    no-EMA route's and the torch fp32 restatement's (ref.adam_update, coefficient 1: no record) bit for bit."""
    from synt_isic_amd import ops
    pa, ma, va = _state(n, offset, 22)
    pb, mb, vb = _state(n, offset, 22)
    host = _host_state(n, 22)
    gen = torch.Generator().manual_seed(23)
    ema = _dev(pa.cpu() + 0.01 * torch.randn(n, generator=gen), offset)
    want = ema.clone()
    bystander = ops.empty(n, dtype=torch.float32, device=DEV)              # a would-be EMA buffer that no call is given
    for step in (1, 2, 3):
        g = _grad(n, 40 + step)
        gd = _dev(g, offset)
        _adam_ema(pa, gd, ma, va, ema, step, decay=decay)
        _adam_ema(pb, gd, mb, vb, None, step)
        torch.cuda.synchronize()
        ref.adam_update(*host[:1], g, *host[1:], step, 1.0, 1.0, **ADAM)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), f"step {step}"
        assert _same_bits((pa, ma, va), host), f"step {step}: not the restatement's bits"
        ref.ema_update(want, pa.clone(), decay)
        assert torch.equal(ema, want), f"step {step}: {(ema != want).sum().item()} of {n} EMA elements differ"
    if decay == 0.0:                                                       # e - 1 * (e - p): p up to the rounding of e - p
        assert float((ema - pa).abs().max()) <= float(np.spacing(np.float32(ema.abs().max().item())))
    assert unwritten(bystander) == n


# ================================================================ 4. through the model =================================
class Arena:
    """the tensors of a state dict as one flat host vector in state-dict order"""

    def __init__(self, sd):
        self.names = list(sd)
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.slices, off = {}, 0
        for k, v in sd.items():
            self.slices[k] = slice(off, off + v.numel())
            off += v.numel()
        self.numel = off

    def flat(self, mapping):
        return torch.cat([mapping[k].detach().reshape(-1).cpu() for k in self.names])

    def named(self, flat):
        return OrderedDict((k, flat[self.slices[k]].view(self.shapes[k])) for k in self.names)


@pytest.fixture(scope="module")
def arena(synthetic_sd):
    return Arena(synthetic_sd)


@pytest.fixture(scope="module")
def grads(arena):
    """three gradient arenas, randn * 10^U(-8, 0): a global norm of several hundred"""
    return [_grad(arena.numel, 500 + i) for i in range(3)]


def _new_model(sd):
    from synt_isic_amd.train import HipAdam
    from synt_isic_amd.unet import HipUNet2DModel
    m = HipUNet2DModel()
    m.load_state_dict(sd)
    m = m.to(DEV)
    HipAdam(m)
    return m


@pytest.fixture(scope="module")
def model(synthetic_sd):
    return _new_model(synthetic_sd)


@pytest.fixture(scope="module")
def other(synthetic_sd):
    return _new_model(synthetic_sd)


def _reset(m, sd):
    m.load_state_dict(sd)           # fresh moments, step 0
    m.train()
    assert m.optimizer_state()["step"] == 0
    return m


def _equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def test_a_neutral_bound_is_the_old_arithmetic(synthetic_sd, arena, grads, model, other):
    """(a) max_grad_norm = 1e30 (coefficient exactly 1) and no EMA against the unchanged HipAdam: bit-equal weights and moments."""
    from synt_isic_amd.train import HipAdam
    a, b = _reset(model, synthetic_sd), _reset(other, synthetic_sd)
    opt_a, opt_b = HipAdam(a, max_grad_norm=1e30), HipAdam(b)
    assert opt_a._extension() is not None and opt_b._extension() is None
    for g in grads:
        named = arena.named(g)
        a.set_grads(named), b.set_grads(named)
        assert opt_a.step() is True and opt_b.step() is True
        assert opt_a.grad_norm > 100.0 and opt_b.grad_norm is None
    sa, sb = a.optimizer_state(), b.optimizer_state()
    assert sa["step"] == sb["step"] == 3
    assert _equal(a.state_dict(), b.state_dict())
    assert _equal(sa["exp_avg"], sb["exp_avg"]) and _equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert not _equal(a.state_dict(), synthetic_sd)


def test_b_active_clipping_against_float64_adam(synthetic_sd, arena, grads, model):
    """(b) max_grad_norm = 1: the reported norm within 1 ulp of the float64 one; the weights after three steps at most ADAM_BAR
    times as far from a float64 torch.optim.Adam as torch's fp32 Adam, both fed the clipped fp32 gradients
    fp32(g * c) with c the fp32 coefficient of the reported norm (which test 1 pins to the norm bit for bit)."""
    from oracle import train as otrain
    from synt_isic_amd.train import HipAdam
    m = _reset(model, synthetic_sd)
    opt = HipAdam(m, max_grad_norm=1.0)                         # lr 1e-3, betas (0.9, 0.999), eps 1e-8
    p0 = arena.flat(synthetic_sd)
    sd = {torch.float64: {"arena": p0.double()}, torch.float32: {"arena": p0.clone()}}
    state = {torch.float64: None, torch.float32: None}
    for g in grads:
        m.set_grads(arena.named(g))
        assert opt.step() is True
        norm64, norm32, _ = ref.clip_stats(g, 1.0, 1.0)
        got = np.float32(opt.grad_norm)
        print(f"(b) grad_norm {got!r}, float64 {norm64!r}")
        assert norm64 > 100.0 and _within_one_ulp(got, norm32), (got, norm32)
        clipped = g * torch.tensor(float(ref.clip_coef_of(got, 1.0)))
        assert clipped.dtype == torch.float32
        for dt in state:
            sd[dt], state[dt] = otrain.adam_step(sd[dt], {"arena": clipped}, state[dt], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    assert m.optimizer_state()["step"] == 3
    p = arena.flat(m.state_dict()).double()
    err = (p - sd[torch.float64]["arena"]).abs().max().item()
    yard = (sd[torch.float32]["arena"].double() - sd[torch.float64]["arena"]).abs().max().item()
    print(f"(b) parameters: GPU {err:.3e} from float64, torch fp32 {yard:.3e}, ratio {err / yard:.3f}")
    assert bool(torch.isfinite(p).all()) and err <= ADAM_BAR * yard, (err, yard)


def test_c_a_skipped_step_moves_only_the_ema(synthetic_sd, arena, grads, model):
    """(c) two clean steps (the EMA now lags the weights), then a planted inf under check_inf: step() is False, weights, moments
    and the step counter keep their bits, and the EMA moves by the published rule towards the unchanged weights."""
    from synt_isic_amd import _lib
    from synt_isic_amd.train import HipAdam, HipEMA
    m = _reset(model, synthetic_sd)
    ema = HipEMA(m, decay=0.9999)
    opt = HipAdam(m, max_grad_norm=1.0, ema=ema)
    for g in grads[:2]:
        m.set_grads(arena.named(g))
        assert opt.step(check_inf=True) is True
    before = (m.state_dict(), m.optimizer_state(), ema.shadow_params())
    assert ema.optimization_step == 2 and before[1]["step"] == 2 and not _equal(before[0], before[2])
    bad = grads[2].clone()
    bad[arena.numel // 2 + 1] = math.inf
    m.set_grads(arena.named(bad))
    assert opt.step(check_inf=True) is False
    after = (m.state_dict(), m.optimizer_state(), ema.shadow_params())
    assert after[1]["step"] == 2 and _lib.load().sisic_unet_train_steps(m.handle) == 2
    assert _equal(after[0], before[0]) and _equal(after[1]["exp_avg"], before[1]["exp_avg"])
    assert _equal(after[1]["exp_avg_sq"], before[1]["exp_avg_sq"])
    assert ema.optimization_step == 3 and ema.cur_decay_value == ref.get_decay(3) == 3 / 12
    want = ref.ema_update(arena.flat(before[2]), arena.flat(before[0]), ref.get_decay(3))
    assert torch.equal(arena.flat(after[2]), want)
    assert not _equal(after[2], before[2])


def _forward(m, x):
    m.eval()
    out = m(x, 10).sample.clone()
    m.train()
    return out


def test_d_average_parameters_swaps_the_ema_in_and_back(synthetic_sd, arena, grads, model, other):
    """(d) inside the context the model is the averaged model -- state dict and a forward call, against a fresh model loaded
    with the averaged weights --, optimizer steps raise, and on exit the trained weights and their forward are back."""
    from synt_isic_amd._lib import SisicError
    from synt_isic_amd.train import HipAdam, HipEMA
    m = _reset(model, synthetic_sd)
    ema = HipEMA(m, decay=0.9999)
    opt = HipAdam(m, ema=ema)
    for g in grads[:2]:
        m.set_grads(arena.named(g))
        assert opt.step() is True
    x = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(41)).to(DEV)
    trained, trained_out = m.state_dict(), _forward(m, x)
    shadow = ema.state_dict()["shadow_params"]
    assert not _equal(trained, shadow)
    fresh_out = _forward(_reset(other, shadow), x)
    with ema.average_parameters():
        assert _equal(m.state_dict(), shadow)
        assert torch.equal(_forward(m, x), fresh_out)
        m.set_grads(arena.named(grads[2]))
        with pytest.raises(SisicError, match="swap"):
            opt.step()
        with pytest.raises(RuntimeError):
            m.load_state_dict(synthetic_sd)
    assert not torch.equal(fresh_out, trained_out)
    assert _equal(m.state_dict(), trained) and torch.equal(_forward(m, x), trained_out)
    assert _equal(ema.shadow_params(), shadow) and m.optimizer_state()["step"] == 2
    assert opt.step() is True                                   # and training goes on


def test_e_fused_training_step_with_both(synthetic_sd, arena, model, other):
    """(e) train_step_fused with clipping and the EMA, batch 2 at 32x32, two steps: the EMA follows the weights read back after
    each step by the published rule; a HipEMA state dict round-trips through a second instance bit for bit."""
    from synt_isic_amd.scheduler import HipDDPMScheduler
    from synt_isic_amd.train import HipAdam, HipEMA, HipGradScaler, train_step_fused
    m = _reset(model, synthetic_sd)
    ema = HipEMA(m, decay=0.9999)
    opt, scaler = HipAdam(m, lr=1e-4, max_grad_norm=1.0, ema=ema), HipGradScaler()
    scheduler = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    gen = torch.Generator().manual_seed(51)
    want = arena.flat(synthetic_sd)
    for step in (1, 2):
        images = (torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1).to(DEV)
        noise = torch.randn(2, 3, 32, 32, generator=gen).to(DEV)
        loss, taken = train_step_fused(m, scheduler, images, noise, torch.randint(0, 1000, (2,), generator=gen), opt, scaler)
        assert math.isfinite(loss) and loss > 0 and taken is True
        assert math.isfinite(opt.grad_norm) and opt.grad_norm > 0
        assert ema.optimization_step == step and ema.cur_decay_value == ref.get_decay(step)
        ref.ema_update(want, arena.flat(m.state_dict()), ref.get_decay(step))
        assert torch.equal(arena.flat(ema.shadow_params()), want), f"step {step}"
    assert m.optimizer_state()["step"] == 2 and not torch.equal(want, arena.flat(m.state_dict()))
    saved = ema.state_dict()
    second = HipEMA(_reset(other, synthetic_sd), decay=0.5, use_ema_warmup=True)
    second.load_state_dict(saved)
    again = second.state_dict()
    assert _equal(again.pop("shadow_params"), saved["shadow_params"])
    assert again == {k: v for k, v in saved.items() if k != "shadow_params"}
    assert second.optimization_step == 2 and second.decay == 0.9999 and second.use_ema_warmup is False


def test_f_train_class_saves_the_ema_beside_the_weights(synthetic_sd, model, tmp_path):
    """(f) one epoch over two batches with ema_decay: both checkpoints are written and differ (the EMA lags the weights)."""
    from synt_isic_amd.train import cosine_schedule_with_warmup, train_class
    m = _reset(model, synthetic_sd)
    gen = torch.Generator().manual_seed(61)
    loader = [torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1 for _ in range(2)]
    history = train_class(m, loader, "x", epochs=1, checkpoint_dir=str(tmp_path), generator=torch.Generator().manual_seed(62),
                          log=None, max_grad_norm=1.0, ema_decay=0.9999, lr_schedule=cosine_schedule_with_warmup(1, 2))
    assert len(history) == 1 and math.isfinite(history[0])
    assert sorted(os.listdir(tmp_path)) == ["unet_x_best.pth", "unet_x_best_ema.pth"]
    raw = torch.load(os.path.join(tmp_path, "unet_x_best.pth"), map_location="cpu")
    avg = torch.load(os.path.join(tmp_path, "unet_x_best_ema.pth"), map_location="cpu")
    assert list(raw) == list(avg) == list(synthetic_sd)
    assert all(bool(torch.isfinite(v).all()) for v in avg.values())
    assert not _equal(raw, avg) and _equal(m.state_dict(), raw)
