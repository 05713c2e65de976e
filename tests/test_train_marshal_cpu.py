"""The marshalling of the training entry points without a GPU: ``train_step_fused`` and ``HipAdam.step`` choose one of the
library's symbols by (labels, optimizer options) and build its argument list from common parts.  ``_lib.load()`` is replaced by
a stand-in that records every call; each recorded call is held to ``_lib.SIGNATURES`` -- the argument count, and every argument
convertible by its declared ctypes type, so that a pointer in the wrong slot is an error here and not a crash on the GPU."""
import ctypes as C

import pytest
import torch

from synt_isic_amd import _lib, train
from synt_isic_amd.scheduler import HipDDPMScheduler
from synt_isic_amd.unet import HipUNet2DModel


class Recorder:
    """every attribute is a library function that records (name, args) and returns SISIC_OK (ema_active: 1, an arena exists)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 1 if name == "sisic_unet_ema_active" else 0
        return fn

    def named(self, prefix):
        return [(n, a) for n, a in self.calls if n.startswith(prefix)]


class Model(HipUNet2DModel):
    """a model whose handle exists without a device"""
    handle = C.c_void_p(0x1000)
    device = torch.device("cpu")


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(train, "_stream", lambda dev: C.c_void_p(0))
    return rec


def _held_to_signature(name, args):
    """the call converts under the symbol's declared argument types"""
    argtypes = _lib.SIGNATURES[name][1]
    assert len(args) == len(argtypes), f"{name}: {len(args)} arguments, the signature has {len(argtypes)}"
    for i, (a, t) in enumerate(zip(args, argtypes)):
        try:
            t.from_param(a)
        except (TypeError, C.ArgumentError) as e:
            raise AssertionError(f"{name}: argument {i} ({a!r}) is no {t.__name__}: {e}")


def _found_inf(name, args):
    """the found_inf argument of a step: the one ``int*`` of its signature"""
    (at,) = [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is C.POINTER(C.c_int)]
    return args[at]


def _optimizer(model, with_ext, counter):
    opt = train.HipAdam(model, lr=1e-4, max_grad_norm=1.0 if with_ext else None,
                        ema=train.HipEMA(model) if with_ext else None)
    done = opt._extension_done

    def counted(ext, norm):
        counter.append(ext)
        done(ext, norm)
    opt._extension_done = counted
    return opt


SCALERS = {"none": lambda: None, "enabled": lambda: train.HipGradScaler(), "disabled": lambda: train.HipGradScaler(enabled=False)}


@pytest.mark.parametrize("scaler", list(SCALERS))
@pytest.mark.parametrize("with_ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("with_labels", [False, True], ids=["unconditional", "labels"])
def test_train_step_fused_calls_the_symbol_its_arguments_fit(lib, with_labels, with_ext, scaler):
    model = Model(num_class_embeds=3) if with_labels else Model()
    done = []
    opt = _optimizer(model, with_ext, done)
    sc = SCALERS[scaler]()
    x, noise = torch.zeros(2, 3, 8, 8), torch.ones(2, 3, 8, 8)
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    labels = torch.tensor([2, 0]) if with_labels else None
    lib.calls.clear()
    loss, taken = train.train_step_fused(model, sched, x, noise, torch.tensor([3, 700]), opt, sc, class_labels=labels)
    assert taken is True and loss == 0.0
    steps = lib.named("sisic_unet_train_step")
    want = "sisic_unet_train_step_cond" if with_labels else "sisic_unet_train_step_ext" if with_ext else "sisic_unet_train_step"
    assert [n for n, _ in steps] == [want]
    _held_to_signature(*steps[0])
    assert (_found_inf(*steps[0]) is None) == (scaler != "enabled")
    assert len(done) == (1 if with_ext else 0)
    assert (opt.grad_norm is None) == (not with_ext)
    if with_ext:
        assert opt.ema.optimization_step == 1
    assert model._params_stale is True and not lib.named("sisic_unet_set_loss_weights")


@pytest.mark.parametrize("check_inf", [False, True])
@pytest.mark.parametrize("with_ext", [False, True], ids=["plain", "ext"])
def test_adam_step_calls_the_symbol_its_arguments_fit(lib, with_ext, check_inf):
    model, done = Model(), []
    opt = _optimizer(model, with_ext, done)
    lib.calls.clear()
    assert opt.step(inv_scale=0.5, check_inf=check_inf) is True
    steps = lib.named("sisic_unet_optimizer_step")
    assert [n for n, _ in steps] == ["sisic_unet_optimizer_step_ext" if with_ext else "sisic_unet_optimizer_step"]
    _held_to_signature(*steps[0])
    assert (_found_inf(*steps[0]) is None) == (not check_inf)
    assert steps[0][1][5] == 0.5
    assert len(done) == (1 if with_ext else 0) and model._params_stale is True


@pytest.mark.parametrize("with_labels", [False, True], ids=["unconditional", "labels"])
def test_snr_weights_are_set_for_the_call_and_cleared(lib, with_labels):
    model = Model(num_class_embeds=3) if with_labels else Model()
    opt = _optimizer(model, False, [])
    sched = HipDDPMScheduler(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2")
    lib.calls.clear()
    train.train_step_fused(model, sched, torch.zeros(2, 3, 8, 8), torch.ones(2, 3, 8, 8), torch.tensor([3, 700]), opt,
                           class_labels=torch.tensor([1, 1]) if with_labels else None, snr_gamma=5.0)
    names = [n for n, _ in lib.calls if n.startswith(("sisic_unet_train_step", "sisic_unet_set_loss_weights"))]
    assert names == ["sisic_unet_set_loss_weights", names[1], "sisic_unet_set_loss_weights"] and "train_step" in names[1]
    (_, set_args), (_, clear_args) = lib.named("sisic_unet_set_loss_weights")
    assert set_args[2] == 2 and clear_args[1:] == (None, 0)
    _held_to_signature("sisic_unet_set_loss_weights", set_args)


def test_loss_weights_clear_after_an_exception(lib):
    model = Model()
    with pytest.raises(ZeroDivisionError):
        with train._loss_weights(model, torch.ones(2)):
            assert model._loss_weights_set is True
            1 / 0
    assert model._loss_weights_set is False
    assert [a[1:] for _, a in lib.named("sisic_unet_set_loss_weights")][-1] == (None, 0)
    # without weights the block makes no call, unless a leftover has to go
    lib.calls.clear()
    with train._loss_weights(model, None):
        pass
    assert lib.calls == []
    model._loss_weights_set = True
    with train._loss_weights(model, None):
        assert model._loss_weights_set is False
    assert [a[1:] for _, a in lib.calls] == [(None, 0)]
