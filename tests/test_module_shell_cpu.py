"""The handle-owning shell of the two model classes (synt_isic_amd/_module.py) without a GPU: which library symbols a load, a
move, a read and the end of the object call, in which order and with which arguments.  ``_lib.load()`` is replaced by a stand-in
that records every call and answers the tensor directory from the class's own spec; each recorded call is held to
``_lib.SIGNATURES`` (tests/test_train_marshal_cpu.py: the argument count, and every argument convertible by its declared ctypes
type).  Tensors stay on the host: a move to ``cuda`` changes the model's device and nothing else."""
import ctypes as C
import math

import pytest
import torch

import arch_ref
from synt_isic_amd import _lib, ops
from synt_isic_amd.classifier import HipMelanomaClassifier
from synt_isic_amd.unet import HipUNet2DModel
from synt_isic_amd.weights import synthetic_resnet18_state_dict, synthetic_unet_state_dict
from test_train_marshal_cpu import _held_to_signature

CUDA0 = torch.device("cuda", 0)
UNET_CFG = arch_ref.ARCHS["D"]           # one block: the fewest tensors


class Recorder:
    """every attribute is a library function that records (name, args) and returns SISIC_OK; ``*_num_tensors`` and
    ``*_tensor_name`` list ``names``, ``*_create*`` writes a handle through its last argument"""

    def __init__(self, names):
        self.calls, self.names, self.handles = [], list(names), 0

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name.endswith("_num_tensors"):
                return len(self.names)
            if name.endswith("_tensor_name"):
                return self.names[args[1]].encode()
            if "_create" in name:
                self.handles += 1
                args[-1]._obj.value = 0x1000 * self.handles
            return 0
        return fn

    def take(self):
        """the symbols called since the last take, every call held to its signature"""
        calls, self.calls = self.calls, []
        for name, args in calls:
            _held_to_signature(name, args)
        return [name for name, _ in calls]


CASES = {
    "unet": dict(make=lambda: HipUNet2DModel(**arch_ref.unet_kwargs(UNET_CFG)), weights=lambda: synthetic_unet_state_dict(cfg=UNET_CFG),
                 prefix="sisic_unet", create=["sisic_unet_create"], release=["sisic_unet_dropout_next_call", "sisic_unet_destroy"],
                 on_cpu="HipUNet2DModel runs on MI355X only: call .to('cuda') first (there is no CPU path)",
                 no_weights="HipUNet2DModel has no weights: call load_state_dict() first",
                 keys="libsisic_hip.so and synt_isic_amd.arch disagree on the state-dict keys"),
    "classifier": dict(make=lambda: HipMelanomaClassifier(num_classes=7), weights=synthetic_resnet18_state_dict,
                       prefix="sisic_resnet", create=["sisic_resnet_create"], release=["sisic_resnet_destroy"],
                       on_cpu="HipMelanomaClassifier runs on MI355X only: call .to('cuda') first (no CPU path)",
                       no_weights="HipMelanomaClassifier has no weights: call load_state_dict() first",
                       keys="libsisic_hip.so and synt_isic_amd.arch disagree on the classifier keys"),
}


@pytest.fixture(params=list(CASES))
def case(request, monkeypatch):
    """(the case, a model of its class, the recorder that stands in for the library)"""
    c = CASES[request.param]
    model = c["make"]()
    rec = Recorder(model._spec)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(ops, "context", lambda device, *a: C.c_void_p(0x10))
    to = torch.Tensor.to

    def host_to(self, *args, **kwargs):          # no GPU here: a tensor asked to move to cuda stays where it is
        args = tuple("cpu" if isinstance(a, torch.device) and a.type == "cuda" else a for a in args)
        if isinstance(kwargs.get("device"), torch.device) and kwargs["device"].type == "cuda":
            kwargs["device"] = "cpu"
        return to(self, *args, **kwargs)
    monkeypatch.setattr(torch.Tensor, "to", host_to)
    yield c, model, rec
    model._release()                             # while the stand-in is in place: its handles are no library objects


def test_the_library_calls_of_a_load_two_moves_three_reads_and_the_end(case):
    c, model, rec = case
    p, n = c["prefix"], len(model._spec)
    upload = c["create"] + [f"{p}_num_tensors"] + [f"{p}_tensor_name"] * n + [f"{p}_load"]
    model.load_state_dict(c["weights"]())
    assert rec.take() == []                                        # on the CPU: host copies only
    assert model.to(CUDA0) is model and model.device == CUDA0
    calls = list(rec.calls)
    assert rec.take() == upload
    # what the load was given: the spec's names and element counts, in the spec's order
    _, (handle, count, names, ptrs, numels) = calls[-1]
    assert handle.value == 0x1000 and count == n and len(ptrs) == n and all(ptrs)
    assert list(names) == [k.encode() for k in model._spec]
    assert list(numels) == [math.prod(shape) for shape in model._spec.values()]
    assert model.handle.value == 0x1000 and rec.take() == []       # uploaded: the handle costs nothing more
    assert model.to(CUDA0) is model and model.to(None) is model and rec.take() == []
    model.to("cpu")
    assert rec.take() == c["release"] and model.device == torch.device("cpu")
    model.to(CUDA0)
    assert rec.take() == upload and model.handle.value == 0x2000   # a new handle, listed once again
    some = list(model._spec)[::max(1, n // 3)][:3]
    for name in some:
        assert tuple(model.read_tensor(0, name).shape) == tuple(model._spec[name])
    reads = list(rec.calls)
    assert rec.take() == [f"{p}_read"] * 3                         # no listing per access
    assert [a[2] for _, a in reads] == [list(model._spec).index(name) for name in some]
    assert [a[4] for _, a in reads] == [math.prod(model._spec[name]) for name in some]
    model.__del__()
    assert rec.take() == c["release"]
    model.__del__()                                                # nothing left to release
    assert rec.take() == []


def test_the_directory_is_listed_once_per_handle(case):
    c, model, rec = case
    p, n = c["prefix"], len(model._spec)
    model.load_state_dict(c["weights"]())
    model.to(CUDA0)
    model._read_all(0)
    model.read_tensor(0, next(iter(model._spec)))
    model.load_state_dict(c["weights"]())                          # a reload keeps the handle and its directory
    model._read_all(0)
    names = rec.take()
    assert names.count(f"{p}_tensor_name") == n and names.count(f"{p}_num_tensors") == 1
    assert names.count(f"{p}_load") == 2 and names.count(f"{p}_read") == 2 * n + 1
    assert sum(name in c["create"] for name in names) == 1


def test_the_handle_refusals_and_the_key_disagreement_keep_their_words(case):
    c, model, rec = case

    def said(call):
        with pytest.raises(RuntimeError) as e:
            call()
        return str(e.value)
    assert said(lambda: model.handle) == c["on_cpu"]               # no weights either: the device is asked first
    model.load_state_dict(c["weights"]())
    assert said(lambda: model.handle) == c["on_cpu"]
    bare = c["make"]().to(CUDA0)
    assert said(lambda: bare.handle) == c["no_weights"]
    assert rec.take() == []
    rec.names[-1] = "not.a.key"
    assert said(lambda: model.to(CUDA0)) == c["keys"]
    assert f"{c['prefix']}_load" not in rec.take()
