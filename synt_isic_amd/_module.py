"""HipModule -- what HipUNet2DModel and HipMelanomaClassifier share: a library handle and the named fp32 tensors behind it.

The shell owns the host copies (``_params``, on ``_device``), the handle and its life (created on the first upload, destroyed on
a move or with the object), the upload (``<prefix>_load``: refused whole or taken whole, the handle is never half loaded), the
name -> index table of the handle (listed once per handle) and every tensor read and write.  A subclass names its symbols
(``_PREFIX``), creates its handle (``_create_handle``), and says what follows an upload (``_after_upload``), what precedes a
release (``_before_release``) and which host copies an optimizer step leaves stale (``_stale_names``)."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Iterable, Optional

import torch

from . import _lib
from ._lib import check


class HipModule:
    _PREFIX = ""              # "sisic_unet" / "sisic_resnet": <prefix>_load, _destroy, _read, _write, _num_tensors, _tensor_name
    _NAME = ""                # the class as its refusals name it
    _NO_CPU_PATH = ""         # ... and how they say that there is no CPU path
    _KEYS = ""                # ... and what the library and arch.py disagree on

    def __init__(self, spec: "OrderedDict[str, tuple]"):
        self._spec = spec
        self._params: "OrderedDict[str, torch.Tensor]" = OrderedDict()   # on self._device
        self._device = torch.device("cpu")
        self._handle: Optional[C.c_void_p] = None
        self._index: Optional[Dict[str, int]] = None     # name -> index of the handle's tensors; dropped with the handle
        self._uploaded = False
        self._params_stale = False    # the library's weights have moved on (optimizer steps) since _params was read

    # ---- what a subclass supplies ---------------------------------------------------------------
    def _create_handle(self) -> None:
        """create the library object on ``_device`` into ``self._handle`` and bring it to the model's settings"""
        raise NotImplementedError

    def _after_upload(self) -> None:
        pass

    def _before_release(self) -> None:
        pass

    def _stale_names(self) -> Iterable[str]:
        return self._spec

    # ---- device ---------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self._device

    def to(self, device=None, *args, **kwargs):
        if device is None:
            return self
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        self._refresh_params()
        self._release()
        self._params = OrderedDict((k, v.to(device)) for k, v in self._params.items())
        self._device = device
        if device.type == "cuda" and self._params:
            self._upload()
        return self

    def cuda(self, index: Optional[int] = None):
        return self.to(torch.device("cuda", index if index is not None else torch.cuda.current_device()))

    def cpu(self):
        return self.to("cpu")

    # ---- library handle -------------------------------------------------------------------------
    def _fn(self, name: str):
        return getattr(_lib.load(), f"{self._PREFIX}_{name}")

    def _list_tensors(self, h) -> Dict[str, int]:
        name = self._fn("tensor_name")
        return {name(h, i).decode(): i for i in range(self._fn("num_tensors")(h))}

    def _set_params(self, new: "OrderedDict[str, torch.Tensor]") -> None:
        """the end of a load_state_dict: new host copies, uploaded at once on the GPU"""
        self._params = new
        self._uploaded = False
        self._params_stale = False
        if self._device.type == "cuda":
            self._upload()

    def _upload(self) -> None:
        if self._handle is None:
            self._create_handle()
            self._index = self._list_tensors(self._handle)
            if sorted(self._index) != sorted(self._spec):     # the library's own view of the expected keys must agree with ours
                raise RuntimeError(f"libsisic_hip.so and synt_isic_amd.arch disagree on the {self._KEYS}")
        host = [(k, v.detach().to("cpu", torch.float32).contiguous()) for k, v in self._params.items()]
        n = len(host)
        names = (C.c_char_p * n)(*[k.encode() for k, _ in host])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for _, t in host])
        numels = (C.c_int64 * n)(*[t.numel() for _, t in host])
        check(self._fn("load")(self._handle, n, names, ptrs, numels))
        self._uploaded = True
        self._after_upload()

    def _release(self) -> None:
        self._before_release()
        if self._handle is not None:
            self._fn("destroy")(self._handle)
            self._handle = self._index = None
            self._uploaded = False

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        if self.device.type != "cuda":
            raise RuntimeError(f"{self._NAME} runs on MI355X only: call .to('cuda') first ({self._NO_CPU_PATH})")
        if not self._params:
            raise RuntimeError(f"{self._NAME} has no weights: call load_state_dict() first")
        if not self._uploaded:
            self._upload()
        return self._handle

    # ---- tensors --------------------------------------------------------------------------------
    def _tensor_index(self) -> Dict[str, int]:
        h = self.handle
        if self._index is None:
            self._index = self._list_tensors(h)
        return self._index

    def _refresh_params(self) -> None:
        """after optimizer steps: read the current weights back from the library"""
        if not self._params_stale or self._handle is None:
            return
        for name in self._stale_names():
            self._params[name] = self.read_tensor(0, name).to(self._device)
        self._params_stale = False

    _sync_params = _refresh_params

    def read_tensor(self, what: int, name: str) -> torch.Tensor:
        """one tensor of the library's arenas on the CPU (<prefix>_read): what = 0 parameter, 1 gradient, 2 / 3 Adam m / v"""
        out = torch.empty(tuple(self._spec[name]), dtype=torch.float32)
        check(self._fn("read")(self.handle, int(what), self._tensor_index()[name], C.cast(out.data_ptr(), _lib.c_float_p),
                               out.numel()))
        return out

    def write_tensor(self, what: int, name: str, value: torch.Tensor) -> None:
        """the counterpart (<prefix>_write): gradients and moments only, parameters are set by load_state_dict"""
        v = value.detach().to("cpu", torch.float32).contiguous()
        if tuple(v.shape) != tuple(self._spec[name]):
            raise ValueError(f"{name}: shape {tuple(v.shape)}, expected {tuple(self._spec[name])}")
        check(self._fn("write")(self.handle, int(what), self._tensor_index()[name], C.cast(v.data_ptr(), _lib.c_float_p),
                                v.numel()))

    def _read_all(self, what: int) -> "OrderedDict[str, torch.Tensor]":
        self.handle                       # (a model without one refuses here, whatever its spec)
        return OrderedDict((name, self.read_tensor(what, name)) for name in self._spec)

    def _write_all(self, what: int, mapping: Dict[str, torch.Tensor], label: str) -> None:
        """{name: tensor} into one of the library's training arenas: 1 gradient, 2 / 3 Adam moments, 4 EMA"""
        self.handle
        for name, t in mapping.items():
            if name not in self._spec:
                raise KeyError(f"{label}: no parameter named {name}")
            if tuple(t.shape) != tuple(self._spec[name]):
                raise RuntimeError(f"{label}: size mismatch for {name}: {tuple(t.shape)} vs {tuple(self._spec[name])}")
            self.write_tensor(what, name, t)
