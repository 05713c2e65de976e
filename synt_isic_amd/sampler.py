"""The T-step reverse-diffusion sampler: ``generate(seed, class_name, T)``.

Product-side equivalent of ``ImageGenerator.generate_single_image``
(core/generator/image_generator.py:308-500): seed policy (:586-592, :626-637),
initial noise and ``noise_hash`` (:369-389), the loop (:395-403) -- executed by
``sisic_sample`` in libsisic_hip.so without returning to Python between steps --
trajectory capture (:406-407) and de-normalisation to uint8 HWC (:441-447).

Noise contract (a defined extension): image b owns one CPU
``torch.Generator().manual_seed(seed_b)``; ``x_T[b]`` is drawn first, then ``z_t[b]``
for every step with t > 0 in loop order.  Results are independent of the batch an
image is sampled in and of how images are sharded over GPUs.

``scheduler="ddim"`` (``"ddpm"`` is the default) runs the same loop under the DDIM rule (``HipDDIMScheduler``; ``eta``,
``use_clipped_model_output``): the same x_T and ``noise_hash`` for a seed in either noise mode, and the same contract for z
-- only the steps whose sigma is not zero consume a ``z_t[b]``, in loop order.  Under DDPM those are the steps with t > 0;
under DDIM at eta = 0 there are none: nothing is drawn, no noise buffer exists and no worker thread runs.  (diffusers'
DDIMScheduler draws a z on every step at eta > 0, also where it multiplies it by a sigma of 0.)

``scheduler="dpmsolver++"`` runs the loop under DPM-Solver++(2M) (``HipDPMSolverMultistepScheduler``; ``solver_order``,
``algorithm_type``), the rule for 10 to 25 steps.  The same x_T, ``noise_hash`` and z contract again: the ODE variant draws
nothing beyond x_T, the SDE variant (``"sde-dpmsolver++"``) one ``z_t[b]`` for every step but the last.  The rule keeps the
previous step's x0, and a run cut into several library calls would lose it at every cut, so a host-noise SDE run draws all
its z first (``draw_noise``: T is small under this rule) and runs in one call instead of streaming segments.

``noise="device"`` (off by default) is a second contract with the same independence: ``x_T[b]`` from torch's device
generator seeded with ``seed_b`` (the reference's own spelling on a GPU, so its ``noise_hash``), and every ``z_t[b]``
generated inside the scheduler-step kernel by Philox4x32-10 keyed with ``seed_b``: no host RNG,
no noise buffer, no upload.  The two modes give different images for one seed.

Image editing (``init_image``, ``mask``, ``strength``, ``jump_length``, ``n_resample``): image-to-image starts the loop from
``add_noise(init_image, x_T, t)`` at an intermediate level of the grid (SDEdit) and changes nothing else; inpainting
(RePaint) additionally re-imposes the known region of ``init_image`` in every step, inside the step kernel, at that step's
noise level, optionally with the paper's resampling jumps (``scheduler.resample_schedule``).  x_T and ``noise_hash`` of a
seed are those of a plain run.  Inpainting draws on the device only (``noise="device"``): the known region's noise and the
jumps are two more streams of the device-noise contract (tags 5 and 6).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .scheduler import MIRRORS, check_dpmpp_options, check_thresholding, edit_rows, resample_schedule      # noqa: F401
from .unet import HipUNet2DModel

ISIC_CLASSES = ("MEL", "NV", "BCC", "AKIEC", "BKL", "DF", "VASC")   # xai/XAI.py:196


def class_seed_offset(class_name: str) -> int:
    """image_generator.py:586-592 -- 31-bit md5 offset per class."""
    h = hashlib.md5(class_name.encode("utf-8")).hexdigest()
    return int(h[:8], 16) & 0x7FFFFFFF


def image_seed(base_seed: int, class_name: str, index: int) -> int:
    """image_generator.py:626-631."""
    return (int(base_seed) + class_seed_offset(class_name) + int(index)) & 0x7FFFFFFF


def noise_hash(x_T: torch.Tensor) -> str:
    """image_generator.py:383-389 -- sha256 of the fp32 bytes of x_T, first 16 hex digits."""
    return hashlib.sha256(x_T.detach().to("cpu").contiguous().numpy().tobytes()).hexdigest()[:16]


def draw_noise(seeds: Sequence[int], n_noise_steps: int, chw: Tuple[int, int, int],
               pin: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host noise per the contract above: x_T [B,C,H,W] and z [n_noise_steps,B,C,H,W]."""
    B = len(seeds)
    x_T = torch.empty((B,) + tuple(chw), dtype=torch.float32)
    z = torch.empty((n_noise_steps, B) + tuple(chw), dtype=torch.float32, pin_memory=pin)
    for b, s in enumerate(seeds):
        g = torch.Generator(device="cpu")
        g.manual_seed(int(s))
        x_T[b] = torch.randn((1,) + tuple(chw), generator=g)[0]
        if n_noise_steps:
            # one draw of n*numel values == n consecutive draws of numel (numel is a multiple of 16)
            z[:, b] = torch.randn((n_noise_steps,) + tuple(chw), generator=g)
    return x_T, z


NOISE_MODES = ("host", "device")


def _check_noise_mode(noise: str) -> str:
    if noise not in NOISE_MODES:
        raise ValueError(f"noise must be one of {NOISE_MODES}, got {noise!r}")
    return noise


SCHEDULERS = tuple(_lib.RULES)


def _check_scheduler(scheduler: str, eta: float, use_clipped_model_output: bool = False, solver_order: int = 2,
                     algorithm_type: str = "dpmsolver++") -> str:
    mirror = MIRRORS.get(scheduler) if isinstance(scheduler, str) else None
    if mirror is None:
        raise ValueError(f"scheduler must be one of {SCHEDULERS}, got {scheduler!r}")
    if not mirror._takes_eta and (float(eta) != 0.0 or use_clipped_model_output):
        raise ValueError("eta and use_clipped_model_output belong to scheduler='ddim'; the DDPM and DPM-Solver++ rules have "
                         "neither")
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must lie in 0 .. 1, got {eta!r}")
    if mirror._takes_solver_options:
        try:
            check_dpmpp_options(solver_order, algorithm_type)
        except NotImplementedError as e:
            raise ValueError(str(e)) from None
    elif solver_order != 2 or algorithm_type != "dpmsolver++":
        raise ValueError("solver_order and algorithm_type belong to scheduler='dpmsolver++'")
    return scheduler


def _rule_tables(scheduler, eta: float, use_clipped_model_output: bool):
    """(host [T, row width] coefficient table, SISIC_RULE_* id, rule flags) of a scheduler mirror (its ``rule_table``), with the
    refusals of eta and use_clipped_model_output under a rule that has neither.  Sigma is column 4 under every rule.  A
    DPM-Solver++ mirror carries its own solver_order and algorithm_type."""
    _check_scheduler(scheduler.rule, eta, use_clipped_model_output)
    rule, table, flags = scheduler.rule_table(eta, use_clipped_model_output)
    return table, rule.id, flags


@dataclass(frozen=True)
class DeviceNoise:
    """Per-step noise generated inside the scheduler-step kernel (``sisic_sample_frames_rng``): image b of the batch draws
    with ``seeds[b]``, step i of the loop with step index ``step0 + i`` (a run cut into several calls passes its offset)."""
    seeds: Tuple[int, ...]
    step0: int = 0

    def __post_init__(self):
        object.__setattr__(self, "seeds", tuple(int(s) for s in self.seeds))
        if any(s < 0 or s >> 64 for s in self.seeds):
            raise ValueError("seeds must be integers in 0 .. 2**64-1")


@dataclass(frozen=True)
class Guidance:
    """What a class-conditional model's loop needs beside the latents (``sisic_sample_frames_cond``): one label per image,
    the null label of classifier-free guidance and the guidance scale.  Scale 1 is plain conditional sampling, one UNet pass
    per step; any other scale runs each step once at twice the batch and steps on ``eps_u + scale * (eps_c - eps_u)``."""
    labels: Tuple[int, ...]
    null_label: int
    scale: float = 1.0

    def __post_init__(self):
        object.__setattr__(self, "labels", tuple(int(v) for v in self.labels))
        object.__setattr__(self, "scale", check_guidance_scale(self.scale))


@dataclass(frozen=True)
class ClassifierGuidance:
    """What a classifier-guided run needs beside the latents (``sisic_sample_frames_clf``): the classifier, image b's target
    output and the scale.  Every step then applies its rule to ``eps - (scale * sqrt(1 - abar_t)) * g``, ``g`` the classifier's
    input gradient of ``log(softmax(clf(x_t))[target_b] + 1e-8)`` at the step's latent.  Scale 0 gives the unguided bits."""
    classifier: object
    targets: Tuple[int, ...]
    scale: float = 1.0

    def __post_init__(self):
        object.__setattr__(self, "targets", tuple(int(v) for v in self.targets))
        object.__setattr__(self, "scale", _finite_number("classifier_scale", self.scale))


@dataclass(frozen=True)
class Edit:
    """What an inpainting run needs beside the latents (``sisic_sample_frames_edit``): the known image (GPU fp32 [B,C,H,W] in
    [-1, 1], finite everywhere), the mask (GPU fp32 [B,1,H,W]; 1 keeps the known pixel, 0 synthesises, values in between
    blend) and the schedule of UNet passes, ``(index into scheduler.timesteps, jump)`` per pass
    (``scheduler.resample_schedule``); None is the plain grid, every entry once and no jump."""
    image: torch.Tensor
    mask: torch.Tensor
    schedule: Optional[Sequence[Tuple[int, int]]] = None


MAX_CALL_STEPS = 1000        # steps of one library call of the loop (include/sisic.h)


def _finite_number(name: str, value) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not np.isfinite(value):
        raise ValueError(f"{name} must be a finite number, got {value!r}")
    return float(value)


def check_guidance_scale(guidance_scale) -> float:
    """a finite real number (negative scales are legal: they push away from the class)"""
    return _finite_number("guidance_scale", guidance_scale)


def _check_guidance(model: HipUNet2DModel, guidance: Optional[Guidance], B: int) -> None:
    n = model.config.num_class_embeds
    if n is None:
        if guidance is not None:
            raise ValueError("class labels and guidance need a class-conditional model (num_class_embeds)")
        return
    if guidance is None:
        raise ValueError("a class-conditional model samples under labels: pass guidance=Guidance(labels, null_label, scale)")
    if len(guidance.labels) != B:
        raise ValueError(f"{len(guidance.labels)} class labels for a batch of {B}")
    for v in guidance.labels + (guidance.null_label,):
        if not 0 <= int(v) < n:
            raise ValueError(f"class label {v} is outside [0, {n})")


def draw_x_T_device(seeds: Sequence[int], chw: Tuple[int, int, int], device: torch.device) -> torch.Tensor:
    """x_T [B,C,H,W] on ``device``, image by image from ``torch.Generator(device=device).manual_seed(seed_b)``: the
    reference's spelling (image_generator.py:369-381), so ``noise_hash`` is what it records for that seed on that device."""
    rows = []
    for s in seeds:
        g = torch.Generator(device=device)
        g.manual_seed(int(s))
        rows.append(torch.randn((1,) + tuple(chw), device=device, generator=g))
    return torch.cat(rows, dim=0)


class NoiseStream:
    """The same noise as ``draw_noise``, produced while the GPU samples.

    ``draw_noise`` materialises every z_t first: 786 M normals (3.1 GB) for 64 images at 64x64, T=1000 -- seconds of
    single-threaded RNG in front of an 8 s sampling run.  Here the per-image generators are advanced on worker
    threads, one segment of steps at a time, into two pinned buffers that are uploaded on a side stream; the sampler
    consumes segment k while segment k+1 is drawn.  One big ``randn`` of n*numel values equals n consecutive draws of
    numel values (numel is a multiple of 16), and each generator is only ever advanced by one task at a time, so the
    stream is bit-identical to ``draw_noise`` whatever the segment length or worker count.
    """

    def __init__(self, seeds: Sequence[int], chw: Tuple[int, int, int], device: torch.device, segment_steps: int,
                 workers: Optional[int] = None, buffer_cache: Optional[dict] = None):
        self.chw = tuple(chw)
        self.B = len(seeds)
        self.device = device
        self.seg = max(1, int(segment_steps))
        # a caller that samples repeatedly (Sampler) keeps the worker pool, the copy stream and the staging buffers in
        # ``buffer_cache`` between calls: creating them costs milliseconds, a one-image T=50 run is ~110 ms
        self._own_pool = True
        if buffer_cache is not None and workers is None and "pool" in buffer_cache:
            self.pool = buffer_cache["pool"]
            self._own_pool = False
        else:
            if workers is None:
                try:
                    cpus = len(os.sched_getaffinity(0))
                except AttributeError:                      # pragma: no cover
                    cpus = os.cpu_count() or 1
                n_workers = max(1, min(cpus, 16))
            else:
                n_workers = max(1, int(workers))
            self.pool = ThreadPoolExecutor(max_workers=n_workers)
            if buffer_cache is not None and workers is None:
                buffer_cache["pool"] = self.pool
                self._own_pool = False
        self.gens = []
        for sd in seeds:
            g = torch.Generator(device="cpu")
            g.manual_seed(int(sd))
            self.gens.append(g)
        self.x_T = torch.empty((self.B,) + self.chw, dtype=torch.float32)
        list(self.pool.map(self._draw_x, range(self.B)))
        shape = (self.seg, self.B) + self.chw
        # pinning ~100 MB costs tens of milliseconds: a caller that samples repeatedly (Sampler) passes a dict in which
        # the two pinned and two device buffers of a shape are kept between calls
        key = (shape, str(device))
        if buffer_cache is not None and buffer_cache.get("shape") == key:
            self.host, self.dev = buffer_cache["buffers"]
        else:
            self.host = [torch.empty(shape, dtype=torch.float32, pin_memory=True) for _ in range(2)]
            self.dev = [ops.empty(shape, dtype=torch.float32, device=device) for _ in range(2)]
            if buffer_cache is not None:                # one shape at a time: bounded memory
                buffer_cache["shape"], buffer_cache["buffers"] = key, (self.host, self.dev)
        if buffer_cache is not None and buffer_cache.get("copy_stream_device") == str(device):
            self.copy_stream = buffer_cache["copy_stream"]
        else:
            self.copy_stream = torch.cuda.Stream(device)
            if buffer_cache is not None:
                buffer_cache["copy_stream"], buffer_cache["copy_stream_device"] = self.copy_stream, str(device)
        # uploads of less than 8 MB per segment (a few images) go on the sampling stream itself
        self.same_stream = (os.environ.get("SISIC_NOISE_SAME_STREAM", "1") != "0") and self.seg * self.B * int(np.prod(self.chw)) * 4 <= (8 << 20)
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]      # upload of slot i finished
        self.uploaded = [False, False]
        self.consumed = [None, None]                               # event after the sampler's last read of slot i
        self.pending = [None, None]

    def _draw_x(self, b: int) -> None:
        self.x_T[b] = torch.randn((1,) + self.chw, generator=self.gens[b])[0]

    def _draw_z(self, slot: int, n: int, b: int) -> None:
        # numpy copies on this worker thread alone: a torch copy of this size starts an intra-op thread team from every worker
        # at once (workers x intra-op threads), which on a host with a CPU quota spins the quota away
        self.host[slot][:n, b].numpy()[...] = torch.randn((n,) + self.chw, generator=self.gens[b]).numpy()

    def prefetch(self, slot: int, n: int) -> None:
        """start drawing the next n noise tensors of every image into pinned buffer ``slot``"""
        if n <= 0:
            self.pending[slot] = []
            return
        if self.uploaded[slot]:
            self.ready[slot].synchronize()           # the previous upload out of this pinned buffer has completed
        self.pending[slot] = [self.pool.submit(self._draw_z, slot, n, b) for b in range(self.B)]

    def acquire(self, slot: int, n: int) -> Optional[torch.Tensor]:
        """wait for the draws of ``slot``, upload them on the side stream and make the current stream wait"""
        if n <= 0:
            return None
        for f in self.pending[slot]:
            f.result()
        cur = torch.cuda.current_stream(self.device)
        if self.same_stream:
            # small runs (one image): the upload rides the sampling stream itself -- stream order replaces the two events
            self.dev[slot][:n].copy_(self.host[slot][:n], non_blocking=True)
            self.ready[slot].record(cur)
            self.uploaded[slot] = True
            return self.dev[slot][:n]
        with torch.cuda.stream(self.copy_stream):
            if self.consumed[slot] is not None:
                self.copy_stream.wait_event(self.consumed[slot])
            self.dev[slot][:n].copy_(self.host[slot][:n], non_blocking=True)
            self.ready[slot].record(self.copy_stream)
            self.uploaded[slot] = True
        cur.wait_event(self.ready[slot])
        return self.dev[slot][:n]

    def release(self, slot: int) -> None:
        """the sampler's reads of ``slot`` are enqueued on the current stream"""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.consumed[slot] = ev

    def close(self) -> None:
        if self._own_pool:
            self.pool.shutdown(wait=True)
        else:                                            # a shared pool: wait for this run's draws only
            for tasks in self.pending:
                for f in tasks or []:
                    f.result()
            for slot in range(2):                        # ... and for the uploads out of the shared pinned buffers
                if self.uploaded[slot]:
                    self.ready[slot].synchronize()


def trajectory_save_indices(timesteps: Sequence[int], save_every: int) -> List[int]:
    """Which steps of a run the XAI trajectory keeps (xai/XAI.py:751-777 `save_indices`, :815-822): every
    ``save_every``-th step by index and always the last one; when ``save_every`` is not smaller than the number of steps
    it is read as a stride in t instead: the steps nearest to t = 0, max(t) and the multiples of ``save_every`` up to 1000,
    and every step whose own t is such a multiple (or 0).  Sorted step indices."""
    ts = [int(float(t)) for t in timesteps]
    n = len(ts)
    every = int(save_every)
    if every <= 0:
        raise ValueError("save_every must be positive")
    keep = set(range(0, n, every))
    if n:
        keep.add(n - 1)
    if every >= n and n:
        want = {0, max(ts)} | set(range(0, 1001, every))
        for dt in want:
            keep.add(min(range(n), key=lambda i: abs(ts[i] - dt)))
        keep |= {i for i, t in enumerate(ts) if t % every == 0 or t == 0}
    return sorted(keep)


@dataclass
class SampleResult:
    images: torch.Tensor                       # uint8 [B,H,W,3] on the GPU
    latents: torch.Tensor                      # fp32 [B,3,H,W] final x_0 on the GPU
    trajectory: Optional[torch.Tensor] = None  # fp32 [n_kept,B,3,H,W] on the GPU: x after the steps of trajectory_steps
    trajectory_steps: List[int] = field(default_factory=list)   # step indices of the kept frames (all T without a stride)
    seeds: List[int] = field(default_factory=list)
    noise_hashes: List[str] = field(default_factory=list)
    timesteps: List[int] = field(default_factory=list)
    steps_done: int = 0
    cancelled: bool = False                    # the stop flag ended the loop early: images/latents are NOT a result
    scheduler: str = "ddpm"                    # the step rule of the run ...
    eta: float = 0.0                           # ... and its eta (DDIM; 0.0 under DDPM)
    strength: float = 1.0                      # image-to-image / inpainting: the part of the grid the run went through
    n_resample: int = 1                        # inpainting: RePaint's resampling count (1: no jumps)
    unet_passes: int = 0                       # UNet passes of the whole run (the grid's steps plus the resampled ones)
    prediction_type: str = "epsilon"           # what the model's output meant to the step rule (the model's own property)
    classifier_scale: Optional[float] = None   # classifier guidance: its scale (None: the run had none) ...
    classifier_passes: int = 0                 # ... and the classifier's gradient walks, one per UNet pass
    thresholding: Optional[Tuple[float, float]] = None   # dynamic thresholding of x0: (ratio, sample_max_value), or None


def _frame_rows(T: int, return_trajectory: bool, save_indices: Optional[Sequence[int]]):
    """(kept step indices, host int32 [T] row table or None) for sisic_sample_frames"""
    if not return_trajectory:
        return [], None
    if save_indices is None:
        return list(range(T)), None
    kept = sorted({int(i) for i in save_indices})
    if kept and (kept[0] < 0 or kept[-1] >= T):
        raise ValueError(f"save_indices outside 0..{T - 1}")
    rows = np.full((T,), -1, dtype=np.int32)
    rows[kept] = np.arange(len(kept), dtype=np.int32)
    return kept, rows


@torch.no_grad()
def run_sampling_loop(model: HipUNet2DModel, scheduler, x_T: torch.Tensor, noise, *, thresholding: Optional[bool] = None,
                      dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, **kwargs) -> SampleResult:
    """``_run_sampling_loop`` (whose keyword arguments these are) under dynamic thresholding of x0:
    ``thresholding`` True with its two published companions, False, or None (the default) for what the scheduler object was
    set to (its constructor or ``set_thresholding``).  The model's handle is set from them on EVERY call, on or off, so no
    setting outlives the call that made it; under thresholding the scheduler's ``clip_sample`` is not read.  ``SampleResult.thresholding`` records (ratio, max) or
    None."""
    if thresholding is None:
        threshold = getattr(scheduler, "threshold", None)
    else:
        threshold = check_thresholding(thresholding, dynamic_thresholding_ratio, sample_max_value)
    if threshold is not None and x_T[0].numel() > ops.THRESHOLD_MAX_PER_IMAGE:
        raise ValueError(f"thresholding takes images of at most 2**24 elements, these have {x_T[0].numel()}")
    res = _run_sampling_loop(model, scheduler, x_T, noise, threshold=threshold, **kwargs)
    res.thresholding = threshold
    return res


def _set_thresholding(lib, model: HipUNet2DModel, threshold) -> None:
    """the handle's thresholding setting of the call about to run: (ratio, max), or off"""
    ratio, max_value = threshold if threshold is not None else (0.0, 1.0)
    check(lib.sisic_unet_set_thresholding(model.handle, ratio, max_value))


def _check_classifier_guidance(model: HipUNet2DModel, classifier: ClassifierGuidance, noise, guidance, edit, B: int) -> None:
    """every refusal of a classifier-guided run that needs no library call (the library checks them again)"""
    if guidance is not None or model.config.num_class_embeds is not None:
        raise ValueError("classifier guidance steers an unconditional model: it does not compose with a class-conditional "
                         "model or guidance_scale (classifier-free guidance)")
    if edit is not None:
        raise ValueError("classifier guidance does not compose with init_image / mask (image-to-image, inpainting)")
    if getattr(model, "prediction_type", "epsilon") != "epsilon":
        raise ValueError(f"classifier guidance takes epsilon-prediction models only; this model's prediction_type is "
                         f"{model.prediction_type!r}")
    if not isinstance(noise, DeviceNoise):
        raise ValueError('classifier guidance requires noise="device" (a DeviceNoise): the guided step kernels draw their noise')
    if len(classifier.targets) != B:
        raise ValueError(f"{len(classifier.targets)} classifier targets for a batch of {B}")
    n = int(classifier.classifier.num_classes)
    for v in classifier.targets:
        if not 0 <= v < n:
            raise ValueError(f"classifier target {v} is outside [0, {n})")


def check_edit_schedule(rule: str, schedule, T: int) -> List[Tuple[int, int]]:
    """the schedule of an edited run as a list of (grid index, jump); None: the plain grid.  Jumps belong to ddpm and ddim: a
    jump invalidates the history DPM-Solver++ keeps."""
    if schedule is None:
        return [(i, 0) for i in range(T)]
    sched = [(int(i), int(j)) for i, j in schedule]
    if not sched:
        raise ValueError("an empty edit schedule")
    if rule == "dpmsolver++" and (any(j for _, j in sched) or [i for i, _ in sched] != list(range(T))):
        raise ValueError("resampling (n_resample > 1) is offered under scheduler='ddpm' and 'ddim': a jump invalidates the "
                         "history of DPM-Solver++, which takes a mask with n_resample=1 only")
    return sched


def segment_bounds(T: int, seg: int, per_step: int) -> List[int]:
    """Step boundaries of the segments a streamed run is cut into (``NoiseStream``): ``seg`` steps each, except that a run
    whose segment is a noticeable amount of RNG (more than 1 M normals: one 128x128 image draws 3 M per 64 steps, 64 images
    at 64x64 draw 50 M) starts with 4, 8, 16, ... steps, so that the GPU starts after a millisecond or two instead of a
    whole segment's worth.  The draws do not depend on the segmentation.  (Round 2 kept one 128x128 image in ONE segment
    because every extra ``sisic_sample`` call cost ~20 ms: a segment of another length re-allocated the per-step tables,
    which rebuilt the captured graph, and every call ran its first step eagerly.  The tables now have a fixed size and a
    call that finds its graph replays from step 0, so an extra segment costs its launches only.)"""
    ramp_min = int(os.environ.get("SISIC_NOISE_RAMP_MIN", "1000000"))
    bounds, n = [0], (4 if per_step * seg > ramp_min else seg)
    while bounds[-1] < T:
        bounds.append(min(T, bounds[-1] + min(n, seg)))
        n *= 2
    return bounds


@dataclass(frozen=True)
class PlannedCall:
    """One library call of a run (``plan_calls``)."""
    k: int                         # its place in the plan
    a: int                         # the steps [a, b) of the run it takes
    b: int
    z_first: int                   # the run's noise rows [z_first, z_first + z_rows): one per step whose sigma is not zero
    z_rows: int
    rows: Optional[np.ndarray]     # its slice of the run's frame-row table (int32 [b - a]; -1: not kept); None: no trajectory
    step0: int                     # device noise: the step index of its first step
    last: bool                     # the one call that writes the images


def plan_calls(noisy: Sequence[bool], cuts: Sequence[int], kept: Sequence[int], step0: int = 0) -> List[PlannedCall]:
    """The library calls of a run, as data: ``noisy[i]`` says whether step i adds noise, ``cuts`` are the step boundaries of the
    calls (``[0, T]``: one call; ``segment_bounds`` for a ``NoiseStream``; every ``max_call_steps`` passes of an edited run),
    ``kept`` the steps whose frame the trajectory keeps (none: no trajectory) and ``step0`` the step index of step 0."""
    T, cuts = len(noisy), [int(c) for c in cuts]
    if len(cuts) < 2 or cuts[0] != 0 or cuts[-1] != T or any(b <= a for a, b in zip(cuts[:-1], cuts[1:])):
        raise ValueError(f"the calls {cuts} do not tile the {T} steps of the run")
    kept, rows = _frame_rows(T, True, kept)         # (a cut run's steps go to their rows of the whole run)
    before = [0]
    for flag in noisy:
        before.append(before[-1] + bool(flag))
    return [PlannedCall(k, a, b, before[a], before[b] - before[a], np.ascontiguousarray(rows[a:b]) if kept else None,
                        int(step0) + a, b == T) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]


class _NoiseSource:
    """Where the calls of a run take their z from.  ``seeds``: the seed array of a run whose step kernel draws (else None);
    ``start`` sees the plan before the first call, ``z_ptr`` gives a call's noise rows in device memory (None: it has none) and
    ``enqueued`` follows the call.  This one adds no noise."""
    seeds = None

    def start(self, plan: List[PlannedCall]) -> None:
        pass

    def z_ptr(self, call: PlannedCall) -> Optional[int]:
        return None

    def enqueued(self, call: PlannedCall) -> None:
        pass


class _BufferNoise(_NoiseSource):
    """a resident buffer [n_noise,B,C,H,W]"""

    def __init__(self, z: torch.Tensor):
        self.z = z

    def z_ptr(self, call):
        return self.z[call.z_first:].data_ptr() if call.z_rows else None


class _SeedNoise(_NoiseSource):
    """a ``DeviceNoise``: the step kernel draws, no buffer"""

    def __init__(self, seeds: Sequence[int]):
        self.seeds = (C.c_uint64 * len(seeds))(*seeds)


class _StreamNoise(_NoiseSource):
    """a ``NoiseStream``: call k reads slot k & 1 while the stream draws call k + 1's rows into the other slot"""

    def __init__(self, ns: NoiseStream):
        self.ns = ns

    def start(self, plan):
        self.plan = plan
        self.ns.prefetch(0, plan[0].z_rows)

    def z_ptr(self, call):
        z = self.ns.acquire(call.k & 1, call.z_rows)
        if call.k + 1 < len(self.plan):
            self.ns.prefetch((call.k & 1) ^ 1, self.plan[call.k + 1].z_rows)    # drawn while the GPU runs this call
        return z.data_ptr() if z is not None else None

    def enqueued(self, call):
        self.ns.release(call.k & 1)


def _library_call(lib, model: HipUNet2DModel, x: torch.Tensor, tables, clip: float, rule: int, rule_flags: int, call: PlannedCall,
                  z_ptr, seeds, guidance: Optional[Guidance], edit: Optional[Edit], classifier: Optional[ClassifierGuidance],
                  traj, out_u8, cancel_flag, stream) -> Tuple[int, int]:
    """(return code, steps done) of one library call of the loop, through the entry point of its kind of run: _clf under a
    ``ClassifierGuidance``, _edit under an ``Edit``, _cond under labels, else _rule_rng with seeds and _rule without.
    tables: the run's (timesteps, coefficient rows, edit rows or None) on the host; the call takes its steps' rows."""
    B, _, H, W = x.shape
    ts, coef, erows = (t[call.a:call.b].contiguous() if t is not None else None for t in tables)
    done = C.c_int(0)
    head = (model.handle, x.data_ptr(), B, H, W, call.b - call.a, C.cast(ts.data_ptr(), _lib.c_int64_p),
            C.cast(coef.data_ptr(), _lib.c_float_p), float(clip), rule, rule_flags)
    tail = (traj.data_ptr() if call.rows is not None else None,
            call.rows.ctypes.data_as(C.POINTER(C.c_int)) if call.rows is not None else None,
            out_u8.data_ptr() if call.last else None,
            C.byref(cancel_flag) if cancel_flag is not None else None, C.byref(done), stream)
    step0 = call.step0 if seeds is not None else 0
    if classifier is not None:
        a = _lib.SampleClfArgs(x=head[1], timesteps=head[6], coef=head[7], noise=None, seeds=seeds,
                               classifier=classifier.classifier.handle, targets=(C.c_int64 * B)(*classifier.targets),
                               traj=tail[0], traj_row=tail[1], out_u8=tail[2],
                               cancel=C.pointer(cancel_flag) if cancel_flag is not None else None, stream=stream,
                               B=B, H=H, W=W, T=head[5], rule=rule, rule_flags=rule_flags, step0=step0, clip=float(clip),
                               scale=classifier.scale)
        return lib.sisic_sample_frames_clf(model.handle, C.byref(a)), a.steps_done
    cond = (None, 0, 1.0)
    if guidance is not None:
        cond = ((C.c_int64 * B)(*guidance.labels), int(guidance.null_label), float(guidance.scale))
    if edit is not None:
        rc = lib.sisic_sample_frames_edit(*head, seeds, step0, *cond, edit.image.data_ptr(), edit.mask.data_ptr(),
                                          C.cast(erows.data_ptr(), _lib.c_float_p), *tail)
    elif guidance is not None:
        rc = lib.sisic_sample_frames_cond(*head, z_ptr, seeds, step0, *cond, *tail)
    elif seeds is not None:
        rc = lib.sisic_sample_frames_rule_rng(*head, seeds, step0, *tail)
    else:
        rc = lib.sisic_sample_frames_rule(*head, z_ptr, *tail)
    return rc, done.value


def _check_edit(edit: Edit, x_T: torch.Tensor) -> Edit:
    """the known image and the mask of an edited run at the latents' shape and device, contiguous"""
    (B, Cc, H, W), dev = x_T.shape, x_T.device
    image, mask = edit.image, edit.mask
    if tuple(image.shape) != (B, Cc, H, W) or image.device != dev or image.dtype != torch.float32:
        raise ValueError(f"the known image must be fp32 {(B, Cc, H, W)} on {dev}, got {image.dtype} {tuple(image.shape)}")
    if tuple(mask.shape) != (B, 1, H, W) or mask.device != dev or mask.dtype != torch.float32:
        raise ValueError(f"the mask must be fp32 {(B, 1, H, W)} on {dev}, got {mask.dtype} {tuple(mask.shape)}")
    return Edit(image.contiguous(), mask.contiguous(), edit.schedule)


@torch.no_grad()
def _run_sampling_loop(model: HipUNet2DModel, scheduler, x_T: torch.Tensor,
                       noise, *, return_trajectory: bool = False, save_indices: Optional[Sequence[int]] = None,
                       cancel_flag: Optional[C.c_int] = None, eta: float = 0.0,
                       use_clipped_model_output: bool = False, guidance: Optional[Guidance] = None,
                       edit: Optional[Edit] = None, max_call_steps: int = MAX_CALL_STEPS,
                       classifier: Optional[ClassifierGuidance] = None, threshold=None) -> SampleResult:
    """threshold: (ratio, sample_max_value) of dynamic thresholding or None, as ``run_sampling_loop`` resolved it.
    classifier: classifier guidance (``ClassifierGuidance``) of an unconditional epsilon-prediction model; needs a
    ``DeviceNoise`` and composes with neither ``guidance`` nor ``edit``.
    edit: an inpainting run (``Edit``): the known region is re-imposed inside every step kernel; needs a ``DeviceNoise``.
    The run has one step per entry of ``edit.schedule`` (``timesteps``, ``steps_done``, the trajectory and ``save_indices``
    count those passes), and one longer than ``max_call_steps`` (at most 1000, the library's limit per call) is cut into calls
    with their step offsets: bit-equal to the uncut run under ddpm and ddim; a DPM-Solver++ run is never cut.
    guidance: the labels, null label and scale of a class-conditional model (``Guidance``); None for an unconditional one.
    x_T: GPU fp32 [B,C,H,W]; noise: GPU fp32 [n_noise,B,C,H,W], None (no noise added), a ``NoiseStream``
    (the loop then runs segment by segment while the stream draws and uploads the next segment's noise), or a
    ``DeviceNoise`` (the step kernel generates z_t from the images' seeds: one call for the whole run, no buffer).
    return_trajectory keeps x after every step, or after the steps in ``save_indices`` only (``trajectory_save_indices``).
    scheduler: a ``HipDDPMScheduler``, a ``HipDDIMScheduler`` or a ``HipDPMSolverMultistepScheduler``; its ``rule`` selects
    the step kernel.  eta and use_clipped_model_output are the DDIM rule's.  n_noise is the number of steps whose sigma is not
    zero under that rule and eta -- none for DDIM at eta = 0 and for the ODE variant of DPM-Solver++, where every noise
    source gives the same result.  A DPM-Solver++ run takes no ``NoiseStream``: the history lives inside one library call.

    Every kind of run goes the same way: the checks, the rule's tables, the plan of its library calls (``plan_calls``: one call,
    unless a ``NoiseStream``'s segments or an edited run's ``max_call_steps`` cut it), then call by call with the noise of its
    source."""
    B, Cc, H, W = x_T.shape
    rule_name = scheduler.rule
    if classifier is not None:
        _check_classifier_guidance(model, classifier, noise, guidance, edit, B)
    if isinstance(noise, NoiseStream) and rule_name == "dpmsolver++":
        raise ValueError("a DPM-Solver++ run is not cut into segments (each cut would lose the history): pass the whole "
                         "noise buffer, a DeviceNoise or None")
    _check_guidance(model, guidance, B)
    if edit is not None and not isinstance(noise, DeviceNoise):
        raise ValueError("inpainting draws on the device only (the known region's noise and the jumps are streams of the "
                         "device-noise contract): pass noise=DeviceNoise(seeds)")
    lib = _lib.load()
    dev = x_T.device
    if dev.type != "cuda":
        raise RuntimeError("the sampling loop runs on MI355X only")
    _set_thresholding(lib, model, threshold)
    if isinstance(noise, DeviceNoise) and len(noise.seeds) != B:
        raise ValueError(f"DeviceNoise holds {len(noise.seeds)} seeds for a batch of {B}")
    ts = scheduler.timesteps.to(torch.int64).contiguous()
    erows = None
    if edit is not None:
        max_call_steps = int(max_call_steps)
        if not 1 <= max_call_steps <= MAX_CALL_STEPS:
            raise ValueError(f"max_call_steps must lie in 1 .. {MAX_CALL_STEPS}, got {max_call_steps}")
        edit = _check_edit(edit, x_T)
        schedule = check_edit_schedule(rule_name, edit.schedule, ts.numel())
    coef, rule, rule_flags = _rule_tables(scheduler, eta, use_clipped_model_output)
    if edit is not None:
        idx = torch.tensor([i for i, _ in schedule], dtype=torch.int64)
        if int(idx.min()) < 0 or int(idx.max()) >= ts.numel():
            raise ValueError(f"edit schedule indices outside 0..{ts.numel() - 1}")
        # a pass runs under the row of ITS grid entry (t -> its own previous grid point), wherever the next pass goes
        ts, coef, erows = ts[idx].contiguous(), coef[idx].contiguous(), edit_rows(scheduler, schedule).contiguous()
        if len(schedule) > max_call_steps and rule == _lib.RULE_DPMPP:
            raise ValueError(f"a DPM-Solver++ run of {len(schedule)} steps is not cut into calls of {max_call_steps} (each cut "
                             "would lose the history)")
    T = ts.numel()                                              # steps of the run: UNet passes
    noisy = (coef[:, 4] != 0).tolist()
    cuts, step0 = [0, T], 0
    if isinstance(noise, DeviceNoise):
        source, step0 = _SeedNoise(noise.seeds), noise.step0
        if edit is not None:
            cuts = list(range(0, T, max_call_steps)) + [T]
    elif isinstance(noise, NoiseStream):
        source, cuts = _StreamNoise(noise), segment_bounds(T, noise.seg, B * Cc * H * W)
    else:
        if noise is not None:
            if tuple(noise.shape) != (sum(noisy), B, Cc, H, W) or noise.device != dev or noise.dtype != torch.float32:
                raise ValueError(f"noise must be fp32 {(sum(noisy), B, Cc, H, W)} on {dev}, got {tuple(noise.shape)}")
            noise = noise.contiguous()
        source = _BufferNoise(noise) if noise is not None else _NoiseSource()
    kept = _frame_rows(T, return_trajectory, save_indices)[0]
    plan = plan_calls(noisy, cuts, kept, step0)
    x = x_T.to(torch.float32).contiguous().clone()
    traj = ops.empty((len(kept), B, Cc, H, W), dtype=torch.float32, device=dev) if return_trajectory else None
    out_u8 = ops.empty((B, H, W, Cc), dtype=torch.uint8, device=dev)
    clip = scheduler.config.clip_sample_range if scheduler.config.clip_sample else 0.0
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    steps_done, rc = 0, 0
    source.start(plan)
    for call in plan:
        rc, done = _library_call(lib, model, x, (ts, coef, erows), clip, rule, rule_flags, call, source.z_ptr(call), source.seeds,
                                 guidance, edit, classifier, traj, out_u8, cancel_flag, stream)
        source.enqueued(call)
        steps_done += done
        if rc != 0:
            break
    if rc != _lib.SISIC_ECANCEL:
        check(rc)
    cancelled = rc == _lib.SISIC_ECANCEL
    if cancelled:
        out_u8.zero_()                         # never hand uninitialised pixels to a caller that ignores `cancelled`
    return SampleResult(images=out_u8, latents=x, trajectory=traj, trajectory_steps=kept, timesteps=[int(t) for t in ts],
                        steps_done=steps_done, cancelled=cancelled, scheduler=rule_name, eta=float(eta), unet_passes=T,
                        prediction_type=getattr(model, "prediction_type", "epsilon"),
                        classifier_scale=classifier.scale if classifier is not None else None,
                        classifier_passes=steps_done if classifier is not None else 0)


def _check_strength(strength) -> float:
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 < float(strength) <= 1.0:
        raise ValueError(f"strength must lie in (0, 1], got {strength!r}")
    return float(strength)


def strength_steps(T: int, strength) -> int:
    """how many of a T-step grid's entries, counted from its end, an edit of this ``strength`` runs: ``min(int(T * strength),
    T)``; ``strength`` lies in (0, 1] and must leave at least one step"""
    n = min(int(int(T) * _check_strength(strength)), int(T))
    if n < 1:
        raise ValueError(f"strength={strength} leaves no step of a {T}-step grid to run")
    return n


def check_edit_options(scheduler: str, noise: str, has_image: bool, has_mask: bool, strength, jump_length, n_resample) -> None:
    """every refusal of the editing keywords that needs no tensor, before anything touches the GPU"""
    if isinstance(n_resample, bool) or not isinstance(n_resample, int) or n_resample < 1:
        raise ValueError(f"n_resample must be a positive integer, got {n_resample!r}")
    if isinstance(jump_length, bool) or not isinstance(jump_length, int) or jump_length < 1:
        raise ValueError(f"jump_length must be a positive integer, got {jump_length!r}")
    _check_strength(strength)
    if not has_image:
        if has_mask or float(strength) != 1.0 or n_resample != 1:
            raise ValueError("mask, strength and n_resample edit an image: pass init_image")
        return
    if not has_mask:
        if float(strength) == 1.0:
            raise ValueError("image-to-image at strength=1 starts from pure noise and would ignore init_image: pass a "
                             "strength below 1, or a mask")
        if n_resample != 1:
            raise ValueError("n_resample resamples the seam of a mask: image-to-image has none")
        return
    if noise != "device":
        raise ValueError("inpainting needs noise='device': the known region's noise and the resampling jumps are drawn in "
                         "the step kernel (host-noise inpainting is not offered)")
    if scheduler == "dpmsolver++" and n_resample != 1:
        raise ValueError("resampling (n_resample > 1) is offered under scheduler='ddpm' and 'ddim': a jump invalidates the "
                         "history of DPM-Solver++, which takes a mask with n_resample=1 only")


def prepare_init_image(init_image, B: int, chw: Tuple[int, int, int], device) -> torch.Tensor:
    """fp32 [B,C,H,W] on ``device`` from fp32 [B,C,H,W] / [C,H,W] in [-1, 1] or uint8 [B,H,W,C] / [H,W,C] (the inverse of
    ``denorm_u8``'s scaling: v / 255 * 2 - 1); a single image is broadcast over the batch"""
    t = torch.as_tensor(init_image)
    Cc, H, W = chw
    if t.dtype == torch.uint8:
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or tuple(t.shape[1:]) != (H, W, Cc):
            raise ValueError(f"a uint8 init_image must be [B,{H},{W},{Cc}] or [{H},{W},{Cc}], got {tuple(t.shape)}")
        t = (t.to(torch.float32) / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2)
    else:
        if not t.dtype.is_floating_point:
            raise ValueError(f"init_image must be fp32 in [-1, 1] or uint8, got {t.dtype}")
        t = t.to(torch.float32)
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or tuple(t.shape[1:]) != (Cc, H, W):
            raise ValueError(f"an fp32 init_image must be [B,{Cc},{H},{W}] or [{Cc},{H},{W}], got {tuple(t.shape)}")
    if t.shape[0] not in (1, B):
        raise ValueError(f"init_image holds {t.shape[0]} images for a batch of {B}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError("init_image must be finite everywhere (also under the mask: the blend multiplies it by 0)")
    return t.expand(B, Cc, H, W).contiguous().to(device)


def prepare_mask(mask, B: int, hw: Tuple[int, int], device) -> torch.Tensor:
    """fp32 [B,1,H,W] on ``device`` from [B,1,H,W], [1,1,H,W] or [H,W]; 1 = keep the known pixel, values within [0, 1]"""
    t = torch.as_tensor(mask).to(torch.float32)
    H, W = hw
    if t.dim() == 2:
        t = t[None, None]
    if t.dim() != 4 or tuple(t.shape[1:]) != (1, H, W) or t.shape[0] not in (1, B):
        raise ValueError(f"mask must be [B,1,{H},{W}] or [{H},{W}], got {tuple(t.shape)}")
    if not bool(((t >= 0) & (t <= 1)).all()):
        raise ValueError("mask values must lie in [0, 1] (1 = keep the known pixel)")
    return t.expand(B, 1, H, W).contiguous().to(device)


COLOR_BLEND = 0.35            # image_generator.py:532 "alpha"
COLOR_SCALE_CLIP = (0.6, 1.4)  # image_generator.py:527


def apply_color_statistics(images: np.ndarray, stats: Optional[dict]) -> np.ndarray:
    """Colour post-processing of the GUI path (``ImageGenerator._apply_color_postprocessing``,
    image_generator.py:502-545) for a batch of uint8 [B,H,W,3] images: each image's per-channel mean and standard
    deviation are pulled towards the class statistics of ``color_statistics.json`` -- scale clipped to [0.6, 1.4],
    35 % blend with the original, clip to [0,255], truncation to uint8.  Host-side numpy in the reference's float32
    operation order (bit-identical results); images are processed one by one because the reference's statistics are
    per image.  ``stats`` = the JSON entry of the class, or None / incomplete: images are returned unchanged."""
    if not stats or "rgb" not in stats or "mean" not in stats["rgb"]:
        return images
    t_mean = np.asarray(stats["rgb"].get("mean", [128, 128, 128]), dtype=np.float32)
    t_std = np.asarray(stats["rgb"].get("std", [50, 50, 50]), dtype=np.float32)
    out = np.empty_like(images)
    for b in range(images.shape[0]):
        img = images[b]
        mean = img.mean(axis=(0, 1)).astype(np.float32)             # float64 accumulation, then float32 like the reference
        std = img.std(axis=(0, 1)).astype(np.float32)
        scale = np.clip(t_std / np.maximum(std, 1e-6), *COLOR_SCALE_CLIP)
        f = img.astype(np.float32)
        moved = (f - mean) * scale + t_mean
        mixed = COLOR_BLEND * moved + (1.0 - COLOR_BLEND) * f
        out[b] = np.clip(mixed, 0, 255).astype(np.uint8)
    return out


class Sampler:
    """Holds one loaded UNet per class, like ``ModelManager.loaded_models`` (model_manager.py:19-171)."""

    def __init__(self, device="cuda", beta_schedule: str = "squaredcos_cap_v2", latency_mode: bool = False):
        """latency_mode=True: every model of this sampler uses the single-image kernel choices
        (HipUNet2DModel.set_latency_mode) -- for the GUI's one-image-at-a-time calls; throughput batches keep the default."""
        self.device = torch.device(device)
        self.beta_schedule = beta_schedule
        self.latency_mode = bool(latency_mode)
        self.models: Dict[str, HipUNet2DModel] = {}
        self.class_labels: Dict[str, int] = {}        # class name -> its label in the conditional model registered for it
        self.cancel = C.c_int(0)          # cooperative stop flag (image_generator.py:320,396)
        self.last_trajectory_steps: List[int] = []   # step indices of the frames the last generate(..., return_trajectory=True) kept
        self.noise_segment_steps = 64     # steps of noise drawn and uploaded per pipeline stage (NoiseStream)
        self.color_statistics: Dict[str, dict] = {}   # class -> color_statistics.json entry (image_generator.py:142-170)
        self._noise_buffers: dict = {}    # pinned/device staging buffers of the last noise shape (NoiseStream)
        self.classifier = None            # set_classifier: the classifier of generate(..., classifier_scale=) ...
        self.classifier_index: Dict[str, int] = {}    # ... and class name -> its output

    def close(self) -> None:
        """Shut the noise producers' thread pool down and drop the pinned / device staging buffers (the models stay)."""
        pool = self._noise_buffers.pop("pool", None)
        if pool is not None:
            pool.shutdown(wait=True)
        self._noise_buffers.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:              # interpreter shutdown: the executor module may already be gone
            pass

    def load_color_statistics(self, path: str) -> int:
        """``checkpoints/color_statistics.json`` (image_generator.py:142-170); returns the number of classes read.
        A missing file leaves post-processing a no-op, as in the reference."""
        import json
        import os as _os
        if not _os.path.exists(path):
            return 0
        with open(path, "r") as f:
            self.color_statistics = json.load(f)
        return len(self.color_statistics)

    def add_model(self, class_name: str, state_dict: Dict[str, torch.Tensor], prediction_type: str = "epsilon",
                  **unet_kwargs) -> HipUNet2DModel:
        """``prediction_type``: what the checkpoint was trained to predict ("epsilon", "sample" or "v_prediction").  The model
        carries it, so every ``generate*`` call and loop uses the matching step arithmetic with nothing new from the caller;
        ``SampleResult.prediction_type`` records it."""
        m = HipUNet2DModel(prediction_type=prediction_type, **unet_kwargs)
        m.set_latency_mode(self.latency_mode)
        m.load_state_dict(state_dict)
        m = m.to(self.device)
        m.eval()
        self.models[class_name] = m
        return m

    def add_conditional_model(self, class_names: Sequence[str], state_dict: Dict[str, torch.Tensor],
                              prediction_type: str = "epsilon", **unet_kwargs) -> HipUNet2DModel:
        """ONE class-conditional model for several class names (``train.train_conditional``'s checkpoint): the label of a
        name is its index in ``class_names``, the null label of classifier-free guidance is ``len(class_names)``, so the model
        has ``len(class_names) + 1`` embedding rows.  Every name then works wherever a class name does, and a call may mix
        them (``generate_seeds(["MEL", "NV", "MEL"], seeds, ...)``)."""
        names = [str(n) for n in class_names]
        if isinstance(class_names, str) or not names or len(set(names)) != len(names):
            raise ValueError(f"class_names must be a non-empty sequence of distinct names, got {class_names!r}")
        taken = [n for n in names if n in self.models]
        if taken:
            raise ValueError(f"a model is already registered for {taken}")
        rows = unet_kwargs.setdefault("num_class_embeds", len(names) + 1)
        if rows != len(names) + 1:
            raise ValueError(f"a conditional model for {len(names)} classes has {len(names) + 1} embedding rows (the last is "
                             f"the null label), got num_class_embeds={rows}")
        m = self.add_model(names[0], state_dict, prediction_type=prediction_type, **unet_kwargs)
        for k, n in enumerate(names):
            self.models[n] = m
            self.class_labels[n] = k
        return m

    def set_classifier(self, clf, class_index: Dict[str, int]) -> None:
        """The classifier ``generate*(..., classifier_scale=)`` steers with, and ``class_index``: class name -> the classifier
        output that stands for it.  ``clf``: a loaded ``HipMelanomaClassifier`` on this sampler's device."""
        index = {str(k): int(v) for k, v in dict(class_index).items()}
        n = int(clf.num_classes)
        bad = {k: v for k, v in index.items() if not 0 <= v < n}
        if bad:
            raise ValueError(f"class_index entries outside the classifier's outputs [0, {n}): {bad}")
        self.classifier = clf
        self.classifier_index = index

    def _classifier_guidance(self, names: List[str], model: HipUNet2DModel, classifier_scale, noise: str, guidance_scale,
                             edited: bool) -> ClassifierGuidance:
        """the ClassifierGuidance of a generate* call; every refusal of the public interface is here"""
        if self.classifier is None:
            raise ValueError("classifier_scale needs a classifier: Sampler.set_classifier(clf, class_index) first")
        if noise != "device":
            raise ValueError('classifier_scale requires noise="device"')
        if check_guidance_scale(guidance_scale) != 1.0 or model.config.num_class_embeds is not None:
            raise ValueError("classifier_scale steers an unconditional model: it does not compose with guidance_scale or a "
                             "class-conditional model")
        if edited:
            raise ValueError("classifier_scale does not compose with init_image / mask")
        missing = sorted({c for c in names if c not in self.classifier_index})
        if missing:
            raise KeyError(f"set_classifier's class_index has no entry for {missing}")
        return ClassifierGuidance(self.classifier, tuple(self.classifier_index[c] for c in names), classifier_scale)

    def _resolve_classes(self, class_name, n_images: int, guidance_scale,
                         one_model_suffices: bool = False) -> Tuple[HipUNet2DModel, List[str], Optional[Guidance]]:
        """(model, one class name per image, Guidance or None) of a call; every refusal of the public interface is here.
        one_model_suffices: a classifier-guided call, where the names of an unconditional model's batch may differ (they choose
        the classifier's targets) as long as they are registered to ONE model."""
        scale = check_guidance_scale(guidance_scale)
        if isinstance(class_name, str):
            names = [class_name] * n_images
        else:
            names = [str(c) for c in class_name]
            if len(names) != n_images:
                raise ValueError(f"{len(names)} class names for {n_images} images: a sequence holds one entry per seed")
            if not names:
                raise ValueError("no class name given")
        for c in names:
            if c not in self.models:
                raise KeyError(f"no model loaded for class '{c}'")
        model = self.models[names[0]]
        if any(self.models[c] is not model for c in names):
            raise ValueError("the class names of one call must belong to one conditional model")
        if model.config.num_class_embeds is None:
            if len(set(names)) > 1 and not one_model_suffices:
                raise ValueError("an unconditional model generates one class per call")
            if scale != 1.0:
                raise ValueError(f"guidance_scale={scale} needs a class-conditional model (add_conditional_model); the model "
                                 f"of '{names[0]}' is unconditional")
            return model, names, None
        null = model.config.num_class_embeds - 1
        labels = [self.class_labels[c] for c in names]
        if scale == 0.0:              # the unconditional prediction alone: null labels at scale 1, one pass per step
            labels, scale = [null] * n_images, 1.0
        return model, names, Guidance(tuple(labels), null, scale)

    def create_scheduler(self, T: int, scheduler: str = "ddpm", solver_order: int = 2, algorithm_type: str = "dpmsolver++"):
        """model_manager.py:196-212; scheduler="ddim": the DDIM mirror over the same tables and timestep grid;
        scheduler="dpmsolver++": the DPM-Solver++ mirror over the same tables and the same grid (its "leading" spacing; the
        mirror's own default is the published "linspace"), with the clamp of x0 the other two rules apply (clip_sample=True)."""
        mirror = MIRRORS[_check_scheduler(scheduler, 0.0, False, solver_order, algorithm_type)]
        own = dict(solver_order=solver_order, algorithm_type=algorithm_type, clip_sample=True,
                   timestep_spacing="leading") if mirror._takes_solver_options else {}
        s = mirror(num_train_timesteps=1000, beta_schedule=self.beta_schedule, **own)
        s.set_timesteps(max(1, min(1000, int(T))))
        return s

    def request_stop(self) -> None:
        """Cooperative stop (``stop_generation``, image_generator.py:784-786): the running loop ends at the next step."""
        self.cancel.value = 1

    def generate_images(self, class_name, seeds: Sequence[int], T: int, **kwargs) -> SampleResult:
        """Start of a generation run in the reference's sense (``generate_images`` clears ``stop_requested`` before
        its first image, image_generator.py:567): resets the stop flag, then samples ``seeds``.  A stop request that
        arrives later ends this run only."""
        self.cancel.value = 0
        return self.generate_seeds(class_name, seeds, T, **kwargs)

    def generate_seeds(self, class_name, seeds: Sequence[int], T: int, size: Tuple[int, int] = (128, 128),
                       return_trajectory: bool = False, save_every_n: Optional[int] = None,
                       noise: str = "host", scheduler: str = "ddpm", eta: float = 0.0,
                       use_clipped_model_output: bool = False, solver_order: int = 2,
                       algorithm_type: str = "dpmsolver++", guidance_scale: float = 1.0, init_image=None, mask=None,
                       strength: float = 1.0, jump_length: int = 10, n_resample: int = 1,
                       max_call_steps: int = MAX_CALL_STEPS, classifier_scale: Optional[float] = None,
                       thresholding: bool = False, dynamic_thresholding_ratio: float = 0.995,
                       sample_max_value: float = 1.0) -> SampleResult:
        """thresholding, dynamic_thresholding_ratio, sample_max_value: dynamic thresholding of x0 (Saharia et al. 2022), the
        published schedulers' arguments of these names: per image and step, s = the ``ratio`` quantile of |x0| clamped to
        [1, ``sample_max_value``], and x0 becomes clamp(x0, -s, s) / s in place of the static clamp.  Every rule, both noise modes,
        every guidance and edit.  Off (the default) is today's run; the result records ``thresholding``.
        classifier_scale: classifier guidance (Dhariwal & Nichol 2021) of an unconditional epsilon-prediction model with the
        classifier of ``set_classifier``: every step applies its rule to ``eps - (scale * sqrt(1 - abar_t)) * g``, ``g`` the
        classifier's input gradient towards image b's class at the step's latent.  ``class_name`` may then be a sequence with one
        name per image, all registered to one model (``sampler.models[name]`` is the same object); the names choose the targets
        through ``class_index``.  Requires noise="device"; refused with ``guidance_scale``, ``init_image`` / ``mask`` and on a
        class-conditional model.  None (the default) is today's run; the result records ``classifier_scale`` and
        ``classifier_passes``.
        init_image, mask, strength, jump_length, n_resample: image editing (module docstring).  init_image: fp32 [B,3,H,W]
        in [-1, 1] or uint8 [B,H,W,3], a single image is broadcast.  Without a mask the call is image-to-image: the run goes
        through the last ``min(int(T * strength), T)`` entries of the grid, starting from ``add_noise(init_image, x_T, t)`` at
        the first of them (``strength`` below 1; both noise modes, every rule; DPM-Solver++ starts first order there).  mask
        ([B,1,H,W] or [H,W], 1 = keep): inpainting, which needs noise="device"; ``strength=1`` starts from x_T itself;
        ``n_resample > 1`` adds RePaint's resampling jumps of ``jump_length`` levels (ddpm and ddim).  The result records
        ``strength``, ``n_resample`` and ``unet_passes``.  max_call_steps: the longest library call of an inpainting run.
        save_every_n: keep only the trajectory frames the reference's XAI run keeps (``trajectory_save_indices``,
        xai/XAI.py:751-777) instead of all T -- 3.1 GB at 64 images x 64x64 x T = 1000 otherwise.
        noise: "host" (the default: one CPU generator per image, see the module docstring) or "device" (x_T from torch's
        device generator, z_t generated in the step kernel: no host RNG, no noise buffers; other images for the same seed).
        scheduler: "ddpm" (the default) or "ddim" with its ``eta`` (0 = deterministic) and ``use_clipped_model_output``; x_T and
        ``noise_hashes`` of a seed do not depend on it.  Host-mode z rows go to the steps with sigma != 0 only (module
        docstring): at eta = 0 nothing beyond x_T is drawn.
        scheduler="dpmsolver++": DPM-Solver++(2M) with ``solver_order`` (1 or 2) and ``algorithm_type`` ("dpmsolver++", which
        like DDIM at eta = 0 draws nothing beyond x_T, or "sde-dpmsolver++"); it has no eta and no
        use_clipped_model_output.
        class_name: for a model registered with ``add_conditional_model`` also a sequence with one name per seed (a batch may
        mix classes).  guidance_scale: classifier-free guidance for such a model -- 1 (the default) samples under the labels
        alone, one UNet pass per step; any other value steps on ``eps_u + scale * (eps_c - eps_u)`` with both predictions from
        one pass at twice the batch; 0 is the null-label model alone and runs as null labels at scale 1.  x_T, the noise
        contract and ``noise_hashes`` do not depend on labels or scale.  A scale other than 1 on an unconditional model is a
        ValueError."""
        _check_noise_mode(noise)
        _check_scheduler(scheduler, eta, use_clipped_model_output, solver_order, algorithm_type)
        check_edit_options(scheduler, noise, init_image is not None, mask is not None, strength, jump_length, n_resample)
        model, names, guidance = self._resolve_classes(class_name, len(seeds), guidance_scale, classifier_scale is not None)
        sched = self.create_scheduler(T, scheduler, solver_order, algorithm_type)
        check_thresholding(thresholding, dynamic_thresholding_ratio, sample_max_value)
        rule_args = dict(eta=eta, use_clipped_model_output=use_clipped_model_output, guidance=guidance,
                         thresholding=bool(thresholding), dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                         sample_max_value=sample_max_value)
        if classifier_scale is not None:
            rule_args["classifier"] = self._classifier_guidance(names, model, classifier_scale, noise, guidance_scale,
                                                                init_image is not None or mask is not None)
        H, W = size
        start = None                     # image-to-image and inpainting below strength 1: x_T -> the noised init_image
        if init_image is not None:
            B, chw = len(seeds), (model.config.in_channels, H, W)
            n_steps = strength_steps(sched.timesteps.numel(), strength)
            image = prepare_init_image(init_image, B, chw, self.device)
            # the last n_steps entries of the grid: the rules' rows are those of the grid (a step goes to its own previous grid
            # point), and DPM-Solver++'s first row there is first order
            sched.timesteps = sched.timesteps[sched.timesteps.numel() - n_steps:]
            if float(strength) < 1.0:
                t0 = sched.timesteps[:1].expand(B)
                start = lambda x_T: sched.add_noise(image, x_T.to(self.device), t0)      # noqa: E731
            if mask is not None:
                passes = resample_schedule(n_steps, jump_length, n_resample) if n_resample > 1 else None
                rule_args.update(edit=Edit(image, prepare_mask(mask, B, (H, W), self.device), passes),
                                 max_call_steps=max_call_steps)
        save_indices = None
        if return_trajectory and save_every_n is not None:
            pass_ts = [int(sched.timesteps[i]) for i, _ in rule_args["edit"].schedule] \
                if rule_args.get("edit") is not None and rule_args["edit"].schedule is not None else [int(t) for t in sched.timesteps]
            save_indices = trajectory_save_indices(pass_ts, save_every_n)
        n_noise = int((_rule_tables(sched, eta, use_clipped_model_output)[0][:, 4] != 0).sum())     # steps with sigma != 0

        chw = (model.config.in_channels, H, W)
        ns = None
        try:
            if noise == "device":
                x_T, source = draw_x_T_device(seeds, chw, self.device), DeviceNoise(tuple(seeds))
            elif scheduler == "dpmsolver++" or (scheduler == "ddim" and n_noise == 0):
                # DDIM at eta = 0 and the ODE variant of DPM-Solver++: the run draws x_T and nothing else -- no z, no staging
                # buffers, no worker threads.  The SDE variant: every z of the run up front and ONE library call, because the
                # segments of a NoiseStream would each start without the history (T is 10 to 25 under this rule).
                x_T, z = draw_noise(seeds, n_noise, chw)
                source = z.to(self.device) if n_noise else None
            else:
                # noise is drawn segment by segment on worker threads while the GPU samples (NoiseStream); the values are
                # those of draw_noise(seeds, n_noise, ...)
                ns = NoiseStream(seeds, chw, self.device, self.noise_segment_steps, buffer_cache=self._noise_buffers)
                x_T, source = ns.x_T, ns if n_noise else None
            hashes = [noise_hash(x_T[b:b + 1]) for b in range(len(seeds))]
            res = run_sampling_loop(model, sched, x_T.to(self.device) if start is None else start(x_T), source,
                                    return_trajectory=return_trajectory, save_indices=save_indices, cancel_flag=self.cancel,
                                    **rule_args)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            if ns is not None:
                ns.close()
        res.seeds = [int(s) for s in seeds]
        res.noise_hashes = hashes
        if init_image is not None:
            res.strength, res.n_resample = float(strength), int(n_resample)
        return res

    def generate(self, seed: int, class_name, T: int, *, count: int = 1, size: Tuple[int, int] = (128, 128),
                 return_trajectory: bool = False, seed_is_base: bool = False, postprocess: bool = False,
                 save_every_n: Optional[int] = None, noise: str = "host", scheduler: str = "ddpm", eta: float = 0.0,
                 use_clipped_model_output: bool = False, solver_order: int = 2, algorithm_type: str = "dpmsolver++",
                 guidance_scale: float = 1.0, init_image=None, mask=None, strength: float = 1.0, jump_length: int = 10,
                 n_resample: int = 1, classifier_scale: Optional[float] = None, thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0):
        """``generate(seed, class, T)``: returns (uint8 [count,H,W,3] numpy, trajectory list | None).

        save_every_n: with return_trajectory, the list holds only the frames of ``trajectory_save_indices`` (every n-th
        step and the last: xai/XAI.py:751-757), in step order; ``last_trajectory_steps`` then names their step indices.

        seed_is_base=False: image i uses ``manual_seed(seed + i)`` directly (the literal call);
        seed_is_base=True: ``seed`` is the GUI's base seed and image i uses
        ``(seed + md5_offset(class) + i) & 0x7fffffff`` (image_generator.py:626-631).
        postprocess=True applies the class colour statistics (``load_color_statistics``) to the uint8 images like
        ``generate_single_image(..., postprocess=True)`` does before saving (image_generator.py:449-452).
        noise: "host" or "device", as in ``generate_seeds``.
        scheduler, eta, use_clipped_model_output, solver_order, algorithm_type: the step rule, as in ``generate_seeds``.
        init_image, mask, strength, jump_length, n_resample: image-to-image and inpainting, as in ``generate_seeds``.
        classifier_scale: classifier guidance, as in ``generate_seeds``.
        thresholding, dynamic_thresholding_ratio, sample_max_value: dynamic thresholding of x0, as in ``generate_seeds``.
        class_name, guidance_scale: as in ``generate_seeds``; a sequence of names gives one image per name (``count`` must be 1
        or its length), and with seed_is_base image i derives its seed from ITS class name.
        Always returns a tuple (the reference's bare ``return False`` on early exit is a latent bug).
        """
        if not isinstance(class_name, str):
            names = [str(c) for c in class_name]
            if count not in (1, len(names)):
                raise ValueError(f"{len(names)} class names for count={count}: a sequence holds one entry per image")
            count = len(names)
        else:
            names = [class_name] * count
        if seed_is_base:
            seeds = [image_seed(seed, names[i], i) for i in range(count)]
        else:
            seeds = [(int(seed) + i) & 0x7FFFFFFF for i in range(count)]
        res = self.generate_images(class_name, seeds, T, size=size, return_trajectory=return_trajectory,
                                   save_every_n=save_every_n, noise=noise, scheduler=scheduler, eta=eta,
                                   use_clipped_model_output=use_clipped_model_output, solver_order=solver_order,
                                   algorithm_type=algorithm_type, guidance_scale=guidance_scale, init_image=init_image,
                                   mask=mask, strength=strength, jump_length=jump_length, n_resample=n_resample,
                                   classifier_scale=classifier_scale, thresholding=thresholding,
                                   dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value)
        self.last_trajectory_steps = list(res.trajectory_steps)
        n_frames = sum(1 for i in res.trajectory_steps if i < res.steps_done)       # kept frames of the completed steps
        if res.cancelled:
            # the reference returns False for a stopped image (image_generator.py:396-398); the tuple shape is kept, with
            # no images, and the steps that did complete when a trajectory was asked for
            traj = [res.trajectory[i] for i in range(n_frames)] if return_trajectory else None
            return None, traj
        images = res.images.cpu().numpy()
        if postprocess and isinstance(class_name, str):
            images = apply_color_statistics(images, self.color_statistics.get(class_name))
        elif postprocess:             # mixed classes: each image towards its own class statistics
            images = np.concatenate([apply_color_statistics(images[i:i + 1], self.color_statistics.get(names[i]))
                                     for i in range(count)])
        traj = None
        if return_trajectory:
            # list of per-step (B,3,H,W) tensors, the shape xai_integration.py consumes
            traj = [res.trajectory[i] for i in range(n_frames)]
        return images, traj


_default_sampler: Optional[Sampler] = None


def generate(seed: int, class_name: str, T: int, **kwargs):
    """Module-level convenience over a process-wide ``Sampler`` whose models were registered with
    ``default_sampler().add_model(...)``."""
    return default_sampler().generate(seed, class_name, T, **kwargs)


def default_sampler() -> Sampler:
    global _default_sampler
    if _default_sampler is None:
        _default_sampler = Sampler()
    return _default_sampler
