"""CPU restatement of the bf16x3 arithmetic contract (conv_winograd_bf3.inc:5-17, restated by ``att_split2`` in attention.hip).

TEST INFRASTRUCTURE ONLY.  The dominant kernels form fp32 products on the bf16 matrix pipe: every operand is split EXACTLY
into three bf16 terms

    hi  = the top 16 bits of x          mid = the top 16 bits of x - hi          lo = the top 16 bits of (x - hi) - mid

(truncations and exact differences, never roundings), and SIX of the nine term products -- hi*hi, hi*mid, mid*hi, mid*mid,
hi*lo, lo*hi; the first factor is the A operand (filter, key), the second the B operand (input, query) -- are summed in fp32
by three v_mfma_f32_32x32x16_bf16 per eight channels:

    instruction 1   A = (hi, mid)  B = (hi , mid)      hi*hi  + mid*mid
    instruction 2   A = (hi, mid)  B = (mid, hi )      hi*mid + mid*hi
    instruction 3   A = (hi, lo )  B = (lo , hi )      hi*lo  + lo*hi

This file states that twice for a contraction over a channel axis -- the CONTRACT (the six-term sum in float64) and an
fp32 EMULATION (16 products per instruction summed exactly, rounded into the fp32 accumulator once per instruction, the model
of tools/bf16x3_accuracy.py) -- and removes one kept product over some channels on request (``missing``): the mutants a test
of this arithmetic has to tell from the real thing.  The adapters below put each kernel's operands into the contraction the
way the kernel does; ``CASES`` is the one case table of tests/test_bf3_ref_cpu.py (which proves on the CPU that every case
separates right from wrong) and tests/test_gpu_bf3_terms.py (which holds the kernels to the bound those mutants set).
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

CHUNK = 8                                   # channels per MFMA: K = 16 is eight channels x two terms
HI, MID, LO = 0, 1, 2
# the three instructions of a chunk, each two (A term, B term) products
INSTRUCTIONS = (((HI, HI), (MID, MID)), ((HI, MID), (MID, HI)), ((HI, LO), (LO, HI)))
# the third-order products: the kept ones whose loss the 1e-5 parity bound does not see
THIRD_ORDER = {"mid*mid": (MID, MID), "hi*lo": (HI, LO), "lo*hi": (LO, HI)}


def _trunc16(x: torch.Tensor) -> torch.Tensor:
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split3(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """x (fp32) -> (hi, mid, lo), three fp32 tensors with 8 significant bits each and hi + mid + lo == x exactly."""
    assert x.dtype == torch.float32
    hi = _trunc16(x)
    r1 = x - hi
    mid = _trunc16(r1)
    lo = _trunc16(r1 - mid)
    return hi, mid, lo


def six_term(a: torch.Tensor, b: torch.Tensor, missing=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """a [..., M, K] (x) b [..., K, N] over K, both fp32, K in the order the kernel's chunks of eight take it.

    Returns (emulation fp32, contract float64).  ``missing = (product, where)``: the product ("mid*mid", "hi*lo", "lo*hi") is
    left out over the K indices ``where`` (a slice, or a bool mask over K)."""
    K = a.shape[-1]
    assert b.shape[-2] == K
    ta, tb = split3(a), split3(b)
    keep = None
    if missing is not None:
        prod, where = missing
        gone = torch.zeros(K, dtype=torch.bool)
        gone[where] = True
        keep = (~gone).to(torch.float64)
        missing = THIRD_ORDER[prod]
    ta64, tb64 = [t.double() for t in ta], [t.double() for t in tb]
    shape = torch.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1])
    acc = torch.zeros(shape, dtype=torch.float32)
    contract = torch.zeros(shape, dtype=torch.float64)
    for k0 in range(0, K, CHUNK):
        sl = slice(k0, min(k0 + CHUNK, K))
        for ins in INSTRUCTIONS:
            block = torch.zeros(shape, dtype=torch.float64)
            for prod in ins:
                x = ta64[prod[0]][..., sl]
                if prod == missing:
                    x = x * keep[sl]
                block = block + x @ tb64[prod[1]][..., sl, :]          # (16-bit products, at most 16 of them: exact)
            acc = (acc.double() + block).float()                      # one rounding into the accumulator per instruction
            contract = contract + block
    return acc, contract


# --------------------------------------------------------------------------------------------------------------- adapters
# Every adapter returns (emulation, contract) of the kernel's OUTPUT, both float64 tensors shaped like it: whatever follows the
# products (the Winograd output transform, the bias, the softmax and P.V) is applied to both in float64.

def direct_1x1(x, w, bias=None, missing=None):
    """1x1 stride 1 (conv_pointwise_bf3.hip): weights and inputs are split as they are.  ``missing`` over input channels."""
    B, C, H, W = x.shape
    em, ct = six_term(w.reshape(w.shape[0], C), x.permute(1, 0, 2, 3).reshape(C, -1), missing)
    out = []
    for m in (em.double(), ct):
        y = m.reshape(-1, B, H, W).permute(1, 0, 2, 3)
        out.append(y if bias is None else y + bias.double()[None, :, None, None])
    return out[0], out[1]


def direct_3x3_s2(x, w, bias=None, missing=None):
    """3x3 stride 2, padding 1 (conv_s2_bf3.hip), by unfolding: per chunk of eight channels nine taps, three instructions per
    tap.  ``missing = (product, channel slice)`` over input channels."""
    B, C, H, W = x.shape
    assert C % CHUNK == 0
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    cols = F.unfold(x, 3, padding=1, stride=2)                                         # [B, C * 9, L], (channel, tap)
    cols = cols.reshape(B, C // CHUNK, CHUNK, 9, -1).permute(1, 3, 2, 0, 4).reshape(C * 9, -1)     # K = [chunk][tap][8]
    wk = w.reshape(-1, C // CHUNK, CHUNK, 9).permute(0, 1, 3, 2).reshape(-1, C * 9)
    if missing is not None:
        gone = torch.zeros(C, dtype=torch.bool)
        gone[missing[1]] = True
        missing = (missing[0], gone.reshape(C // CHUNK, 1, CHUNK).expand(-1, 9, -1).reshape(-1))
    em, ct = six_term(wk, cols, missing)
    out = []
    for m in (em.double(), ct):
        y = m.reshape(-1, B, Ho, Wo).permute(1, 0, 2, 3)
        out.append(y if bias is None else y + bias.double()[None, :, None, None])
    return out[0], out[1]


def winograd_filter(w: torch.Tensor) -> torch.Tensor:
    """U = G g G^T as the pack kernel makes it (pack_device.h): float64 arithmetic, stored as fp32.  [16, Cout, Cin]"""
    g = w.double()
    g0, g1, g2 = g[:, :, 0], g[:, :, 1], g[:, :, 2]                                    # rows of the 3 x 3 filter
    t = torch.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2], dim=2)       # [Cout, Cin, 4, 3]
    c0, c1, c2 = t[..., 0], t[..., 1], t[..., 2]
    u = torch.stack([c0, 0.5 * (c0 + c1 + c2), 0.5 * (c0 - c1 + c2), c2], dim=3)       # [Cout, Cin, 4, 4]
    return u.float().reshape(u.shape[0], u.shape[1], 16).permute(2, 0, 1).contiguous()


def winograd_input(x, gn=None, silu=False, x2=None, upsample=False) -> Tuple[torch.Tensor, int, int]:
    """V = B^T d B of every 4 x 4 patch in fp32, in the kernels' operation order: [16, Cin, B * tiles], and the tile grid."""
    if x2 is not None:
        x = torch.cat([x, x2], dim=1)
    if gn is not None:
        x = x * gn[0][:, :, None, None] + gn[1][:, :, None, None]                      # fp32, as staged
        if silu:
            x = F.silu(x)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    B, C, H, W = x.shape
    ty, tx = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (1, 2 * tx - W + 1, 1, 2 * ty - H + 1))                              # zero padding, whole 2 x 2 output tiles
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                             # [B, C, ty, tx, 4, 4]
    # rows first, then columns: V_ij = (d[a][c] + sr d[b][c]) + sc (d[a][e] + sr d[b][e]), every sum rounded to fp32
    r = torch.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :],
                     d[..., 1, :] - d[..., 3, :]], dim=-2)
    v = torch.stack([r[..., 0] - r[..., 2], r[..., 1] + r[..., 2], r[..., 2] - r[..., 1], r[..., 1] - r[..., 3]], dim=-1)
    v = v.reshape(B, C, ty * tx, 16).permute(3, 1, 0, 2).reshape(16, C, B * ty * tx)
    return v.contiguous(), ty, tx


def winograd_3x3(x, w, bias=None, gn=None, silu=False, x2=None, upsample=False, missing=None):
    """F(2x2,3x3) (conv_winograd_bf3.inc, tile_cfg 74 and its 8x8 K-split form 92): GroupNorm scale / shift and SiLU, zero
    padding, optional nearest-2x and two-input concatenation, V and U in fp32, both split, contracted per Winograd position,
    Y = A^T M A plus bias.  ``missing = (product, channel slice)`` over the (concatenated) input channels."""
    B = x.shape[0]
    v, ty, tx = winograd_input(x, gn, silu, x2, upsample)
    u = winograd_filter(w)
    H, W = (2 * x.shape[2], 2 * x.shape[3]) if upsample else (x.shape[2], x.shape[3])
    out = []
    for m in six_term(u, v, missing):
        m = m.double().reshape(4, 4, -1, B, ty, tx)
        s = torch.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]], dim=0)               # A^T M      [2, 4, ...]
        y = torch.stack([s[:, 0] + s[:, 1] + s[:, 2], s[:, 1] - s[:, 2] - s[:, 3]], dim=1)          # ... A  [2, 2, Cout, B, ty, tx]
        y = y.permute(3, 2, 4, 0, 5, 1).reshape(B, -1, 2 * ty, 2 * tx)[:, :, :H, :W]
        out.append(y if bias is None else y + bias.double()[None, :, None, None])
    return out[0], out[1]


ATT_SCALE = torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.sqrt(torch.tensor(8.0, dtype=torch.float32))


def attention(qkv, heads, missing=None):
    """attention.hip: q times head_dim**-0.5 * log2(e) in fp32 BEFORE the split, S^T = K^T Q with the key as the A operand and
    the eight head dimensions as the chunk; softmax (base 2, the same function) and P.V in float64.  ``missing`` names the
    product only: it is removed over the whole head dimension."""
    B, C3, N = qkv.shape
    C = C3 // 3
    d = C // heads
    assert d == CHUNK
    q, k, v = qkv.reshape(B, 3, heads, d, N).unbind(1)                                 # [B, heads, d, N]
    qs = q * ATT_SCALE
    if missing is not None and not isinstance(missing, tuple):
        missing = (missing, slice(None))
    out = []
    for s in six_term(k.transpose(2, 3), qs, missing):                                 # [B, heads, key, query]
        s = s.double()
        p = torch.exp2(s - s.max(dim=2, keepdim=True).values)
        p = p / p.sum(dim=2, keepdim=True)
        out.append(torch.einsum("bhkq,bhdk->bhdq", p, v.double()).reshape(B, C, N))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------------------------ cases
class Case(NamedTuple):
    """One case of the GPU test.  mode "chunks": one run per 8-channel chunk with ONLY that chunk active (every other channel
    has zero data and zero GroupNorm scale and shift), mutants = the three third-order products missing in that chunk;
    mode "dense": one run on dense inputs, mutants = the three products missing everywhere."""
    kind: str                 # "wino" | "pw" | "s2" | "att"
    cfg: int                  # tile_cfg forced through ops.conv2d (attention: the query-block form the batch selects)
    B: int
    H: int                    # input plane (attention: H = N, W = 1)
    W: int
    c0: int
    c1: int                   # second (concatenated) input
    cout: int
    mode: str = "chunks"
    pro: bool = False         # GroupNorm scale / shift + SiLU prologue
    ups: bool = False         # nearest-2x input
    images: Optional[Tuple[int, ...]] = None      # the images the CPU reference is computed for (None: all)

    @property
    def cin(self):
        return self.c0 + self.c1

    @property
    def ident(self):
        s = f"{self.kind}{self.cfg}-B{self.B}-{self.H}x{self.W}-{self.c0}" + (f"+{self.c1}" if self.c1 else "") + f"to{self.cout}"
        return s + ("-ups" if self.ups else "") + ("-gn" if self.pro else "") + ("-dense" if self.mode == "dense" else "")


# the chunk counts that enter and leave every body of the pipelined channel loops: 1, 2, 3, 5, 6, 7, 9, 13
LOOP_TAIL_CINS = (8, 16, 24, 40, 48, 56, 72, 104)
# the largest reduction of the network's layers (test_conv_reference_layer_shapes: 512 -> 256 at 16x16 and 8x8)
NET_MAX_CIN = 512
# 320 work items of tile_cfg 74 on 256 persistent workgroups (test_conv3x3_winograd_bf16x3_persistent_workgroups' first
# shape): with 256 CUs the items 256 .. 319 are tiles of images 2, 4, 7, 9, 12, 14, 17 and 19 -- the reference is computed
# for one image whose tiles are all first items and two that hold second items (reached through the halo prefetch)
PERSISTENT_IMAGES = (0, 9, 19)

CASES = (
    [Case("wino", 74, 1, 16, 16, c, 0, 64, pro=True) for c in LOOP_TAIL_CINS]
    + [Case("wino", 74, 1, 8, 8, 24, 0, 64, ups=True),                         # nearest-2x: 8x8 -> 16x16
       Case("wino", 74, 1, 16, 16, 20, 20, 64, pro=True),                      # the concatenation's seam inside chunk 2
       Case("wino", 74, 20, 64, 64, 24, 0, 64, mode="dense", pro=True, images=PERSISTENT_IMAGES),
       Case("wino", 74, 1, 16, 16, NET_MAX_CIN, 0, 64, mode="dense", pro=True),
       Case("wino", 92, 4, 8, 8, 128, 0, 64, pro=True),
       Case("wino", 92, 4, 8, 8, NET_MAX_CIN, 0, 64, mode="dense", pro=True)]
    + [Case("pw", cfg, 2, 16, 16, c, 0, 128) for cfg in (29, 30) for c in LOOP_TAIL_CINS]
    + [Case("pw", 34, 2, 16, 16, c, 0, 384) for c in LOOP_TAIL_CINS]
    + [Case("pw", 35, 2, 16, 16, c, 0, 128) for c in (128, 256)]
    + [Case("pw", 28, 2, 16, 16, NET_MAX_CIN, 0, 128, mode="dense"),
       Case("pw", 35, 2, 16, 16, NET_MAX_CIN, 0, 128, mode="dense"),
       Case("pw", 34, 2, 16, 16, 256, 0, 384, mode="dense")]                   # (the staged form takes at most 391 channels)
    + [Case("s2", 36, 2, 16, 16, c, 0, 64) for c in (8, 24, 72)]
    + [Case("s2", 36, 2, 16, 16, NET_MAX_CIN, 0, 64, mode="dense")]
    # attention, C = 64 (eight heads): N = 100 has a masked tail tile, N = 300 two key blocks; B * heads * ceil(N / 256) >= 1024
    # selects two query blocks per wave (cfg 2), a batch of two takes one (cfg 1)
    + [Case("att", 1, 2, 100, 1, 64, 0, 64, mode="dense"), Case("att", 2, 128, 100, 1, 64, 0, 64, mode="dense", images=(0, 64, 127)),
       Case("att", 1, 2, 300, 1, 64, 0, 64, mode="dense"), Case("att", 2, 64, 300, 1, 64, 0, 64, mode="dense", images=(0, 32, 63))]
)


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def runs(case: Case):
    """the case's runs: the active chunk of each, or (None,) for a dense case"""
    return (None,) if case.mode == "dense" else tuple(range(case.cin // CHUNK))


def inputs(case: Case, chunk: Optional[int]):
    """The run's tensors as the kernel gets them (fp32, CPU): dict(x, x2, w, bias, gn).  ``chunk``: only channels
    8 * chunk .. 8 * chunk + 7 are non-zero -- data, scale and shift -- so the prologue leaves the others at exactly 0.
    Weights are scaled for O(1) outputs from the channels that are active."""
    idx = CASES.index(case)
    seed = 7000 + 100 * idx
    if case.kind == "att":
        return dict(qkv=_rand(case.B, 3 * case.cin, case.H, seed=seed) * 1.5)
    k = 1 if case.kind == "pw" else 3
    cin = case.cin
    # A dense reduction over hundreds of channels: the emulation's own distance grows with the number of roundings made while the
    # accumulator is large (5e-7 at 512 channels of equal magnitude, 1.3e-6 for the 4608 products of the stride-2 form) and
    # the mutants' does not (1e-5 of the largest output at every length), so equal magnitudes do not separate by 16.  The
    # channels' magnitudes therefore RISE along the channel axis, four decades from the first channel to the last: every chunk
    # still goes through the loop with non-zero operands, the accumulator is large for the last seventh of it only.  (What
    # a chunk early in the loop does to the third-order products is the one-chunk runs' business.)
    ramp = chunk is None and cin > 64
    mag = 10.0 ** (-4.0 * (1.0 - torch.arange(cin) / (cin - 1.0))) if ramp else torch.ones(cin)
    active = (mag ** 2).sum().item() if chunk is None else CHUNK
    w = _rand(case.cout, cin, k, k, seed=seed + 1, scale=(k * k * active) ** -0.5)
    bias = _rand(case.cout, seed=seed + 2, scale=0.1)
    rs = seed + 10 + 3 * (0 if chunk is None else chunk)
    x = _rand(case.B, cin, case.H, case.W, seed=rs) * mag[None, :, None, None]
    gn = (1.0 + 0.3 * _rand(case.B, cin, seed=rs + 1), 0.3 * _rand(case.B, cin, seed=rs + 2) * mag) if case.pro else None
    if chunk is not None:
        on = torch.zeros(cin)
        on[CHUNK * chunk:CHUNK * chunk + CHUNK] = 1.0
        x = x * on[None, :, None, None]
        if gn is not None:
            gn = (gn[0] * on, gn[1] * on)
    x2 = None
    if case.c1:
        x, x2 = x[:, :case.c0].contiguous(), x[:, case.c0:].contiguous()
    return dict(x=x, x2=x2, w=w, bias=bias, gn=gn)


class Reference(NamedTuple):
    contract: torch.Tensor    # float64, the images of case.images
    top: float                # max |contract|
    d_emul: float             # max |fp32 emulation - contract| / top
    d_mut: float              # the smallest over the run's mutants of max |mutant - contract| / top
    mutants: dict             # product -> its distance


@functools.lru_cache(maxsize=4)
def reference(case: Case, chunk: Optional[int]) -> Reference:
    """contract, d_emul and d_mut of one run, from this file's arithmetic alone.  A run with one active chunk is contracted over
    that chunk only: the other channels' operands are exactly zero in the kernel and here."""
    t = inputs(case, chunk)
    pick = (lambda a: a) if case.images is None else (lambda a: None if a is None else a[list(case.images)].contiguous())
    if case.kind == "att":
        fn = functools.partial(attention, pick(t["qkv"]), case.cin // CHUNK)
        where = slice(None)
    else:
        x = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], dim=1)
        w, gn = t["w"], t["gn"]
        if chunk is not None:
            sl = slice(CHUNK * chunk, CHUNK * chunk + CHUNK)
            x, w, gn = x[:, sl], w[:, sl], (None if gn is None else (gn[0][:, sl], gn[1][:, sl]))
        x, gn = pick(x.contiguous()), (None if gn is None else (pick(gn[0]), pick(gn[1])))
        if case.kind == "wino":
            fn = functools.partial(winograd_3x3, x, w, t["bias"], gn, case.pro, None, case.ups)
        else:
            fn = functools.partial(direct_1x1 if case.kind == "pw" else direct_3x3_s2, x, w, t["bias"])
        where = slice(None)
    em, ct = fn(missing=None)
    top = ct.abs().max().item()
    d_emul = (em - ct).abs().max().item() / top
    mut = {}
    for prod in THIRD_ORDER:
        m = fn(missing=(prod, where))[1]
        mut[prod] = (m - ct).abs().max().item() / top
    return Reference(ct, top, d_emul, min(mut.values()), mut)


SEPARATION = 16.0             # d_mut >= SEPARATION * d_emul for every run (test_bf3_ref_cpu.py)
KERNEL_ROOM = 4.0             # the kernel's bound: max |kernel - contract| / top <= d_mut / KERNEL_ROOM (test_gpu_bf3_terms.py)
