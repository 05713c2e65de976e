"""Which kernel and form every forward convolution of an architecture resolves to, per level ("Other
architectures").  Host only: the executor's convolutions are walked in Python as Fwd::run (unet.cpp) issues them and each is put
to sisic_conv_plan_info with made-up, 16-byte aligned addresses; no device is touched.  Default mode (latency mode forces its own
tile configurations, conv_plan.cpp: conv_latency_cfg).

    python tools/arch_plan_table.py            # markdown table: architectures A - D of tests/arch_ref.py, then the reference's
"""
import ctypes as C
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ["small-Cout", "direct", "pointwise f32", "pointwise bf16x3", "stride-2 bf16x3", "Winograd first", "Winograd second",
           "Winograd third", "Winograd bf16x3"]
PWB_FORMS = ["K-split", "staged", "64 px", "32 px", "staged K-split"]
IN0, IN1, WP, WW, BIAS, GNS, GNH, RES, OUT = (0x10000000 * i for i in range(1, 10))


def plan(B, c0, c1, cout, H, W, k, stride=1, ups=0, gn=False, silu=False, residual=False):
    from synt_isic_amd import _lib
    a = _lib.ConvArgs()
    a.in0, a.c0, a.in1, a.c1 = IN0, c0, (IN1 if c1 else None), c1
    a.B, a.Hin, a.Win, a.upsample, a.ksize, a.stride = B, H, W, ups, k, stride
    a.w_packed, a.bias, a.Cout = WP, BIAS, cout
    # what prepare_conv builds and Fwd::conv passes: Winograd filters for 3x3 stride 1 with Cout > 4, the split filter for stride 2
    a.w_winograd = WW if (k == 3 and (stride == 2 or cout > 4)) else None
    if gn:
        a.gn_scale, a.gn_shift, a.gn_silu = GNS, GNH, int(silu)
    a.residual, a.out = (RES if residual else None), OUT
    kern, cfg, form = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    msg = C.create_string_buffer(256)
    rc = _lib.load().sisic_conv_plan_info(C.byref(a), C.byref(kern), C.byref(cfg), C.byref(form), msg, len(msg))
    if rc != 0:
        return f"REFUSED: {msg.value.decode()}"
    name = KERNELS[kern.value]
    if kern.value == 3:
        name += f" ({PWB_FORMS[form.value]})"
    return f"{name}, cfg {cfg.value}"


def walk(cfg, B, H, W):
    """level -> list of (what, plan) in execution order"""
    boc, n, L = cfg.block_out_channels, len(cfg.block_out_channels), cfg.layers_per_block
    levels = OrderedDict((i, []) for i in range(n))

    def add(i, what, *a, **kw):
        levels[i].append((what, plan(B, *a, **kw)))

    def resnet(i, c0, c1, cout, h, w):
        add(i, f"3x3 {c0}{'+' + str(c1) if c1 else ''}->{cout}", c0, c1, cout, h, w, 3, gn=True, silu=True)
        add(i, f"3x3 {cout}->{cout} +res", cout, 0, cout, h, w, 3, gn=True, silu=True, residual=True)
        if c0 + c1 != cout:
            add(i, f"1x1 {c0}{'+' + str(c1) if c1 else ''}->{cout}", c0, c1, cout, h, w, 1)

    def attention(i, c, h, w):
        add(i, f"1x1 {c}->{3 * c} qkv", c, 0, 3 * c, h, w, 1, gn=True)
        add(i, f"1x1 {c}->{c} +res", c, 0, c, h, w, 1, residual=True)

    add(0, f"3x3 {cfg.in_channels}->{boc[0]} conv_in", cfg.in_channels, 0, boc[0], H, W, 3)
    ch, skips = boc[0], [boc[0]]
    for i in range(n):
        h, w = H >> i, W >> i
        for j in range(L):
            resnet(i, ch, 0, boc[i], h, w)
            ch = boc[i]
            if cfg.down_has_attn[i]:
                attention(i, ch, h, w)
            skips.append(ch)
        if i != n - 1:
            add(i, f"3x3 {ch}->{ch} stride 2", ch, 0, ch, h, w, 3, stride=2)
            skips.append(ch)
    h, w = H >> (n - 1), W >> (n - 1)
    resnet(n - 1, ch, 0, ch, h, w)
    attention(n - 1, ch, h, w)
    resnet(n - 1, ch, 0, ch, h, w)
    for i in range(n):
        lvl = n - 1 - i
        h, w = H >> lvl, W >> lvl
        for j in range(L + 1):
            resnet(lvl, ch, skips.pop(), boc[lvl], h, w)
            ch = boc[lvl]
            if cfg.up_has_attn[i]:
                attention(lvl, ch, h, w)
        if i != n - 1:
            add(lvl, f"3x3 {ch}->{ch} nearest 2x", ch, 0, ch, h, w, 3, ups=1)
    assert not skips
    add(0, f"3x3 {boc[0]}->{cfg.out_channels} conv_out", boc[0], 0, cfg.out_channels, H, W, 3, gn=True, silu=True)
    return levels


def rows(label, cfg, B, H, W):
    out = []
    for i, convs in walk(cfg, B, H, W).items():
        plans = OrderedDict()
        for what, p in convs:
            plans.setdefault(p, []).append(what)
        for p, whats in plans.items():
            uniq = list(OrderedDict.fromkeys(whats))
            out.append((label, f"{H >> i}x{W >> i}", p, len(whats), "; ".join(uniq)))
    return out


def main():
    import arch_ref
    from synt_isic_amd.arch import UNetConfig
    reference = set()
    for B, H, W in ((2, 64, 64), (1, 128, 128), (2, 32, 32), (3, 40, 56)):
        reference |= {r[2] for r in rows("", UNetConfig(), B, H, W)}
    print("| architecture, batch | plane | kernel, tile configuration | launches | convolutions | new |")
    print("|---|---|---|---|---|---|")
    for name, cfg in arch_ref.ARCHS.items():
        for B, H, W in arch_ref.SHAPES[name]:
            for label, plane, p, count, whats in rows(f"{name} {B}x{H}x{W}", cfg, B, H, W):
                print(f"| {label} | {plane} | {p} | {count} | {whats} | {'' if p in reference else 'yes'} |")
    print()
    print("the reference's architecture at 2x64x64, 1x128x128, 2x32x32 and 3x40x56 reaches:")
    for p in sorted(reference):
        print(f"  {p}")


if __name__ == "__main__":
    main()
