"""The plan's side of the staged K-split 1x1 form (tile_cfg 37, conv_plan.cpp): what a forced 37 refuses, that the queries answer
as for the K-split form (tile_cfg 35) on every shape it takes, and which layers the automatic choice routes to it -- none with
SISIC_POINTWISE_STAGED_KSPLIT=0.  Host only: sisic_conv_plan_info and the two queries touch no device, the addresses are made up.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWITCH = "SISIC_POINTWISE_STAGED_KSPLIT"
IN0, IN1, WP, BIAS, GNS, GNH, RES, OUT, STATS = (0x10000000 * i for i in range(1, 10))
FORM_KSPLIT, FORM_STAGED_KSPLIT = 0, 4          # PwbForm, csrc/conv_plan.h
CK_POINTWISE_BF3 = 3                            # ConvKernel


def args(c0, c1, cout, H, W, B=2, cfg=0, gn=False, relu=False):
    from synt_isic_amd._lib import ConvArgs
    a = ConvArgs()
    a.in0, a.c0, a.in1, a.c1 = IN0, c0, (IN1 if c1 else None), c1
    a.B, a.Hin, a.Win = B, H, W
    a.upsample, a.ksize, a.stride = 0, 1, 1
    a.w_packed, a.bias, a.Cout = WP, BIAS, cout
    if gn:
        a.gn_scale, a.gn_shift, a.gn_silu = GNS, GNH, 1
    a.relu = int(relu)
    a.residual, a.out, a.tile_cfg, a.stats_out = RES, OUT, cfg, STATS
    return a


def info(a):
    """(return code, kernel, cfg, form, refusal)"""
    from synt_isic_amd import _lib
    lib = _lib.load()
    k, c, f = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    msg = C.create_string_buffer(256)
    rc = lib.sisic_conv_plan_info(C.byref(a), C.byref(k), C.byref(c), C.byref(f), msg, len(msg))
    return rc, k.value, c.value, f.value, msg.value.decode()


# the shapes the form takes: (c0, c1, Cout, H, W)
TAKEN = [(128, 0, 64, 8, 8), (128, 0, 128, 16, 16), (256, 0, 256, 16, 16), (128, 128, 256, 16, 16), (256, 128, 256, 16, 16),
         (256, 256, 256, 8, 8), (256, 256, 256, 16, 16), (128, 0, 256, 16, 16), (256, 0, 64, 32, 32), (1024, 0, 256, 16, 16)]

# one violated condition each: (what, arguments, a word of the message)
REFUSED = [
    ("Cin not a multiple of 128", dict(c0=192, c1=0, cout=256, H=16, W=16), "multiple of 128 input channels"),
    ("Cin not a multiple of 128, two inputs", dict(c0=128, c1=64, cout=256, H=16, W=16), "multiple of 128 input channels"),
    ("HW not a multiple of 64", dict(c0=128, c1=0, cout=64, H=4, W=8), "whole 64-pixel tiles"),
    ("HW not a multiple of 64, 96 pixels", dict(c0=128, c1=0, cout=64, H=8, W=12), "whole 64-pixel tiles"),
    ("Cout 192", dict(c0=128, c1=0, cout=192, H=16, W=16), "64, 128 or 256 output channels"),
    ("Cout 512", dict(c0=128, c1=0, cout=512, H=16, W=16), "64, 128 or 256 output channels"),
    ("Cout 768", dict(c0=256, c1=0, cout=768, H=16, W=16), "64, 128 or 256 output channels"),
    ("GroupNorm prologue", dict(c0=256, c1=0, cout=256, H=16, W=16, gn=True), "no GroupNorm prologue"),
    ("relu", dict(c0=256, c1=0, cout=256, H=16, W=16, relu=True), "no relu"),
]


@pytest.mark.parametrize("what,kw,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_forced_37_is_refused_with_a_message(what, kw, word):
    rc, kernel, cfg, form, msg = info(args(cfg=37, **kw))
    assert rc == 1, f"{what}: not refused"
    assert msg.startswith("conv2d(pointwise bf16x3") and word in msg, f"{what}: {msg!r}"
    # the same arguments on the K-split form, where it takes them, are not refused: the condition is this form's own
    if kw.get("gn") or kw.get("relu") or kw["cout"] in (192, 512, 768):
        assert info(args(cfg=35, **kw))[0] == 0


def test_lds_need_fits_for_every_shape_taken():
    """the LDS condition cannot be violated alone: the form holds at most 256 channels' operands (96 KB) and one 32-channel block
    of at most sixteen waves' partials (128 KB) -- so every shape that meets the other conditions is taken"""
    for shape in TAKEN:
        rc, kernel, cfg, form, msg = info(args(*shape, cfg=37))
        assert (rc, kernel, cfg, form, msg) == (0, CK_POINTWISE_BF3, 37, FORM_STAGED_KSPLIT, ""), (shape, rc, msg)


def test_queries_answer_as_for_the_ksplit_form():
    from synt_isic_amd import _lib
    lib = _lib.load()
    for shape in TAKEN:
        for B in (1, 2, 64):
            new, old = args(*shape, B=B, cfg=37), args(*shape, B=B, cfg=35)
            assert info(old)[0] == 0
            slots = lib.sisic_conv_stats_slots(C.byref(new))
            assert slots == lib.sisic_conv_stats_slots(C.byref(old)) == shape[3] * shape[4] // 32
            assert lib.sisic_conv_finalizes(C.byref(new)) == lib.sisic_conv_finalizes(C.byref(old)) == 0


def _auto_rows():
    """(c0, c1, Cout, H, B, gn, relu) of the automatic sweep"""
    rows = []
    for c0, c1 in ((128, 0), (256, 0), (256, 128), (256, 256), (512, 0), (1024, 0)):
        for cout in (64, 128, 256):
            for H in (8, 16, 32):
                for B in (1, 2, 32, 64, 65, 128):
                    for gn, relu in ((False, False), (True, False), (False, True)):
                        rows.append((c0, c1, cout, H, B, gn, relu))
    return rows


def _auto_forms():
    return [info(args(c0, c1, cout, H, H, B=B, gn=gn, relu=relu))[1:4] for c0, c1, cout, H, B, gn, relu in _auto_rows()]


def routed(c0, c1, cout, H, B, gn, relu):
    """the routing rule as DESIGN.md section 4 states it"""
    return (not gn and not relu and H == 16 and cout == 256 and c0 + c1 <= 512 and (B * 4) % 256 == 0) if ROUTING_ON else False


# whether the measurement admitted any shape (profiles/r23): the rule above is then the whole routing
ROUTING_ON = True


def test_automatic_choice_follows_the_measured_rule():
    assert os.environ.get(SWITCH) is None and os.environ.get("SISIC_POINTWISE_KSPLIT") is None
    for r, (kernel, cfg, form) in zip(_auto_rows(), _auto_forms()):
        assert kernel == CK_POINTWISE_BF3 and cfg == 28, r
        assert (form == FORM_STAGED_KSPLIT) == routed(*r), (r, form)
        if form != FORM_STAGED_KSPLIT and routed(*r[:5], False, False):
            assert form == FORM_KSPLIT, r        # a prologue or relu keeps the layer on the K-split form


def test_switch_off_restores_the_dispatch():
    """in a fresh process (the switches are read once): no row of the sweep is the new form, and every row that is the new form
    with the switch on is the K-split form with it off; all other rows are unchanged"""
    env = dict(os.environ)
    env[SWITCH] = "0"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--auto-forms"], env=env, check=True, capture_output=True, text=True)
    off = [tuple(v) for v in json.loads(out.stdout)]
    on = _auto_forms()
    assert len(off) == len(on)
    for r, a, b in zip(_auto_rows(), on, off):
        assert b[2] != FORM_STAGED_KSPLIT, r
        assert b == ((a[0], a[1], FORM_KSPLIT) if a[2] == FORM_STAGED_KSPLIT else a), (r, a, b)


if __name__ == "__main__":
    if "--auto-forms" in sys.argv:
        print(json.dumps(_auto_forms()))
