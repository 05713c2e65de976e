"""What a convolution's plan promises its caller -- sisic_conv_stats_slots() and sisic_conv_finalizes() -- pinned over a fixed
grid of argument sets.  Both queries are pure host code: they touch no device, so the addresses are made up (non-null, aligned
as a row says).

tests/golden/conv_plan_answers.json holds the answers of the library as it was BEFORE the dispatch was gathered into one
ConvPlan (conv_plan.cpp); the grid and the recorder below are the ones that recording was made with:
    SISIC_LIB_PATH=<library to record from> python tests/test_conv_plan_cpu.py --record
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plan_answers.json")

BATCHES = (1, 2, 64)
CINS = (3, 64, 72, 128, 256, 384, 512)
COUTS = (3, 18, 64, 128, 256, 768)
PLANES = tuple((n, n) for n in (4, 5, 7, 8, 12, 14, 16, 28, 32, 56, 64)) + ((4, 16), (24, 40))
# (ksize, stride, upsample): every pair the library takes, upsample where stride 1 allows it -- and 1x1 with upsample, which it refuses
KSU = ((1, 1, 0), (1, 1, 1), (1, 2, 0), (3, 1, 0), (3, 1, 1), (3, 1, 2), (3, 2, 0), (7, 2, 0))
# every tile configuration the dispatch names, and two it does not
CFGS = tuple(range(1, 37)) + (41, 42, 50, 51, 52) + tuple(range(60, 75)) + (78, 79, 90, 91, 92, 43, 99)
SWITCHES = ("SISIC_WINO_WIDE", "SISIC_WINO_BF16X3", "SISIC_KSPLIT", "SISIC_POINTWISE", "SISIC_POINTWISE_BF16X3", "SISIC_S2_BF16X3")

IN0, IN1, WP, WW, BIAS, GNS, GNH, RES, OUT, STATS = (0x10000000 * i for i in range(1, 11))
FG, FB, FS, FH = (0x10000000 * i for i in range(11, 15))


def family(cfg):
    """the (ksize, stride) a configuration number belongs to"""
    if 11 <= cfg <= 13 or cfg in (18, 19, 36):
        return (3, 2)
    if 20 <= cfg <= 30 or cfg in (34, 35):
        return (1, 1)
    if 31 <= cfg <= 33:
        return (1, 2)
    if cfg in (41, 42):
        return (7, 2)
    return (3, 1)


def row(k, s, ups, wino, two, cin, cout, plane, gn, cfg=0, off=(0, 0, 0), res=True, per_group=8):
    return (k, s, ups, wino, two, cin, cout, plane[0], plane[1], gn, cfg, off[0], off[1], off[2], int(res), per_group)


def grid():
    rows = []
    # A: the automatic choice over every shape
    for k, s, ups in KSU:
        for wino in ((0, 1) if k == 3 else (0,)):
            for two in (0, 1):
                for cin in CINS:
                    for cout in COUTS:
                        for plane in PLANES:
                            for gn in (0, 1):
                                rows.append(row(k, s, ups, wino, two, cin, cout, plane, gn))
    n_auto = len(rows)
    # B: every configuration number: on its own (ksize, stride) over a set of shapes, on every other pairing once
    shapes = ((3, 64), (64, 3), (72, 64), (128, 256), (256, 128), (512, 768), (384, 18))
    planes = ((4, 4), (7, 7), (8, 8), (12, 12), (16, 16), (32, 32), (64, 64), (24, 40))
    for cfg in CFGS:
        for k, s, ups in KSU:
            if (k, s) != family(cfg):
                rows.append(row(k, s, ups, 1, 0, 128, 256, (8, 8), 0, cfg))
                continue
            for wino in ((0, 1) if k == 3 else (1,)):
                for cin, cout in shapes:
                    for plane in planes:
                        i = len(rows)
                        rows.append(row(k, s, ups, wino, i % 2, cin, cout, plane, (i // 2) % 2, cfg))
    # C: residual / out / stats_out off their 16-byte alignment, 8 and 4 channels per GroupNorm group, with and without a residual
    offs = tuple((a, b, c) for a in (0, 4, 8) for b in (0, 4, 8) for c in (0, 4, 8))
    for k, cfgs in ((3, (0, 74, 90, 91, 92)), (1, (0, 20, 28))):
        for cfg in cfgs:
            for plane in ((8, 8), (16, 16)):
                for cin, cout in ((128, 128), (256, 256), (512, 256)):
                    for per_group in (8, 4):
                        for res in (True, False):
                            for off in offs:
                                rows.append(row(k, 1, 0, 1, 0, cin, cout, plane, 1, cfg, off, res, per_group))
    return rows, n_auto


def switch_rows():
    """the part of the automatic sweep asked again with one dispatch switch off"""
    rows, n_auto = grid()
    return [r for r in rows[:n_auto] if r[5] in (128, 256) and (r[7], r[8]) in ((8, 8), (16, 16), (32, 32))]


def grid_digest(rows):
    return hashlib.sha256(json.dumps(rows).encode()).hexdigest()


def make_args(r, B):
    from synt_isic_amd._lib import ConvArgs
    k, s, ups, wino, two, cin, cout, H, W, gn, cfg, o_res, o_out, o_st, res, per_group = r
    a = ConvArgs()
    c1 = 0
    if two:
        c1 = cin // 2 // 8 * 8 if cin >= 16 else cin // 2
    a.in0, a.c0 = IN0, cin - c1
    a.in1, a.c1 = (IN1 if two else None), c1
    a.B, a.Hin, a.Win = B, H, W
    a.upsample, a.ksize, a.stride = ups, k, s
    a.w_packed, a.bias, a.Cout = WP, BIAS, cout
    if gn:
        a.gn_scale, a.gn_shift, a.gn_silu = GNS, GNH, 1
    if res:
        a.residual = RES + o_res
    a.out = OUT + o_out
    a.tile_cfg = cfg
    a.w_winograd = WW if wino else None
    a.stats_out = STATS + o_st
    if cout % per_group == 0:
        a.fin_gamma, a.fin_beta, a.fin_groups, a.fin_eps = FG, FB, cout // per_group, 1e-5
        a.fin_scale, a.fin_shift = FS, FH
    return a


def answers(rows, batches=BATCHES):
    """slots * 2 + finalizes per row; the queries must not depend on the batch (an image's bits do not depend on its batch)"""
    import ctypes as C
    from synt_isic_amd import _lib
    lib = _lib.load()
    out = []
    for r in rows:
        got = set()
        for B in batches:
            a = make_args(r, B)
            slots_with = lib.sisic_conv_stats_slots(C.byref(a))
            fin = lib.sisic_conv_finalizes(C.byref(a))
            assert fin in (0, 1) and slots_with >= 0, (r, B, slots_with, fin)
            got.add(slots_with * 2 + fin)
        assert len(got) == 1, f"the answers depend on the batch: row {r}: {sorted(got)}"
        out.append(got.pop())
    return out


def encode(values):
    """one character per row: its index in the sorted list of distinct answers"""
    distinct = sorted(set(values))
    assert len(distinct) < 90
    return {"distinct": distinct, "rows": "".join(chr(35 + distinct.index(v)) for v in values)}


def decode(doc):
    return [doc["distinct"][ord(c) - 35] for c in doc["rows"]]


def child_answers(switch):
    """one switch off, in a fresh process that only makes these queries (the switches are read once per process)"""
    env = dict(os.environ)
    for name in SWITCHES:
        env.pop(name, None)
    env[switch] = "0"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--switch-answers"], env=env, check=True, capture_output=True, text=True)
    return json.loads(out.stdout)


def record():
    rows, _ = grid()
    ans = answers(rows)
    # conditions on the recording.  Two families finalise: the K-split 8x8 forms (tile_cfg 90 .. 92, or chosen below 12x12) and
    # tile_cfg 74 where one 16x16 tile holds the image (forced, or chosen from 12x12 up)
    def through_74(r):
        return r[10] == 74 or (r[10] == 0 and (r[7] << (1 if r[2] else 0)) >= 12)
    fin64 = sum(1 for r, v in zip(rows, ans) if v & 1 and not through_74(r))
    fin74 = sum(1 for r, v in zip(rows, ans) if v & 1 and through_74(r))
    assert all(r[10] in (0, 74, 90, 91, 92) for r, v in zip(rows, ans) if v & 1)
    zero = sum(1 for v in ans if v >> 1 == 0)
    print(f"{len(rows)} rows: {fin64} finalise through the K-split 8x8 forms, {fin74} through the single-tile cfg 74, {zero} have no slots")
    assert fin64 >= 100 and fin74 >= 30 and zero >= 100
    switch_off = {sw: child_answers(sw) for sw in SWITCHES}
    index = {r: i for i, r in enumerate(rows)}
    for sw, off in switch_off.items():
        print(f"{sw}=0 changes {sum(1 for r, v in zip(switch_rows(), off) if v != ans[index[r]])} of {len(off)} rows")
    doc = {"grid_sha256": grid_digest(rows), "rows": len(rows), "answers": encode(ans), "switch_rows_sha256": grid_digest(switch_rows()),
           "switch_off": {sw: encode(v) for sw, v in switch_off.items()}}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes")


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _first_differences(rows, got, want, limit=8):
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    return f"{len(bad)} of {len(rows)} rows differ; (row, slots*2+fin now, recorded): {bad[:limit]}"


def test_plan_answers_are_the_recorded_ones(fixture):
    for name in SWITCHES:
        assert os.environ.get(name) is None, f"{name} is set: the recording was made with every switch at its default"
    rows, _ = grid()
    assert grid_digest(rows) == fixture["grid_sha256"] and len(rows) == fixture["rows"], "the grid is not the recorded one"
    want = decode(fixture["answers"])
    got = answers(rows)          # (asserts batch independence row by row)
    assert got == want, _first_differences(rows, got, want)


@pytest.mark.parametrize("switch", SWITCHES)
def test_plan_answers_with_a_switch_off(fixture, switch):
    rows = switch_rows()
    assert grid_digest(rows) == fixture["switch_rows_sha256"]
    want = decode(fixture["switch_off"][switch])
    got = child_answers(switch)
    assert got == want, _first_differences(rows, got, want)


if __name__ == "__main__":
    if "--switch-answers" in sys.argv:
        print(json.dumps(answers(switch_rows(), batches=(2,))))
    elif "--record" in sys.argv:
        record()
