// conv_plan.cpp -- the one place that decides which kernel runs a convolution (conv_plan.h).
#include "conv_plan.h"
#include "poison_switch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace sisic {

namespace {

// the dispatch switches: each read once per process, on unless set to 0
struct Switches { bool wino_wide, wino_bf3, wino_col, ksplit, pointwise, pointwise_bf3, pointwise_ksplit, s2_bf3, pointwise_staged_ksplit; };
const Switches& switches() {
    static const Switches sw{env_on("SISIC_WINO_WIDE"), env_on("SISIC_WINO_BF16X3"), env_on("SISIC_WINO_COL"), env_on("SISIC_KSPLIT"),
                             env_on("SISIC_POINTWISE"), env_on("SISIC_POINTWISE_BF16X3"), env_on("SISIC_POINTWISE_KSPLIT"), env_on("SISIC_S2_BF16X3"),
                             env_on("SISIC_POINTWISE_STAGED_KSPLIT")};
    return sw;
}

}  // namespace

// the allocation test switch (poison_switch.h, workspace.h): off unless set to a non-zero number
bool poison_alloc() {
    static const bool on = [] { const char* e = std::getenv("SISIC_POISON_ALLOC"); return e && std::atoi(e) != 0; }();
    return on;
}

namespace {

struct DirectTiling { int cfg, ks, stride, tw, th, wn; };
constexpr DirectTiling DIRECT[] = {
#define X(id, KS, STRIDE, MT, NT, WM, WN, TW, CIC, OCC, KSP) {id, KS, STRIDE, TW, WN * NT * 32 / TW, WN},
    SISIC_DIRECT_TILINGS(X)
#undef X
};
const DirectTiling* direct_row(int cfg) { for (const DirectTiling& t : DIRECT) if (t.cfg == cfg) return &t; return nullptr; }

//  cfg                      geometry  imgs waves stagger col ksplit tile  profile slot
constexpr WinoCfg WINO[] = {
    {CFG_WINO_1IMG_8W,       WG_FIRST,  1,  8, false,  0,  0, 16, 16, -1},
    {CFG_WINO_4IMG_8W,       WG_FIRST,  4,  8, false,  0,  0,  8,  8, -1},
    {CFG_WINO_1IMG_16W,      WG_FIRST,  1, 16, false,  0,  0, 16, 16, -1},
    {CFG_WINO_4IMG_16W,      WG_FIRST,  4, 16, false,  0,  0,  8,  8, -1},
    {CFG_WINO_1IMG_8W_STAG,  WG_FIRST,  1,  8, true,   0,  0, 16, 16, -1},
    {CFG_WINO_4IMG_8W_STAG,  WG_FIRST,  4,  8, true,   0,  0,  8,  8, -1},
    {CFG_WINO_1IMG_16W_STAG, WG_FIRST,  1, 16, true,   0,  0, 16, 16, PK_WINO_MAIN},
    {CFG_WINO_4IMG_16W_STAG, WG_FIRST,  4, 16, true,   0,  0,  8,  8, -1},
    {CFG_WINO_WIDE128,       WG_SECOND, 1, 16, false, -1,  0,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_WIDE64,        WG_SECOND, 1,  8, false, -1,  0,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_COL128,        WG_SECOND, 1, 16, false,  1,  0,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_COL64,         WG_SECOND, 1,  8, false,  1,  0,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_SECOND128,     WG_SECOND, 1, 16, false,  0,  0,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_SECOND64,      WG_SECOND, 1,  8, false,  0,  0,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_BF3,           WG_BF3,    1, 16, false,  0,  0, 16, 16, PK_WINO_BF3},
    {CFG_WINO_LATENCY128,    WG_SECOND, 1, 16, false, -1, -1,  8, 16, PK_WINO_MAIN},
    {CFG_WINO_LATENCY64,     WG_SECOND, 1,  8, false, -1, -1,  8, 16, PK_WINO_MAIN},
    {CFG_KSPLIT8_FIRST,      WG_FIRST,  4, 16, true,   0,  4,  8,  8, -1},
    {CFG_KSPLIT8_PAIR,       WG_SECOND, 2, 16, false, -1,  4,  8,  8, -1},
    {CFG_KSPLIT8_BF3,        WG_BF3,    4, 16, false,  0,  4,  8,  8, -1},
};

// Winograd F(2x2,3x3) is taken for 3x3 stride-1 convolutions with transformed filters at hand: when forced by one of the
// configurations of the table above, or automatically from 12x12 outputs up and (K-split forms) at the 8x8 level (per-thread
// load offsets there are 32-bit).  Returns the tile configuration, 0 = not Winograd.
// (no batch-size condition anywhere in this function: an image's bits must not depend on the batch it is in)
int winograd_cfg(const sisic_conv_args& a, int Hout, int Wout) {
    if (!(a.ksize == 3 && a.stride == 1 && a.w_winograd != nullptr && a.Cout > 4) || a.upsample == 2) return 0;
    if (wino_cfg_row(a.tile_cfg)) return a.tile_cfg;
    if (a.tile_cfg != 0) return 0;
    const Switches& sw = switches();
    const int Cin = a.c0 + a.c1;
    if (16.0 * std::max(a.c0, a.c1) * a.Hin * a.Win >= 4294967296.0) return 0;
    if (Hout >= 12 && Wout >= 12) {
        // fp32-equivalent products on the bf16 matrix pipe (conv_winograd_bf3.inc) unless SISIC_WINO_BF16X3=0: 64 channels x
        // 16 x 16 pixels per workgroup, so only where those tiles are (nearly) full; measured 1.36 - 1.43x the third f32 form on every
        // such layer of the headline model (profiles/r03/conv_bench_bf16x3.txt), the same error against float64
        // (ragged planes too when at least three quarters of the 16x16-pixel tiles' area is inside: the classifier's 56 / 28 / 14)
        const int th = (Hout + 15) / 16 * 16, tw = (Wout + 15) / 16 * 16;
        // (nearest-2x inputs as well: all 16 positions on the bf16 pipe beat the f32 form's 9 on every upsample layer of the
        //  UNet -- 562 -> 512 us over the three, profiles/r03/conv_bench_bf16x3.txt)
        // (Cin <= 2048: its LDS table of the image's GroupNorm operands)
        const bool bf3_takes = a.Cout % 64 == 0 && 4 * Hout * Wout >= 3 * th * tw && Cin >= 16 && Cin <= 2048 && 4.0 * a.Cout * Hout * Wout < 2147483648.0;
        if (sw.wino_bf3 && bf3_takes) return CFG_WINO_BF3;
        // second geometry (conv_winograd_wide.inc) unless SISIC_WINO_WIDE=0; nearest-2x inputs keep the nine-position form.
        // Measured per layer (tools/conv_bench.py, profiles/r02/conv_bench_geometries.txt): the 128-channel form wins 8-12 % on
        // every Cout >= 128 layer, the 64-channel two-workgroups-per-CU form 1-10 % on every Cout <= 64 layer
        if (sw.wino_wide && !a.upsample) return a.Cout > 64 ? CFG_WINO_WIDE128 : CFG_WINO_WIDE64;
        return CFG_WINO_1IMG_16W_STAG;
    }
    // the 8x8 level (and the classifier's 7x7): four images per workgroup and the input channels split four ways keep all CUs busy
    if (sw.ksplit && Hout <= 8 && Wout <= 8 && Hout >= 5 && Wout >= 5 && Cin >= 128 && Cin % 32 == 0 && a.Cout >= 128) {
        // the same split with fp32-equivalent products on the bf16 pipe, four images per workgroup
        // (conv_winograd_bf3.inc): 38 -> 32 and 59 -> 47 us per launch at B = 64 (profiles/r03/conv_bench_bf16x3.txt)
        if (sw.wino_bf3 && !a.upsample && a.Cout % 64 == 0 && Cin <= 512) return CFG_KSPLIT8_BF3;
        // second geometry with two images per workgroup: 45 -> 39 us and 67 -> 57 us per launch at B = 64
        return (sw.wino_wide && !a.upsample) ? CFG_KSPLIT8_PAIR : CFG_KSPLIT8_FIRST;
    }
    return 0;
}

// the first refusal is the one reported
#define PLAN_REFUSE_UNLESS(cond, ...) do { if (!(cond) && !pl.refusal[0]) std::snprintf(pl.refusal, sizeof pl.refusal, __VA_ARGS__); } while (0)

void plan_winograd(const sisic_conv_args& a, ConvPlan& pl) {
    const WinoCfg& w = *wino_cfg_row(pl.cfg);
    const int Hout = pl.Hout, Wout = pl.Wout, Cin = a.c0 + a.c1;
    const bool third = w.col < 0 ? switches().wino_col : w.col == 1;
    const bool fits32 = 4.0 * std::max(a.c0, a.c1) * a.Hin * a.Win * (w.geom == WG_FIRST ? w.imgs : 1) < 4294967296.0;
    PLAN_REFUSE_UNLESS(fits32, "conv2d(winograd): per-thread load offsets are 32-bit; this tensor needs the direct kernel");
    pl.ksplit = w.ksplit < 0 ? wino_latency_ksplit(a.Cout, Cin, Hout, Wout) : std::max(w.ksplit, 1);
    pl.stats_slots = cdiv(Hout, w.tile_h) * cdiv(Wout, w.tile_w);
    pl.kernel = w.geom == WG_FIRST ? CK_WINO_FIRST : w.geom == WG_BF3 ? CK_WINO_BF3 : third ? CK_WINO_THIRD : CK_WINO_SECOND;
    if (w.geom == WG_SECOND && w.ksplit != 4) PLAN_REFUSE_UNLESS(!a.upsample, "conv2d(winograd wide): no upsample form");
    // F(2x2,3x3) multiplies 16 positions per 2x2 outputs instead of 36 taps, and only 9 of them for nearest-2x inputs
    // (conv_winograd.hip, upsample form: tile_cfg 66 without a GroupNorm prologue)
    const bool ups9 = a.upsample && !a.gn_scale && pl.cfg == CFG_WINO_1IMG_16W_STAG;
    pl.issued_flops = pl.flops * (ups9 ? 9.0 : 16.0) / 36.0;
    pl.profile_slot = ups9 ? -1 : w.profile_slot;
    // Where a workgroup holds whole GroupNorm groups (eight channels) of an image it finalizes them (sisic_conv_finalizes)
    const bool fin_asked = a.fin_gamma && a.fin_groups > 0 && a.Cout % a.fin_groups == 0 && a.Cout / a.fin_groups == 8;
    if (w.ksplit < 0 && pl.ksplit > 1) {            // latency mode: partial slabs summed by the plane reduction, a slot per segment
        pl.stats_slots = wino_latency_segments(Hout, Wout);
    } else if (w.ksplit == 4) {
        pl.stats_slots = 1;                         // one per image, from the reduction
        const bool ok = Hout * Wout <= 256 && (cdiv(Cin, 8) % 4) == 0, plain8 = !a.upsample && Hout <= 8 && Wout <= 8;
        PLAN_REFUSE_UNLESS(ok, "conv2d(winograd K-split): needs <= 256 output pixels per image and a multiple of %d input channels", 4 * 8);
        if (pl.cfg == CFG_KSPLIT8_BF3) PLAN_REFUSE_UNLESS(plain8, "conv2d(winograd bf16x3, 8x8): plain stride-1 convolutions of at most 8x8 pixels");
        if (pl.cfg == CFG_KSPLIT8_PAIR) PLAN_REFUSE_UNLESS(plain8, "conv2d(winograd wide, image pairs): plain stride-1 convolutions of at most 8x8 pixels");
        // the 16-byte form of the reduction: 16 whole channel planes of 64 pixels per workgroup, two whole groups (conv_winograd.hip,
        // ReduceFin).  (Its scratch slabs are the library's own allocation, aligned as hipMalloc aligns.)
        const bool al16 = ((reinterpret_cast<uintptr_t>(a.residual) | reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.stats_out)) & 15) == 0;
        pl.form = (Hout * Wout == 64 && al16) ? REDUCE_64PX : REDUCE_ANY;
        pl.finalizes = fin_asked && pl.form == REDUCE_64PX && a.Cout % 16 == 0;
    } else if (pl.cfg == CFG_WINO_BF3) {
        // the bf16x3 kernel where ONE 16x16-pixel tile is the whole image: a workgroup holds 64 channels of an image whole
        pl.finalizes = fin_asked && !a.upsample && Hout <= 16 && Wout <= 16 && a.Cout % 64 == 0;
    }
    if (pl.finalizes) PLAN_REFUSE_UNLESS(a.fin_beta && a.fin_scale && a.fin_shift, "conv2d: fin_gamma given without fin_beta / fin_scale / fin_shift");
}

// The layers the automatic choice gives to the staged K-split form (conv_pwbsk_kernel) instead of the K-split form -- unless
// SISIC_POINTWISE_STAGED_KSPLIT=0.  By layer shape and batch; both forms give the same bits.  Measured, the two forms alternated
// twice (profiles/r23/conv_bench_pointwise_staged_ksplit.txt), at batch 64 / 128, K-split vs staged K-split in us:
//   256 -> 256 @16 + residual 30.4 - 31.6 vs 22.8 - 24.2 / 54.4 - 54.9 vs 42.0 - 42.4;   256 + 256 -> 256 @16 38.2 - 39.8 vs 32.0 - 32.4 / 72 vs 62;
//   256 + 128 -> 256 @16 32.6 vs 25.7 / 57.8 vs 48.8;   128 -> 256 @16 16.9 vs 14.6 / 29.3 vs 25.7
// -- the 16x16 level's 256-channel layers with whole rounds of one workgroup per CU (256 CUs), which is what was measured.
// NOT routed, slower there: 256 + 128 -> 128 @32 (58.9 vs 65.2: eight waves and 48 KB leave the CU to one workgroup's latencies) and
// 256 + 256 -> 256 @8 (13.6 vs 23.5: 64 workgroups for 256 CUs).
bool pwbsk_routed(const sisic_conv_args& a, bool ks_ok) {
    const int HW = a.Hin * a.Win, Cin = a.c0 + a.c1;
    const int64_t nwg = (int64_t)a.B * (HW / 64);
    return switches().pointwise_staged_ksplit && switches().pointwise_ksplit && ks_ok && a.gn_scale == nullptr && !a.relu && HW == 256 && a.Cout == 256 &&
           Cin <= 512 && nwg >= 256 && nwg % 256 == 0;
}

// 1x1 stride 1 with fp32-equivalent products on the bf16 matrix pipe: which of the kernel's forms
void plan_pointwise_bf3(const sisic_conv_args& a, ConvPlan& pl) {
    const int HW = a.Hin * a.Win, Cin = a.c0 + a.c1;
    pl.kernel = CK_POINTWISE_BF3; pl.cfg = a.tile_cfg ? a.tile_cfg : CFG_PWB; pl.stats_slots = HW / 32;      // one slot per 32 pixels, every form
    // the staged K-split form (tile_cfg 37 forces it): one workgroup per 64-pixel tile, waves = channel items x K quarters, the
    // tile's operands split once into LDS.  The bits of the K-split form, so the choice between the two may depend on the batch.
    // (Its own conditions first: theirs is the message a forced 37 reports.)
    if (a.tile_cfg == CFG_PWB_STAGED_KSPLIT) {
        PLAN_REFUSE_UNLESS((Cin / 8) % (4 * PWB_WAVES) == 0, "conv2d(pointwise bf16x3, staged K-split): tile_cfg 37 needs a multiple of 128 input channels");
        PLAN_REFUSE_UNLESS(HW % 64 == 0, "conv2d(pointwise bf16x3, staged K-split): tile_cfg 37 needs whole 64-pixel tiles");
        PLAN_REFUSE_UNLESS(a.Cout == 64 || a.Cout == 128 || a.Cout == 256, "conv2d(pointwise bf16x3, staged K-split): tile_cfg 37 needs 64, 128 or 256 output channels");
        PLAN_REFUSE_UNLESS(a.gn_scale == nullptr, "conv2d(pointwise bf16x3, staged K-split): tile_cfg 37 has no GroupNorm prologue");
        PLAN_REFUSE_UNLESS(!a.relu, "conv2d(pointwise bf16x3, staged K-split): tile_cfg 37 has no relu");
        PLAN_REFUSE_UNLESS(a.Cout % 64 != 0 || pwbsk_lds_bytes(Cin, a.Cout) <= PWBSK_MAX_LDS, "conv2d(pointwise bf16x3, staged K-split): tile_cfg 37 needs %zu bytes of LDS", pwbsk_lds_bytes(Cin, a.Cout));
    }
    PLAN_REFUSE_UNLESS(conv_pointwise_bf3_applicable(a), "conv2d(pointwise bf16x3): shape not supported by tile_cfg 28");
    // the K-split form (tile_cfg 35 forces it) for the 16x16 and 8x8 levels' layers of up to 256 output channels -- by SHAPE only:
    // its bits are its own.  Measured at batch 64 (profiles/r04/conv_bench_pointwise_forms.txt): 256 -> 256 @16 27.3 vs 34.2 us,
    // 512 -> 256 @8 13.5 vs 24.9, 512 -> 256 @16 38.0 vs 38.7; NOT for 256 -> 768 (76.8 vs 50.7: twelve channel items already
    // fill the chip, and four waves per item fetch the item's filters in four strands)
    const bool ks_ok = (Cin / 8) % (4 * PWB_WAVES) == 0;        // (whole groups of four chunks per wave; the concat seam lies on a chunk boundary)
    // the staged form (tile_cfg 34 forces it) where a layer has 6 .. 12 channel items and enough 64-pixel workgroups for the chip
    // (the choice depends on the batch; the bits do not)
    const bool staged_ok = a.Cout / 64 >= 6 && a.Cout / 64 <= PWBS_MAX_WAVES && pwbs_lds_bytes(Cin) <= 150 * 1024;
    if (a.tile_cfg == CFG_PWB_KSPLIT) PLAN_REFUSE_UNLESS(ks_ok, "conv2d(pointwise bf16x3, K-split): tile_cfg 35 needs a multiple of 128 input channels");
    if (a.tile_cfg == CFG_PWB_STAGED) PLAN_REFUSE_UNLESS(staged_ok, "conv2d(pointwise bf16x3, staged): tile_cfg 34 needs 384 .. 768 output channels and at most %d input channels", (150 * 1024) / 392);
    if (a.tile_cfg == CFG_PWB_STAGED_KSPLIT || (a.tile_cfg == 0 && pwbsk_routed(a, ks_ok))) pl.form = PWB_FORM_STAGED_KSPLIT;
    else if (a.tile_cfg == CFG_PWB_KSPLIT || (a.tile_cfg == 0 && ks_ok && HW <= 256 && a.Cout <= 256 && switches().pointwise_ksplit)) pl.form = PWB_FORM_KSPLIT;
    else if (a.tile_cfg == CFG_PWB_STAGED || (a.tile_cfg == 0 && staged_ok && (int64_t)a.B * (HW / 64) >= 128)) pl.form = PWB_FORM_STAGED;
    // 64-pixel items where they give every SIMD at least two waves (1024 SIMDs), 32-pixel items otherwise: a lone wave has
    // nobody to hide its latencies.  (The choice depends on the batch; the bits of an output do not: its chain of MFMAs is the same.)
    else if (a.tile_cfg == CFG_PWB_64PX || (a.tile_cfg != CFG_PWB_32PX && (int64_t)a.B * (HW / 64) * (a.Cout / 64) >= 2048)) pl.form = PWB_FORM_64PX;
    else pl.form = PWB_FORM_32PX;
    // rider jobs go with the instances without a GroupNorm prologue of the two four-wave kernels and with the staged K-split form
    // (conv_pointwise_bf3.hip)
    pl.carries_rider = a.gn_scale == nullptr && pl.form != PWB_FORM_STAGED;
}

// everything but Winograd: SISIC_EINVAL for arguments no kernel takes
int plan_direct(const sisic_conv_args& a, ConvPlan& pl) {
    const Switches& sw = switches();
    int cfg = a.tile_cfg;
    SISIC_REQUIRE(!wino_cfg_row(cfg), "conv2d: tile_cfg %d needs w_winograd, ksize 3 and stride 1", cfg);
    int Ht = pl.Hout, Wt = pl.Wout;             // the plane as the direct kernel tiles it
    if (a.ksize == 7) {
        if (cfg == 0) cfg = 41;
    } else if (a.ksize == 1 && a.stride == 2) {
        if (cfg == 0) cfg = Wt >= 24 ? 31 : (Wt >= 12 ? 32 : 33);
    } else if (a.ksize == 1) {
        SISIC_REQUIRE(!a.upsample, "conv2d: 1x1 with upsample");
        // fp32-equivalent products on the bf16 matrix pipe (conv_pointwise_bf3.hip) for whole 64-pixel x 64-channel tiles --
        // unless SISIC_POINTWISE_BF16X3=0.  (Shape conditions only: an image's bits must not depend on the batch it is in.)
        const bool pwb_forced = (cfg >= CFG_PWB && cfg <= CFG_PWB_64PX) || cfg == CFG_PWB_STAGED || cfg == CFG_PWB_KSPLIT || cfg == CFG_PWB_STAGED_KSPLIT;
        if (pwb_forced || (cfg == 0 && sw.pointwise_bf3 && conv_pointwise_bf3_applicable(a))) {
            plan_pointwise_bf3(a, pl);
            return SISIC_OK;
        }
        // the lean pointwise kernel (conv_pointwise.hip) for the shapes it takes -- whole 128-pixel tiles and 32-channel chunks --
        // unless SISIC_POINTWISE=0; the generic tilings below for everything else
        if ((cfg == 0 && sw.pointwise && conv_pointwise_applicable(a)) || cfg == CFG_POINTWISE) {
            pl.kernel = CK_POINTWISE; pl.cfg = CFG_POINTWISE; pl.stats_slots = a.Hin * a.Win / 32;                // one slot per 32 pixels
            PLAN_REFUSE_UNLESS(conv_pointwise_applicable(a), "conv2d(pointwise): shape not supported by tile_cfg 20");
            return SISIC_OK;
        }
        Ht = 1; Wt = a.Hin * a.Win;             // the image is a flat row of H*W pixels
        if (cfg == 0) cfg = (Wt <= 64) ? 22 : (Wt <= 256 ? 25 : 24);   // measured (tools/conv_bench.py, B=64)
    } else if (a.stride == 1) {
        if (cfg == 0) cfg = Wt >= 24 ? 8 : (Wt >= 12 ? 9 : 16);   // measured (tools/conv_bench.py, B=64)
    } else {
        // fp32-equivalent products on the bf16 matrix pipe (conv_s2_bf3.hip) where a split filter was supplied -- unless
        // SISIC_S2_BF16X3=0.  (Conditions on the arguments' shape only: an image's bits must not depend on the batch it is in.)
        if ((cfg == 0 && sw.s2_bf3 && conv_s2_bf3_applicable(a)) || cfg == CFG_S2_BF3) {
            const bool ok = conv_s2_bf3_applicable(a);
            pl.kernel = CK_S2_BF3; pl.cfg = CFG_S2_BF3; pl.stats_slots = ok ? conv_s2_bf3_stats_slots(a) : 0;
            PLAN_REFUSE_UNLESS(ok, "conv2d(stride-2 bf16x3): tile_cfg 36 needs ksize 3, stride 2, one input without GroupNorm prologue, Cin %% 8 == 0, Cout %% 64 == 0 and the split filter (sisic_conv_s2_pack) in w_winograd");
            return SISIC_OK;
        }
        if (cfg == 0) cfg = Wt >= 24 ? 11 : (Wt >= 12 ? 12 : 18);   // measured (tools/conv_bench.py, B=64; 16->8: 66 -> 57 us)
    }
    const DirectTiling* t = direct_row(cfg);
    SISIC_REQUIRE(t && t->ks == a.ksize && t->stride == a.stride, "conv2d: tile_cfg %d invalid for ksize %d stride %d", cfg, a.ksize, a.stride);
    const int tiles = cdiv(Wt, t->tw) * cdiv(Ht, t->th);
    const int64_t nwg = (int64_t)a.B * tiles * (conv_cout_pad(a.Cout) / CONV_CO_TILE);
    SISIC_REQUIRE(nwg > 0 && nwg < (int64_t(1) << 31), "conv2d: grid of %lld workgroups unsupported", (long long)nwg);
    pl.kernel = CK_DIRECT; pl.cfg = cfg; pl.stats_slots = tiles * t->wn;             // one slot per pixel tile and pixel-wave
    return SISIC_OK;
}

// the kernel, its configuration and what the launch promises
int choose(const sisic_conv_args& a, ConvPlan& pl) {
    // conv_out: the vector-ALU kernel (conv_small.hip); it leaves no GroupNorm partials
    if (a.ksize == 3 && a.stride == 1 && !a.upsample && a.Cout <= 4 && (a.tile_cfg == 0 || (a.tile_cfg >= CFG_SMALL_32ROWS && a.tile_cfg <= CFG_SMALL_ONE_GROUP))) {
        // 32-row tiles from one workgroup per CU up, 8 rows otherwise; four channel groups per workgroup from 32 input channels
        // up (a rule of the layer's shape: the groups' sums are added in their own order)
        const int nchunks = cdiv(a.c0 + a.c1, CS_CIC);
        const bool rows32 = a.tile_cfg == CFG_SMALL_32ROWS || (a.tile_cfg != CFG_SMALL_8ROWS && (int64_t)a.B * cdiv(a.Win, CS_TW) * cdiv(a.Hin, 32) >= 256);
        const bool groups4 = a.tile_cfg != CFG_SMALL_ONE_GROUP && nchunks % 4 == 0 && nchunks >= 16;
        pl.kernel = CK_SMALLCOUT; pl.cfg = a.tile_cfg ? a.tile_cfg : (rows32 ? CFG_SMALL_32ROWS : CFG_SMALL_8ROWS);
        pl.form = (rows32 ? 1 : 0) | (groups4 ? 2 : 0);
        return SISIC_OK;
    }
    // Winograd F(2x2,3x3): 2.25x fewer MFMA FLOPs
    if ((pl.cfg = winograd_cfg(a, pl.Hout, pl.Wout)) != 0) { plan_winograd(a, pl); return SISIC_OK; }
    return plan_direct(a, pl);
}

}  // namespace

const WinoCfg* wino_cfg_row(int cfg) { for (const WinoCfg& w : WINO) if (w.cfg == cfg) return &w; return nullptr; }

int conv_plan(const sisic_conv_args& a, ConvPlan* out) {
    ConvPlan& pl = *out = ConvPlan{};
    SISIC_REQUIRE(a.in0 && a.w_packed && a.out, "conv2d: null tensor");
    SISIC_REQUIRE(a.B > 0 && a.Hin > 0 && a.Win > 0 && a.c0 > 0 && a.c1 >= 0 && a.Cout > 0, "conv2d: bad shape");
    SISIC_REQUIRE((a.c1 == 0) == (a.in1 == nullptr), "conv2d: in1/c1 mismatch");
    SISIC_REQUIRE(a.ksize == 1 || a.ksize == 3 || a.ksize == 7, "conv2d: ksize %d unsupported", a.ksize);
    SISIC_REQUIRE(a.stride == 1 || a.stride == 2, "conv2d: stride %d unsupported", a.stride);
    SISIC_REQUIRE(a.ksize != 7 || a.stride == 2, "conv2d: 7x7 is built for stride 2 only (the ResNet stem)");
    SISIC_REQUIRE(!(a.upsample && a.stride != 1), "conv2d: upsample with stride");
    SISIC_REQUIRE((a.gn_scale == nullptr) == (a.gn_shift == nullptr), "conv2d: gn_scale/gn_shift mismatch");

    const int ups = a.upsample ? 1 : 0, pad = a.ksize / 2, Cin = a.c0 + a.c1;
    pl.Hout = ((a.Hin << ups) + 2 * pad - a.ksize) / a.stride + 1;
    pl.Wout = ((a.Win << ups) + 2 * pad - a.ksize) / a.stride + 1;
    const double kk = double(a.ksize) * a.ksize, out_elems = double(a.B) * a.Cout * pl.Hout * pl.Wout;
    pl.bytes = 4.0 * (double(a.B) * Cin * a.Hin * a.Win + out_elems) + 4.0 * (Cin * a.Cout * kk + a.Cout) + (a.residual ? 4.0 * out_elems : 0.0);
    pl.flops = pl.issued_flops = 2.0 * out_elems * Cin * kk;
    pl.profile_kind = a.ksize == 1 ? PK_CONV1 : PK_CONV3; pl.profile_slot = -1; pl.ksplit = 1;

    const int rc = choose(a, pl);
    const bool stats_ok = a.stats_out == nullptr || (rc == SISIC_OK && pl.stats_slots > 0);
    SISIC_REQUIRE(stats_ok, "conv2d: stats_out given but sisic_conv_stats_slots() is 0 for these arguments");
    return rc;
}

int conv_stats_slots(const sisic_conv_args& a) { ConvPlan pl; return conv_plan(a, &pl) == SISIC_OK ? pl.stats_slots : 0; }
bool conv_finalizes(const sisic_conv_args& a) { ConvPlan pl; return conv_plan(a, &pl) == SISIC_OK && pl.finalizes; }

int conv_latency_cfg(const sisic_conv_args& a) {
    // the Winograd convolutions split their input channels over workgroups and the 1x1 convolutions take the 64-pixel tiles, so
    // that one image offers a few hundred workgroups per layer
    // (the 64-channel, two-workgroups-per-CU form for every Cout: at one image it is level with or ahead of the
    //  128-channel form on every layer, profiles/r02/ksplit_in_place_ab.txt rows 76 (128-channel) / 77 (64-channel))
    if (a.ksize == 3 && a.stride == 1 && !a.upsample && a.w_winograd && a.Cout > 4 && a.Hin >= 12 && a.Win >= 12) return CFG_WINO_LATENCY64;
    if (a.ksize == 1 && a.stride == 1) return 22;
    if (a.ksize == 3 && a.stride == 2) return 18;      // 8x8-pixel tiles, two K groups of waves: 189 -> 105 us for the three downsamplers of one 128x128 image
    return 0;
}

}  // namespace sisic
