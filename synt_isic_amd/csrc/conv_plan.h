// conv_plan.h -- which kernel runs a convolution and what that launch promises its caller, resolved ONCE.
//
// conv_plan() is a pure function of sisic_conv_args and the process-wide switches: no context, no stream, no launch, no
// allocation.  The queries (sisic_conv_stats_slots, sisic_conv_finalizes) and launch_conv2d() with its per-kernel launchers all
// read the same ConvPlan, so what a launch promises and what it does cannot drift apart.
#pragma once

#include "common.h"

namespace sisic {

// ---- tile configurations (sisic_conv_args.tile_cfg; the numbers are part of the interface: tests and tools/ use them)
// 1 .. 19, 21 .. 27, 31 .. 33, 41, 42: tilings of the direct MFMA kernel, SISIC_DIRECT_TILINGS below
// 20: the lean 1x1 kernel (conv_pointwise.hip)
// 28: 1x1 with fp32-equivalent products on the bf16 matrix pipe (conv_pointwise_bf3.hip), form chosen; 29 / 30: its 32- / 64-pixel
//     items forced (tests of the two forms' bit-equality); 34 / 35: its staged / K-split form forced; 37: its staged K-split form
//     forced (the bits of 35)
// 36: 3x3 stride 2 on the bf16 pipe (conv_s2_bf3.hip)
// 50 .. 52: the vector-ALU kernel for Cout <= 4 (conv_small.hip) with 32-row tiles / 8-row tiles / one channel group forced
// Winograd F(2x2,3x3), conv_winograd.hip (properties: the table in conv_plan.cpp):
// 60 .. 63: first geometry, 1 image x 8x8 tiles (16x16 output pixels) or 4 images x 4x4 tiles (8x8 outputs each), 8 or 16 waves
//           (16: one transform position per wave, 4 waves per SIMD); 64 .. 67 = 60 .. 63 with the MFMA-first / stage-first phase
//           stagger between SIMD partner waves
// 68 / 69:  second geometry, 32 tiles per workgroup, filters straight from global memory into registers: 128 output channels x 16
//           waves (Cout > 64) / 64 channels x 8 waves, two workgroups per CU.  They run the THIRD form (conv_winograd_col.inc: same
//           tiles, same bits, a wave owns a column of the position grid) unless SISIC_WINO_COL=0; 70 / 71 force the third form,
//           72 / 73 the second: A/B and tests
// 74:       fp32-equivalent products on the bf16 pipe (conv_winograd_bf3.inc): 64 channels x 16 x 16 pixels per workgroup
// 78 / 79:  68 / 69 in latency mode: input channels K-split so that one image fills the chip (wino_latency_ksplit)
// 90 .. 92: the 8x8 level, where 64 tiles x 64 channels per workgroup would leave 3/4 of the CUs without work: the input channels
//           split over four workgroups per tile + a reduction launch -- on tiling 67 / on the second geometry with two images per
//           workgroup (bit-identical to 90) / on the bf16x3 kernel with four images per workgroup
enum ConvCfg : int {
    CFG_AUTO = 0, CFG_POINTWISE = 20, CFG_PWB = 28, CFG_PWB_32PX = 29, CFG_PWB_64PX = 30, CFG_PWB_STAGED = 34, CFG_PWB_KSPLIT = 35,
    CFG_S2_BF3 = 36, CFG_PWB_STAGED_KSPLIT = 37, CFG_SMALL_32ROWS = 50, CFG_SMALL_8ROWS = 51, CFG_SMALL_ONE_GROUP = 52,
    CFG_WINO_1IMG_8W = 60, CFG_WINO_4IMG_8W = 61, CFG_WINO_1IMG_16W = 62, CFG_WINO_4IMG_16W = 63,
    CFG_WINO_1IMG_8W_STAG = 64, CFG_WINO_4IMG_8W_STAG = 65, CFG_WINO_1IMG_16W_STAG = 66, CFG_WINO_4IMG_16W_STAG = 67,
    CFG_WINO_WIDE128 = 68, CFG_WINO_WIDE64 = 69, CFG_WINO_COL128 = 70, CFG_WINO_COL64 = 71, CFG_WINO_SECOND128 = 72, CFG_WINO_SECOND64 = 73,
    CFG_WINO_BF3 = 74, CFG_WINO_LATENCY128 = 78, CFG_WINO_LATENCY64 = 79, CFG_KSPLIT8_FIRST = 90, CFG_KSPLIT8_PAIR = 91, CFG_KSPLIT8_BF3 = 92,
};

// Tilings of the direct MFMA kernel (conv_mfma.hip): X(id, KS, STRIDE, MT, NT, WM, WN, TW, CIC, OCC, KSP).  A workgroup owns
// WM*MT*32 = 64 output channels x WN*NT*32 pixels in rows of TW, walks the input channels in chunks of CIC, and leaves one
// GroupNorm partial slot per pixel tile and pixel-wave (WN).  The launch and the slot count both come from this list.
//   16 / 17: cfg 4's 64x64 tile with 8 waves = 2 K groups x (2x2), 16- / 8-channel chunks
//   18 / 19: cfg 13's tile with two K-split wave groups (18 is latency mode's: 8x8 pixels, 8 waves = 2 K groups x (2x2))
//   21 .. 27: 1x1, the image is a flat row of H*W pixels.  (Four-wave tiles at three / six workgroups per CU were measured too --
//            profiles/r02/conv1x1_tilings_and_contraction.txt: within 2 % of 24 / slower -- and removed: occupancy is not what
//            limits these launches)
//   41 / 42: 7x7 stride 2 (the ResNet stem).  41: 2-channel chunks -- 4 spill 256 B/lane (13 weight float4 + 15 halo elements per thread)
#define SISIC_DIRECT_TILINGS(X) \
    X(1, 3, 1, 2, 2, 1, 4, 64, 8, 2, 1)  X(2, 3, 1, 2, 2, 1, 4, 32, 8, 2, 1)  X(3, 3, 1, 2, 2, 1, 4, 16, 8, 2, 1) \
    X(4, 3, 1, 1, 1, 2, 2, 8, 8, 2, 1)  X(5, 3, 1, 2, 1, 1, 4, 16, 8, 2, 1)  X(6, 3, 1, 2, 1, 1, 4, 64, 8, 2, 1) \
    X(7, 3, 1, 2, 1, 1, 4, 32, 8, 2, 1)  X(8, 3, 1, 1, 2, 2, 4, 32, 8, 4, 1)  X(9, 3, 1, 1, 2, 2, 4, 16, 8, 4, 1) \
    X(10, 3, 1, 1, 2, 2, 4, 32, 8, 2, 1)  X(14, 3, 1, 1, 1, 2, 4, 16, 8, 4, 1)  X(15, 3, 1, 1, 1, 2, 4, 8, 8, 4, 1) \
    X(16, 3, 1, 1, 1, 2, 2, 8, 16, 2, 2)  X(17, 3, 1, 1, 1, 2, 2, 8, 8, 2, 2)  X(11, 3, 2, 2, 1, 1, 4, 32, 8, 2, 1) \
    X(12, 3, 2, 2, 1, 1, 4, 16, 8, 2, 1)  X(13, 3, 2, 1, 1, 2, 2, 8, 8, 2, 1)  X(18, 3, 2, 1, 1, 2, 2, 8, 16, 2, 2) \
    X(19, 3, 2, 1, 1, 2, 2, 8, 8, 2, 2)  X(21, 1, 1, 2, 2, 1, 4, 256, 16, 2, 1)  X(22, 1, 1, 1, 1, 2, 2, 64, 16, 2, 1) \
    X(23, 1, 1, 2, 1, 1, 4, 128, 16, 2, 1)  X(24, 1, 1, 1, 2, 2, 4, 256, 32, 4, 1)  X(25, 1, 1, 1, 1, 2, 4, 128, 32, 4, 1) \
    X(26, 1, 1, 1, 2, 2, 4, 256, 16, 4, 1)  X(27, 1, 1, 1, 1, 2, 4, 128, 16, 4, 1)  X(31, 1, 2, 2, 1, 1, 4, 32, 16, 2, 1) \
    X(32, 1, 2, 2, 1, 1, 4, 16, 16, 2, 1)  X(33, 1, 2, 1, 1, 2, 2, 8, 16, 2, 1)  X(41, 7, 2, 2, 1, 1, 4, 32, 2, 2, 1) \
    X(42, 7, 2, 2, 1, 1, 4, 32, 4, 2, 1)

// the launcher's kernel: conv_small.hip; conv_mfma.hip; conv_pointwise.hip; conv_pointwise_bf3.hip (ConvPlan::form = PwbForm);
// conv_s2_bf3.hip; conv_winograd.hip's first geometry (and its nine-position form for nearest-2x inputs), conv_winograd_wide.inc,
// conv_winograd_col.inc, conv_winograd_bf3.inc -- each of the four also K-split (ConvPlan::ksplit > 1) with a reduction launch behind it
enum ConvKernel { CK_SMALLCOUT, CK_DIRECT, CK_POINTWISE, CK_POINTWISE_BF3, CK_S2_BF3, CK_WINO_FIRST, CK_WINO_SECOND, CK_WINO_THIRD, CK_WINO_BF3 };
enum PwbForm { PWB_FORM_KSPLIT, PWB_FORM_STAGED, PWB_FORM_64PX, PWB_FORM_32PX, PWB_FORM_STAGED_KSPLIT };
// the 8x8 level's reduction; REDUCE_64PX: planes of exactly 64 pixels and 16-byte aligned residual / out / stats_out
enum ReduceForm { REDUCE_ANY, REDUCE_64PX };

// the Winograd configurations' properties
enum WinoGeometry { WG_FIRST, WG_SECOND, WG_BF3 };
struct WinoCfg {
    int cfg;
    WinoGeometry geom;
    int imgs, waves;     // images per workgroup tile; waves (second geometry: 16 waves = 128 output channels per workgroup, 8 = 64)
    bool stagger;
    int col;             // second geometry: 1 = third form forced, 0 = second form forced, -1 = third unless SISIC_WINO_COL=0
    int ksplit;          // 0: none, 4: the 8x8 level's split, -1: latency mode's (wino_latency_ksplit)
    int tile_h, tile_w;  // output pixels of a workgroup tile = of a GroupNorm partial slot
    int profile_slot;    // the kernel family's own ProfileKind, or -1
};
const WinoCfg* wino_cfg_row(int cfg);      // nullptr: not a Winograd configuration

// constants the plan shares with conv_small.hip: pixels of a tile row, input channels per chunk
constexpr int CS_TW = 32, CS_CIC = 2;
// ... and with conv_pointwise_bf3.hip
constexpr int PWB_WAVES = 4;             // waves (= independent work items) per workgroup
constexpr int PWBS_MAX_WAVES = 12;       // staged form: channel items (= waves) of a workgroup
// staged form: LDS holds the image's 64 pixels of every input channel as split operands (6 bytes per value) and the GroupNorm table
inline size_t pwbs_lds_bytes(int Cin) { return (size_t)(Cin / 8) * 2 * 64 * 24 + 8 * (size_t)Cin; }
// staged K-split form: waves = (Cout / 64 channel items) x (PWB_WAVES K quarters); LDS holds at most PWBSK_CAP chunks of every
// quarter as split operands (longer contractions run in passes) and later one 32-channel block of every wave's partial accumulators
constexpr int PWBSK_MAX_WAVES = 16, PWBSK_CAP = 8;
constexpr size_t PWBSK_MAX_LDS = 128 * 1024;
inline size_t pwbsk_lds_bytes(int Cin, int Cout) {
    const int nl = Cin / 8 / PWB_WAVES;
    const size_t operands = (size_t)PWB_WAVES * (nl < PWBSK_CAP ? nl : PWBSK_CAP) * 2 * 64 * 24, partials = (size_t)PWB_WAVES * (Cout / 64) * 32 * 64 * 4;
    return operands > partials ? operands : partials;
}

struct ConvPlan {
    ConvKernel kernel;
    int cfg;               // the resolved tile configuration: never 0
    int form;              // the kernel's sub-form where it has one: PwbForm, ReduceForm, conv_small.hip's tile bits
    int Hout, Wout, stats_slots;   // stats_slots 0: this launch writes no GroupNorm partials
    bool finalizes, carries_rider;   // with fin_gamma set, this launch writes fin_scale / fin_shift; it can run rider workgroups (gn_finalize.h)
    int ksplit;            // ways the input channels are split over workgroups (a reduction launch follows); 1 when not
    int profile_kind, profile_slot;         // what ProfileScope is told
    double bytes, flops, issued_flops;
    // A forced configuration on arguments its kernel does not take: the LAUNCH's error.  The queries keep answering for the
    // tiling itself, as they always have; launch_conv2d() reports this text and launches nothing.
    char refusal[200];
};

// SISIC_OK, or SISIC_EINVAL with set_error(): arguments no kernel takes (the queries then answer 0)
int conv_plan(const sisic_conv_args& a, ConvPlan* out);

// latency mode's tile configuration for a layer (sisic_unet_set_latency_mode; the forward and the data gradient), 0 = the
// automatic choice.  From the layer shape only: inside this mode an image's bits are again independent of the batch.
int conv_latency_cfg(const sisic_conv_args& a);

}  // namespace sisic
