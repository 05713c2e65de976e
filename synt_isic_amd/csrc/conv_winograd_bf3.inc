// conv_winograd_bf3.inc -- Winograd F(2x2,3x3) with fp32-EQUIVALENT products on the bf16 matrix pipe (included by
// conv_winograd.hip; tile_cfg 74).
//
// The f32 MFMA is the SIMD's own FMA array: 157 TFLOP/s on paper, 137 at the clock it sustains, and every vector instruction
// beside it costs matrix time (DESIGN.md section 4).  The bf16 MFMA is a separate, 16x faster pipe.  An fp32 number splits
// EXACTLY into three bf16 terms (8 + 8 + 8 significant bits: hi = the top 16 bits, mid = the top 16 bits of x - hi, lo = the
// rest), and a product a * b is the sum of nine term products of which the three smallest (mid*lo, lo*mid, lo*lo) are below
// 2^-24 of it.  The other six -- each exact in fp32 -- are summed by v_mfma_f32_32x32x16_bf16 into its fp32 accumulator.  K = 16
// is two groups of eight (lanes 0-31 / lanes 32-63 of both operands); here a group is FOUR input channels x TWO terms:
//     MFMA 1   A = (U_hi, U_mid)   B = (V_hi , V_mid)      U_hi V_hi  + U_mid V_mid
//     MFMA 2   A = (U_hi, U_mid)   B = (V_mid, V_hi )      U_hi V_mid + U_mid V_hi
//     MFMA 3   A = (U_hi, U_lo )   B = (V_lo , V_hi )      U_hi V_lo  + U_lo  V_hi        (A put together in registers)
// Three 32-cycle instructions replace four 64-cycle ones: 2.7x the matrix throughput, and the bf16 MFMA leaves about half of a
// concurrent vector stream hidden (tools/bf16_overlap_probe.hip) where the f32 MFMA hides none.  Accuracy: emulated against
// float64 (tools/bf16x3_accuracy.py) the six-product sum is MORE accurate than the fp32 FMA chain it replaces (16 products are
// rounded into the accumulator once, not one by one); on the GPU it passes the same per-kernel bound (1e-5) as the f32 forms
// with the same measured error (1.5 - 2.1e-7).  Results are NOT bit-equal to the f32 forms (another summation order): the choice is
// per layer shape, never per batch, so an image's bits still do not depend on the batch it is computed in.
//
// Geometry: workgroup = 64 output channels x 64 tiles (16 x 16 output pixels), 16 waves, one per CU; a wave owns ONE of the 16
// Winograd positions for all 64 x 64 (four 32 x 32 accumulators).
//   stage      8-channel chunk of the 18 x 18 halo -> LDS (fp32, GroupNorm + SiLU applied, zero padding by never-written slots);
//              channels interleaved in pairs, even and odd columns in separate planes of a row: the stride-2 reads below are
//              conflict-free ds_read_b64 of a channel pair
//   transform  lane = (tile t, channel group g): the wave's ONE element of V = B^T d B is two row and two column taps, four
//              reads and three packed FMAs with +-1 scalars per channel pair, for the lane's four channels and two tiles (t, t + 32); split into
//              the three terms IN REGISTERS: with the K grouping above the B operands are the lane's own packed terms -- V never
//              goes through LDS, nothing crosses lanes
//   multiply   2 tile blocks x 2 channel blocks x 3 MFMAs per chunk; A straight from global memory (a packing of the split U:
//              per lane and channel block 16 bytes of (hi, mid) and 8 of lo -- 48 KB per chunk and workgroup; the vector memory
//              path, 64 bytes a clock and CU, is the resource this kernel has least of)
//   output     16 M planes through LDS in four 16-channel rounds, Y = A^T M A, bias / embedding / residual, GroupNorm partials
//   items      a workgroup is persistent: with more work items than CUs it takes items L, L + gridDim.x, ... and requests the next
//              item's first two halo chunks and GroupNorm operands before the output rounds of the current one (see the kernel)
// LDS: [halo buffers 22.5 KB][GroupNorm table 16 KB | filter operands 96 KB]  in the channel loop,
//      [halo buffers 22.5 KB][output planes 2 x 64 KB][plan store offsets 8 KB] in the rounds (the halo buffers' zero padding survives them)
template <int PRO>
struct Bf3Geom {
    static constexpr int CO_T = 64, NW = 16, THREADS = 1024;
    static constexpr int TY = 8, TX = 8, TILES = 64;
    static constexpr int HH = 18, HWD = 18, HROW = 20, HPL = 10;   // a row: [even columns 0..8, spare][odd columns 0..8, spare]
    static constexpr int HPI = HH * HWD;                       // 324 staged elements per channel
    static constexpr int HB1 = 2 * HH * HROW;                  // 720 floats: one channel PAIR in one buffer
    static constexpr int CPS = 2 * HB1;                        // [channel pair][buffer][row][plane][10][2 channels]
    static constexpr int H_FLOATS = (W_CIC / 2) * CPS;         // 5760 floats = 22.5 KB
    static constexpr int TPC = THREADS / W_CIC;                // 128 threads stage one channel
    static constexpr int EPT = (HPI + TPC - 1) / TPC;          // 3
    static constexpr int RCO = 16, ROUNDS = CO_T / RCO;
    static constexpr int M_ROUND = 16 * RCO * TILES;           // one epilogue round: [16 positions][16 channels][64 tiles]
    static constexpr int EPI_FLOATS = 2 * M_ROUND;
    static constexpr int GN_MAX_CH = 2048;                     // the image's GroupNorm (scale, shift) table behind the halo
    static constexpr int UA_WAVE = 768;                        // dwords: a wave's A operands of one chunk (pack_device.h)
    static constexpr int UA_BUF = NW * UA_WAVE;                // 48 KB a buffer, two of them
    static constexpr int UA_OFF = H_FLOATS + 2 * GN_MAX_CH;
    static constexpr int LOOP_FLOATS = UA_OFF + 2 * UA_BUF;    // 22.5 + 16 + 96 = 134.5 KB
    // the output rounds' planes lie BEHIND the halo buffers (23 + 128 KB of the CU's 160): the zeroed padding slots of a tile
    // position survive the rounds, and a workgroup whose next item is the same position of another image keeps its whole plan
    static constexpr int EPI_OFF = H_FLOATS;
    // ... and behind the planes 8 bytes per thread: the plan's three LDS store offsets, which the rounds have no registers for
    static constexpr int HOFF_OFF = (LOOP_FLOATS > EPI_OFF + EPI_FLOATS ? LOOP_FLOATS : EPI_OFF + EPI_FLOATS);
    // ... and 8 bytes per channel of the workgroup: the (sum, M2) partials of a tile that is a whole image, for the GroupNorm
    // finalisation the workgroup then does itself (sisic_conv_args.fin_*)
    static constexpr int FIN_OFF = HOFF_OFF + 2 * THREADS;
    static constexpr size_t LDS_BYTES = sizeof(float) * (size_t)(FIN_OFF + 2 * CO_T);
    static_assert(LDS_BYTES <= 160 * 1024, "bf16x3 Winograd: LDS");
};

#ifndef BF3_PRIO
#define BF3_PRIO 1       // 0: no s_setprio in the channel loop (A/B builds)
#endif
#ifndef BF3_ONE_UA
#define BF3_ONE_UA 1     // 0: round 3's two filter buffers, the fetch in the middle of the chunk before (A/B builds, tools/kernel_variants.sh)
#endif
#ifndef BF3Q_VAR
#define BF3Q_VAR 0
#endif
#ifndef BF3_VAR
#define BF3_VAR 0        // diagnostic builds only (tools/kernel_variants.sh): bit 0 no A loads, 1 no transform, 2 no staging, 3 no MFMA, 4 no output, 5 no halo loads, 6 no SiLU, 7 no halo stores,
                         // 9 ONE V per chunk feeds both tile blocks' MFMAs (what a 128-channel x 32-tile workgroup would do per V), 10 the filter fetch issued twice (its doubled operand bytes),
                         // 11 no U_lo (two of the three filter transfers: what 16-bit filters would fetch), 12 no third MFMA and no lo term of V (what two-term operands would cost)
#endif
// diagnostic build (-DWINO_TIMING=1): EVERY wave stamps s_memtime at its phase boundaries into p.stats
// ([workgroup][16 waves][BF3_STAMPS] uint64, tools/bf3_timeline.py) instead of the GroupNorm partials
#define BF3_STAMPS 16
#if WINO_TIMING
#define BF3_STAMP(slot)                                                                                    \
    do {                                                                                                   \
        unsigned long long t_;                                                                             \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                         \
        if (lane == 0) reinterpret_cast<unsigned long long*>(p.stats)[((size_t)BF3_STAMP_ITEM * 16 + wave_u) * BF3_STAMPS + (slot)] = t_; \
    } while (0)
#else
#define BF3_STAMP(slot) do { } while (0)
#endif
typedef short bf3_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned bf3_u4 __attribute__((ext_vector_type(4)));
typedef float bf3_f2 __attribute__((ext_vector_type(2)));
typedef unsigned bf3_u2 __attribute__((ext_vector_type(2)));

// ---- the item table.  What a workgroup derives from a work item's index L -- the remapped (channel tile, tile position,
// image), the images' element offsets in every tensor, the tile's flags -- is a function of the launch GEOMETRY alone (B, plane,
// channels, grid), not of data or pointers: the same in all 16 waves, in every launch of the layer and in every step of a run.
// It is computed once per geometry by bf3_item_table_kernel into one 64-byte record per item (offsets only, never pointers:
// one table serves every launch of the geometry), and a wave fetches a record with ONE scalar load where it needs it -- the
// 64 bytes stay in the scalar cache, so nothing of them is held (spilled) across the channel loop.
struct Bf3Item {
    unsigned b0, co0, oy0, ox0;
    unsigned slot;              // gy * groups_x + gx
    unsigned in0_off, in1_off;  // elements: the item's image in in0 / in1
    unsigned out_off;           // ... in out / residual
    unsigned gn_off;            // b0 * Cin: gn_scale / gn_shift
    unsigned cb_off;            // b0 * chan_bias_stride
    unsigned stats_off;         // float4s: (b0 * Cout + co0) * slots + slot
    unsigned fin_off;           // b0 * Cout + co0: fin_scale / fin_shift
    unsigned flags;
    unsigned tile_cnt, inv_cnt; // float bits: pixels of the tile inside the plane, and 1 / that
    unsigned tile_off;          // bytes: pixel (oy0, ox0) in a plane of the output
};
static_assert(sizeof(Bf3Item) == 64, "one s_load_dwordx16 per record");
enum : unsigned {
    BF3_IT_WHOLE = 1,      // the 16 x 16 tile lies wholly inside the plane
    BF3_IT_EVEN_W = 2,     // even plane width
    BF3_IT_NEW_TILE = 4,   // another tile position than the same workgroup's item before (or its first item)
    BF3_IT_LAST = 8,       // the workgroup's last item
};
typedef unsigned bf3_u16 __attribute__((ext_vector_type(16)));
// (constant address space: a scalar load wherever it stands -- behind the stores of the item before the compiler makes loads
//  through a global pointer vector loads; the index is made opaque so that a second fetch of a record is a second load and not
//  sixteen registers kept from the first)
__device__ __forceinline__ bf3_u16 bf3_item_fetch(const unsigned* tab, int L) {
    asm volatile("" : "+s"(L));
    return *(reinterpret_cast<const __attribute__((address_space(4))) bf3_u16*>((size_t)tab) + L);
}
#define BF3_IT(rec, field) ((rec)[offsetof(Bf3Item, field) / 4])

// XCD-aware bijective remap of item l (conv_mfma.hip) and its (channel tile, tile column, tile row, image)
__device__ __forceinline__ void bf3_decode(const WinoParams& p, int l, int& co_t, int& gx, int& gy, int& b0) {
    const int nwg = p.nwg;
    const int xcd = l & 7, slot = l >> 3, q = nwg >> 3, r = nwg & 7;
    const int work = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    co_t = work % p.n_co_tiles;
    int grp = work / p.n_co_tiles;
    gx = grp % p.groups_x;
    grp /= p.groups_x;
    gy = grp % p.groups_y;
    b0 = grp / p.groups_y;
}

__global__ void bf3_item_table_kernel(const WinoParams p, unsigned* __restrict__ tab) {
    const int L = blockIdx.x * blockDim.x + threadIdx.x;
    if (L >= p.nwg) return;
    int co_t, gx, gy, b0;
    bf3_decode(p, L, co_t, gx, gy, b0);
    const int oy0 = gy * 16, ox0 = gx * 16, co0 = co_t * 64;
    const unsigned HWin = (unsigned)(p.Hin * p.Win), HWo = (unsigned)(p.Hc * p.Wc), slots = (unsigned)(p.groups_x * p.groups_y);
    Bf3Item it;
    it.b0 = (unsigned)b0; it.co0 = (unsigned)co0; it.oy0 = (unsigned)oy0; it.ox0 = (unsigned)ox0;
    it.slot = (unsigned)(gy * p.groups_x + gx);
    it.in0_off = (unsigned)b0 * (unsigned)p.c0 * HWin;          // (launch_bf3: every product below 2^32)
    it.in1_off = (unsigned)b0 * (unsigned)p.c1 * HWin;
    it.out_off = (unsigned)b0 * (unsigned)p.Cout * HWo;
    it.gn_off = (unsigned)b0 * (unsigned)(p.c0 + p.c1);
    it.cb_off = (unsigned)b0 * (unsigned)p.chan_bias_stride;
    it.stats_off = ((unsigned)b0 * (unsigned)p.Cout + (unsigned)co0) * slots + it.slot;
    it.fin_off = (unsigned)b0 * (unsigned)p.Cout + (unsigned)co0;
    bool new_tile = true;
    if (L >= p.grid) {
        int co_p, gx_p, gy_p, b_p;
        bf3_decode(p, L - p.grid, co_p, gx_p, gy_p, b_p);
        new_tile = gx != gx_p || gy != gy_p;
    }
    it.flags = ((oy0 + 16 <= p.Hc && ox0 + 16 <= p.Wc) ? BF3_IT_WHOLE : 0u) | ((p.Wc & 1) == 0 ? BF3_IT_EVEN_W : 0u) |
               (new_tile ? BF3_IT_NEW_TILE : 0u) | (L + p.grid >= p.nwg ? BF3_IT_LAST : 0u);
    const float tile_cnt = (float)(min(16, p.Hc - oy0) * min(16, p.Wc - ox0));
    it.tile_cnt = __float_as_uint(tile_cnt);
    it.inv_cnt = __float_as_uint(1.0f / tile_cnt);
    it.tile_off = 4u * (unsigned)(oy0 * p.Wc + ox0);
    reinterpret_cast<Bf3Item*>(tab)[L] = it;
}

// TAB: the per-item values come from the item table (p.items); without it (no table for this geometry, SISIC_BF3_ITEM_TABLE=0)
// the instance derives them from the item's index itself -- the same values, the same bits
template <int PRO, bool UPS = false, bool TAB = false>      // UPS: nearest-2x input (an instance of its own: the other one keeps its branch-free loop)
__global__ void __launch_bounds__(1024, 4) conv_winograd_bf3_kernel(const WinoParams p) {
    using G = Bf3Geom<PRO>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const H_lds = smem;                                                  // [4][2][18][2][10][2] fp32
    float* const GN_lds = smem + G::H_FLOATS;                                   // [input channel][scale, shift]
    float* const M_base = smem + G::EPI_OFF;                                    // epilogue: [2][16][16][64], behind the halo buffers

    // A workgroup is PERSISTENT: it takes the work items L = blockIdx.x, blockIdx.x + gridDim.x, ... (launch_bf3: one workgroup
    // per CU when there are more items than CUs) and requests the first two chunks' halo of its next item before the output rounds
    // of the current one -- a fresh workgroup's first loads are first-touch memory latency with nothing to hide behind (3.2 us of a
    // 64 -> 64 workgroup's 21.5), here they fly under the rounds.
    int L = blockIdx.x;
    int co_t, gx, gy, b0, oy0, ox0, co0;
    auto decode = [&](const int l) {   // XCD-aware bijective remap (conv_mfma.hip); gridDim.x is a multiple of 8 whenever a workgroup has a second item
        const int nwg = p.nwg;
        const int xcd = l & 7, slot = l >> 3, q = nwg >> 3, r = nwg & 7;
        const int work = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
        co_t = work % p.n_co_tiles;
        int grp = work / p.n_co_tiles;
        gx = grp % p.groups_x;
        grp /= p.groups_x;
        gy = grp % p.groups_y;
        b0 = grp / p.groups_y;
        oy0 = gy * 2 * G::TY; ox0 = gx * 2 * G::TX;
        co0 = co_t * G::CO_T;
    };
    if constexpr (!TAB) decode(L);
    const int n = p.nchunks;
    // With a whole number of images between a workgroup's successive items (the remap is then regular: nwg a multiple of 8, and
    // gridDim.x / 8 consecutive work indices apart) the next item is the same channel tile and position `img_step` images on: no
    // decode (a hundred scalar instructions of division), no new plan.
    int img_step = 0;
    if constexpr (!TAB) {
        const int per_img = p.n_co_tiles * p.groups_x * p.groups_y;
        img_step = ((p.nwg & 7) == 0 && (int)(gridDim.x >> 3) % per_img == 0) ? (int)(gridDim.x >> 3) / per_img : 0;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int HWin = p.Hin * p.Win, Cin = p.c0 + p.c1;
    // The lane index again, from the hardware (two instructions, no memory), for the per-item code: the channel loop takes all
    // 128 registers, and every lane-derived value kept across it for the item's prologue or output rounds is a scratch reload
    // there -- a vector-memory operation whose s_waitcnt vmcnt(0) also waits for the halo and filter loads in flight.
    auto fresh_lane = [] {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    float* const UA_lds = smem + G::UA_OFF + wave_u * G::UA_WAVE;               // this wave's A operands: [2 buffers][...][768 dwords]
    const unsigned ua_lds_addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)UA_lds);

    __amdgpu_buffer_rsrc_t rs0, rs1;                  // the item's image in both sources
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.uw), 0, -1, 0x00020000);

    // ---- halo staging plan: 128 threads per channel of the chunk (wave-uniform channel); positions outside the image are
    // zeroed once, their lanes store into the spare slot of row 0 afterwards (third form)
    const int sci = wave_u >> 1;
    const int sl = tid & 127;
    unsigned goff[G::EPT];
    int hoff[G::EPT];
    // FULL = false: the item's sources and load offsets only, for the two requests made ahead of the output rounds of the item
    // before (nothing of the plan is kept across the rounds: they need the registers); FULL = true, at the top of the item: load
    // and store offsets, and the zeroing of its padding slots (the rounds used the same LDS)
    auto plan = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        // (recomputed per item from an opaque copy of the thread index: hoisted out of the item loop, these few values would be
        //  live across the channel loop, whose registers are all taken)
        const int sl_i = (wave_u & 1) * 64 + fresh_lane();
#pragma unroll
        for (int i = 0; i < G::EPT; ++i) {
            const int e = sl_i + i * G::TPC;
            const bool in = e < G::HPI;
            const int ec = in ? e : 0;
            const int yy = ec / G::HWD, xx = ec % G::HWD;
            const int y = oy0 - 1 + yy, x = ox0 - 1 + xx;
            const bool v = in && y >= 0 && y < p.Hc && x >= 0 && x < p.Wc;
            const int slot = yy * G::HROW + (xx & 1) * G::HPL + (xx >> 1);
            goff[i] = v ? 4u * (unsigned)((y >> (UPS ? 1 : 0)) * p.Win + (x >> (UPS ? 1 : 0))) : 0u;      // (nearest-2x input: the low-resolution pixel)
            if constexpr (FULL) {
                hoff[i] = 2 * (v ? slot : (G::HPL - 1) + G::HPL * (sl_i & 1));      // (< 2^16)
                if (in && !v) {
                    float* z = H_lds + (sci >> 1) * G::CPS + 2 * slot + (sci & 1);
                    z[0] = 0.0f;
                    z[G::HB1] = 0.0f;
                }
            }
        }
        if constexpr (FULL) {
            static_assert(G::EPT == 3, "three store offsets in two dwords");
            *reinterpret_cast<bf3_u2*>(smem + G::HOFF_OFF + 2 * ((wave_u >> 1) * G::TPC + sl_i)) =
                bf3_u2{(unsigned)hoff[0] | ((unsigned)hoff[1] << 16), (unsigned)hoff[2]};
        }
    };
    auto set_sources = [&] {
        rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in0 + (size_t)b0 * p.c0 * HWin), 0, -1, 0x00020000);
        rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in1 ? p.in1 + (size_t)b0 * p.c1 * HWin : p.in0), 0, -1, 0x00020000);
    };
    auto set_sources_item = [&](const bf3_u16& it) {      // the same two, the image's offsets from its record
        rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in0 + (size_t)BF3_IT(it, in0_off)), 0, -1, 0x00020000);
        rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in1 ? p.in1 + (size_t)BF3_IT(it, in1_off) : p.in0), 0, -1, 0x00020000);
    };
    int gn_base = 0;                                      // the item's image in gn_scale / gn_shift
    if constexpr (TAB) {
        const bf3_u16 it = bf3_item_fetch(p.items, L);
        b0 = (int)BF3_IT(it, b0); co0 = (int)BF3_IT(it, co0); co_t = co0 >> 6; oy0 = (int)BF3_IT(it, oy0); ox0 = (int)BF3_IT(it, ox0);
        gx = gy = 0;
        set_sources_item(it);
        gn_base = (int)BF3_IT(it, gn_off);
    } else {
        set_sources();
    }
    plan(std::false_type{});

    // ---- the wave's position (i, j) of V = B^T d B: rows (a, b) and columns (c, e) of the 4 x 4 patch with signs,
    //      V_ij = (d[a][c] + sr d[b][c]) + sc (d[a][e] + sr d[b][e])
    const int pos = wave_u, pi = pos >> 2, pj = pos & 3;
    // A nearest-2x input repeats every pixel twice in each direction and the tiles start on even pixels, so the two middle rows
    // (columns) of every 4 x 4 patch are equal: row 2 and column 2 of V = B^T d B (d2 - d1) are EXACTLY zero for every tile and
    // channel.  The seven waves that own those positions add nothing: they skip their operands, transforms and MFMAs (their M
    // planes stay zero) and only take part in the staging, the barriers and the output rounds.  9 of 16 positions multiply --
    // the f32 upsample form's saving, kept.
    const bool live = !(UPS && (pi == 2 || pj == 2));
    const int ra = (pi == 0) ? 0 : (pi == 2 ? 2 : 1), rb = (pi == 2) ? 1 : (pi == 3 ? 3 : 2);
    const int ca = (pj == 0) ? 0 : (pj == 2 ? 2 : 1), cb = (pj == 2) ? 1 : (pj == 3 ? 3 : 2);
    const float sr = (pi == 1) ? 1.0f : -1.0f, sc = (pj == 1) ? 1.0f : -1.0f;
    // lane = (tile l31 of the block, channel group half): tile row 2 ty, column 2 tx of the staged patch
    // (the lane's four patch addresses and its filter-fetch offset are made again at the top of every item, from the hardware's
    //  lane index: kept across the output rounds, these five registers were spills there)
    const int col_a = (ca & 1) * G::HPL + (ca >> 1), col_b = (cb & 1) * G::HPL + (cb >> 1);
    const float *p_ac, *p_ae, *p_bc, *p_be;
    unsigned u_lane;
    auto lane_addresses = [&] {
        const int ln = fresh_lane();
        const int hf = ln >> 5, t31 = ln & 31, ty = t31 >> 3, tx = t31 & 7;
        const int xf_lane = (2 * hf) * G::CPS + 2 * ((2 * ty) * G::HROW + tx);
        p_ac = H_lds + xf_lane + 2 * (ra * G::HROW + col_a);
        p_ae = H_lds + xf_lane + 2 * (ra * G::HROW + col_b);
        p_bc = H_lds + xf_lane + 2 * (rb * G::HROW + col_a);
        p_be = H_lds + xf_lane + 2 * (rb * G::HROW + col_b);
        u_lane = 16u * (unsigned)ln;
    };
    lane_addresses();

    const int n_co32 = p.cout_pad >> 5;

    f32x16 acc[2][2];                // [32-channel block][tile block]

    struct HaloRegs {
        float v[G::EPT];
        bool cval = false;
    };
    HaloRegs hs[2];                  // chunk k travels in set k & 1: loaded two chunks before it is staged
    bf3_u4 ua[2];                    // A operands of the current chunk per channel block: (hi, mid) ...
    bf3_u2 ul[2];                    // ... and lo; the (hi, lo) operand is put together from them

    auto load_halo = [&](int chunk, HaloRegs& h) {
        const int c = chunk * W_CIC + sci;
        h.cval = c < Cin;
        const int hcc = min(c, Cin - 1);
        const bool first = hcc < p.c0;
        const __amdgpu_buffer_rsrc_t rs = first ? rs0 : rs1;
        const unsigned soff = 4u * (unsigned)((first ? hcc : hcc - p.c0) * HWin);
#pragma unroll
        for (int i = 0; i < G::EPT; ++i) h.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, goff[i], soff, 0));
    };
    // (scale, shift) of the staged channel from the LDS table: a scalar load here would be waited for at every barrier
    auto stage_halo = [&](int chunk, int hbuf, const HaloRegs& h) {
        float* dst = H_lds + (sci >> 1) * G::CPS + hbuf * G::HB1 + (sci & 1);
        float gsc = 1.0f, gsh = 0.0f;
        if constexpr (PRO != 0) {
            const bf3_f2 g = *reinterpret_cast<const bf3_f2*>(GN_lds + 2 * (chunk * W_CIC + sci));   // zeros past the last channel
            gsc = g.x; gsh = g.y;
        }
#pragma unroll
        for (int i = 0; i < G::EPT; ++i) {
            float v = h.v[i];
            if constexpr (PRO != 0) {
                v = v * gsc + gsh;
                if constexpr (PRO == 2 && (BF3_VAR & 64) == 0) v = wsilu(v);
            } else {
                v = h.cval ? v : 0.0f;
            }
            if constexpr ((BF3_VAR & 128) == 0) dst[hoff[i]] = v;
            else asm volatile("" :: "v"(v));
        }
    };
    // A operands: global -> LDS without registers (three wave-wide 16-byte-per-lane transfers, `buffer_load_dwordx4 ... lds`),
    // half a chunk ahead of their use.  Only this wave reads what it fetched, so its own vmcnt is all the synchronisation
    // there is -- and it is written here by hand: through the builtin the compiler puts s_waitcnt vmcnt(0) in front of every
    // barrier, i.e. a wait for the halo loads issued a moment before.  (Vector memory operations the compiler does not
    // know of can only make its own vmcnt waits stricter: the counter retires in order.)
    auto fetch_u = [&](int chunk, int ubuf) {
        const unsigned s0 = 3072u * (unsigned)(((chunk * 16 + pos) * (n_co32 >> 1)) + co_t);
        const unsigned dst = ua_lds_addr + 4u * (unsigned)(ubuf * G::UA_BUF);
#pragma unroll
        for (int k = 0; k < ((BF3_VAR & 2048) != 0 ? 2 : 3); ++k)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                         :: "s"(dst + 1024u * (unsigned)k), "v"(u_lane), "s"(rsu), "s"(s0 + 1024u * (unsigned)k) : "memory");
        if constexpr ((BF3_VAR & 1024) != 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                             :: "s"(dst + 4u * (unsigned)G::UA_BUF + 1024u * (unsigned)k), "v"(u_lane), "s"(rsu), "s"(s0 + 1024u * (unsigned)k) : "memory");
        }
    };
    // `newer`: vector memory operations this wave has issued since the fetch (the three halo loads, in the steady state)
    auto read_u = [&](int ubuf, auto newer_tag, const bool three_newer = false) {
        if constexpr (decltype(newer_tag)::value == 3 && !WINO_TIMING) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (three_newer && !WINO_TIMING) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const float* const src = UA_lds + ubuf * G::UA_BUF;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            ua[x] = *reinterpret_cast<const bf3_u4*>(src + 256 * x + 4 * lane);
            if constexpr ((BF3_VAR & 2048) != 0) ul[x] = bf3_u2{ua[x].z, ua[x].w};
            else ul[x] = *reinterpret_cast<const bf3_u2*>(src + 512 + 128 * x + 2 * lane);
        }
    };
    // the chunk's contribution for tile block nb: the wave's V element of the lane's four channels, its three terms, six MFMAs.
    // Plain v_fma / v_sub / v_and on purpose: beside the bf16 MFMA a plain vector instruction adds 0.5 - 0.8 cycles to the
    // SIMD's matrix stream, a packed-f32 one (v_pk_fma_f32, v_pk_add_f32) 3.4 -- it is not hidden at all (tools/bf16_issue_probe.hip)
    // INIT (chunk 0): the first product of each accumulator tile takes a zero C operand -- zeroing 64 registers per item by
    // moves is 64 vector instructions x 4 waves of the SIMD x 4 cycles: 0.6 us of a 21 us item
    auto compute_half = [&](int hbuf, auto nb_tag, auto init_tag) {
        constexpr int nb = decltype(nb_tag)::value;
        constexpr bool INIT = decltype(init_tag)::value;
        if constexpr ((BF3_VAR & 512) != 0 && nb == 1) return;
        const int o = hbuf * G::HB1 + nb * (2 * G::TY * G::HROW);    // tiles 32 .. 63: four tile rows = eight patch rows down
        unsigned hi[2], mid[2], lo[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o0 = o + q * G::CPS;
            const bf3_f2 ac = *reinterpret_cast<const bf3_f2*>(p_ac + o0), ae = *reinterpret_cast<const bf3_f2*>(p_ae + o0);
            const bf3_f2 bc = *reinterpret_cast<const bf3_f2*>(p_bc + o0), be = *reinterpret_cast<const bf3_f2*>(p_be + o0);
            float v0 = __builtin_fmaf(sc, __builtin_fmaf(sr, be.x, ae.x), __builtin_fmaf(sr, bc.x, ac.x));
            float v1 = __builtin_fmaf(sc, __builtin_fmaf(sr, be.y, ae.y), __builtin_fmaf(sr, bc.y, ac.y));
            if constexpr ((BF3_VAR & 2) != 0) {
                v0 = ac.x + ae.x + bc.x + be.x; v1 = ac.y + ae.y + bc.y + be.y;
                hi[q] = __float_as_uint(v0); mid[q] = __float_as_uint(v1); lo[q] = __float_as_uint(v0) ^ 1u;
                continue;
            }
            // exact split: truncations and exact differences; the pair's terms packed [channel 2q + 1 : channel 2q]
            const unsigned h0 = __float_as_uint(v0) & 0xffff0000u, h1 = __float_as_uint(v1) & 0xffff0000u;
            const float r0 = v0 - __uint_as_float(h0), r1 = v1 - __uint_as_float(h1);
            const unsigned m0 = __float_as_uint(r0) & 0xffff0000u, m1 = __float_as_uint(r1) & 0xffff0000u;
            const float l0 = r0 - __uint_as_float(m0), l1 = r1 - __uint_as_float(m1);
            hi[q] = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
            mid[q] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
            if constexpr ((BF3_VAR & 4096) != 0) lo[q] = mid[q];
            else lo[q] = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
        }
        const bf3_u4 b_hm = {hi[0], hi[1], mid[0], mid[1]};
        const bf3_u4 b_mh = {mid[0], mid[1], hi[0], hi[1]};
        const bf3_u4 b_lh = {lo[0], lo[1], hi[0], hi[1]};
        if constexpr ((BF3_VAR & 8) != 0) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[x][nb][r] = (INIT ? 0.0f : acc[x][nb][r]) + __uint_as_float(ua[x][r] ^ b_hm[r]) + __uint_as_float(ul[x][r & 1] ^ b_lh[r]) + __uint_as_float(b_mh[r]);
        } else {
            if constexpr ((BF3_VAR & 256) != 0) __builtin_amdgcn_s_setprio(3);
            if constexpr (BF3_PRIO != 0) __builtin_amdgcn_s_setprio(nb == 0 ? 2 : 0);
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const bf3_u4 a_hl = {ua[x].x, ua[x].y, ul[x].x, ul[x].y};
                if constexpr (INIT) {
                    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_hm), zero, 0, 0, 0);
                } else {
                    acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_hm), acc[x][nb], 0, 0, 0);
                }
                acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_mh), acc[x][nb], 0, 0, 0);
                if constexpr ((BF3_VAR & 4096) == 0)
                    acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, a_hl), __builtin_bit_cast(bf3_bf16x8, b_lh), acc[x][nb], 0, 0, 0);
                if constexpr ((BF3_VAR & 512) != 0) {
                    if constexpr (INIT) {
                        const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                        acc[x][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_hm), zero, 0, 0, 0);
                    } else {
                        acc[x][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_hm), acc[x][1], 0, 0, 0);
                    }
                    acc[x][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_mh), acc[x][1], 0, 0, 0);
                    acc[x][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, a_hl), __builtin_bit_cast(bf3_bf16x8, b_lh), acc[x][1], 0, 0, 0);
                }
            }
            if constexpr ((BF3_VAR & 256) != 0) __builtin_amdgcn_s_setprio(0);
        }
        __builtin_amdgcn_sched_barrier(0);           // what follows stays behind: the registers do not hold both tile blocks
    };

    // ---- the output rounds' scalar operands now (scalar loads: at the end each would be a wait of its own): in round q this
    // wave owns channel co0 + 16 q + wave
    const int cor = wave_u;
    // ---- first loads of the first item
    // The item's GroupNorm operands travel like its first halo chunks: thread t requests channel t's pair ahead (clamped: no
    // branch), the table is written at the top of the item; channels from 1024 up are loaded in place there.
    float gn_pre0 = 0.0f, gn_pre1 = 0.0f;
    auto prefetch_gn = [&] {
        if constexpr (PRO != 0) {
            const int ci = (TAB ? gn_base : b0 * Cin) + min(wave_u * 64 + fresh_lane(), Cin - 1);
            gn_pre0 = p.gn_scale[ci];
            gn_pre1 = p.gn_shift[ci];
        }
    };
    // Where the requests made ahead are waited for.  The compiler counts: "all but the newest N vector-memory operations", N the
    // smallest over all paths that reach the use.  At the top of the item loop the paths are the kernel's entry (nothing behind
    // the requests) and the loop's back edge (the rounds' stores behind them), so a use there is a wait for the STORES of the
    // item before.  The waits are therefore pinned (an empty asm that "modifies" the registers) where every path has the same
    // operations behind the requests: before the loop for the first item, in the last round for the others.
    auto pin_requests = [&] {
#pragma unroll
        for (int i = 0; i < G::EPT; ++i) asm volatile("" : "+v"(hs[0].v[i]));
#pragma unroll
        for (int i = 0; i < G::EPT; ++i) asm volatile("" : "+v"(hs[1].v[i]));
        if constexpr (PRO != 0) asm volatile("" : "+v"(gn_pre0), "+v"(gn_pre1));
    };
    load_halo(0, hs[0]);
    if (live) fetch_u(0, 0);
    if (n > 1) load_halo(1, hs[1]);
    prefetch_gn();
    pin_requests();
    bool first = true;
    bool new_tile = true;            // the item's tile position differs from the one the plan (and the zeroed padding) was made for
  for (;;) {                       // the workgroup's items
#define BF3_STAMP_ITEM L
    BF3_STAMP(0);
    if constexpr (UPS) {            // (the nearest-2x instance has waves without products, whose planes are zero: it zeroes by moves)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[x][nb][r] = 0.0f;
    }
    // (the plan costs ~65 vector instructions per lane, 16 cycles each with four waves on the SIMD: 0.6 us of a 21 us item -- and a
    //  workgroup's items are the same position of successive images whenever gridDim.x / 8 is a multiple of the positions x channel
    //  tiles of an image, as on every layer of the UNet)
    if (new_tile) plan(std::true_type{});
    {   // the store offsets from the thread's own slot (written by the plan: just now, or some items ago)
        const bf3_u2 h = *reinterpret_cast<const bf3_u2*>(smem + G::HOFF_OFF + 2 * (wave_u * 64 + fresh_lane()));
        hoff[0] = (int)(h.x & 0xffffu); hoff[1] = (int)(h.x >> 16); hoff[2] = (int)h.y;
    }
    lane_addresses();
    float tile_cnt = 0.0f, inv_cnt = 0.0f;       // (from the item's record behind the channel loop)
    if constexpr (!TAB) {
        tile_cnt = (float)(min(2 * G::TY, p.Hc - oy0) * min(2 * G::TX, p.Wc - ox0));
        inv_cnt = 1.0f / tile_cnt;
    }
    // the next item's record is asked for here, a channel loop ahead of its use: a line of the scalar cache, not registers
    unsigned it_warm = 0;
    if constexpr (TAB) it_warm = bf3_item_fetch(p.items, min(L + p.grid, p.nwg - 1))[0];

    // (the zeroed padding slots are never staged to: no barrier between the zeroing and the first staging)
    if constexpr (PRO != 0) {
        // both operands requested before either is waited for; the filter fetch behind them -- the compiler's wait for these two
        // is a wait for every vector-memory operation it does not know of as well
        const int c0t = wave_u * 64 + fresh_lane();
        if (c0t < n * W_CIC) {
            const bool cv = c0t < Cin;
            *reinterpret_cast<bf3_f2*>(GN_lds + 2 * c0t) = bf3_f2{cv ? gn_pre0 : 0.0f, cv ? gn_pre1 : 0.0f};
        }
        for (int c = c0t + G::THREADS; c < n * W_CIC; c += G::THREADS) {
            const bool cv = c < Cin;
            const int ci = (TAB ? gn_base : b0 * Cin) + min(c, Cin - 1);
            const float gsc = p.gn_scale[ci], gsh = p.gn_shift[ci];
            *reinterpret_cast<bf3_f2*>(GN_lds + 2 * c) = bf3_f2{cv ? gsc : 0.0f, cv ? gsh : 0.0f};
        }
    }
    // A later item's filter fetch (the first item's went out with its halo): everything requested ahead has been waited for, so
    // no wait of the compiler's stands between this fetch, which it does not know of, and the staging.
    if (!first && live) fetch_u(0, 0);
    first = false;
    if constexpr (PRO != 0) __syncthreads();
    stage_halo(0, 0, hs[0]);
    if (n > 2) load_halo(2, hs[0]);
    __syncthreads();
    if constexpr (TAB) asm volatile("" :: "s"(it_warm));
    BF3_STAMP(1);                                // prologue done
    {
        // chunk c is in halo buffer c & 1 and its A operands in ua.  The staging of chunk c + 1 (GroupNorm, SiLU: latency-bound
        // work) sits BETWEEN the two tile blocks, under the first block's MFMAs: at the end of the body it would be a tail that
        // the last wave runs alone while fifteen wait at the barrier
        // STEADY: chunks c + 1 .. c + 3 exist (the previous body issued its three halo loads after its fetch)
        auto body = [&](const int c, auto par_tag, auto steady_tag, auto init_tag) {
            constexpr int PAR = decltype(par_tag)::value;
            constexpr bool STEADY = decltype(steady_tag)::value;
            if (c == 2 + PAR) BF3_STAMP(2 + 4 * PAR);            // chunks 2 and 3 in detail: start, first block issued + staged, second block issued, barrier passed
            // A wave's issue priority FALLS as it gets through the chunk (3 at its start, 2 at the first tile block's MFMAs, 1 at
            // the second block, 0 at its MFMAs): the SIMD's arbiter serves the oldest wave first, so its four waves (w, w + 4, w + 8,
            // w + 12) arrive at the barrier 0.85 us apart, always in that order, and the chunk ends with the youngest wave working
            // alone (profiles/r04/bf3_wave_skew.txt); a wave that is behind now overtakes the ones ahead.  -1.6 % on a forward's
            // Winograd layers (BF3_PRIO=0: without, A/B); the same bits.
            if constexpr (BF3_PRIO != 0) __builtin_amdgcn_s_setprio(3);
            if (live) {
                // (chunk 0: the three loads of chunk 2's halo are the only requests behind the fetch, whichever item this is)
                if constexpr ((BF3_VAR & 1) == 0) {
                    read_u(BF3_ONE_UA ? 0 : PAR, std::integral_constant<int, STEADY ? 3 : 0>{}, c == 0 && n > 2);
                    if constexpr (BF3_ONE_UA != 0) {
                        // ONE filter buffer: a wave's region is read by that wave only, so once its reads have returned the next
                        // chunk's operands can be fetched over them -- a whole chunk ahead of their use instead of half of one
                        // (the fetch's latency was partly exposed: without the fetches the loop ran 18 % faster)
                        if (STEADY || c + 1 < n) {
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                            fetch_u(c + 1, 0);
                        }
                    }
                }
            }
            if (live) compute_half(PAR, std::integral_constant<int, 0>{}, init_tag);
            if (STEADY || c + 1 < n) {
                // (between the two tile blocks for EVERY wave: with half of a SIMD's waves staging before their first block instead --
                //  so that their vector work would meet the others' MFMAs -- every layer ran 4 - 9 % slower, profiles/r04)
                if constexpr ((BF3_VAR & 4) == 0) stage_halo(c + 1, PAR ^ 1, hs[PAR ^ 1]);
                if constexpr ((BF3_VAR & 1) == 0 && BF3_ONE_UA == 0)
                    if (live) fetch_u(c + 1, PAR ^ 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (c == 2 + PAR) BF3_STAMP(3 + 4 * PAR);
            if constexpr (BF3_PRIO != 0) __builtin_amdgcn_s_setprio(1);
            if (live) compute_half(PAR, std::integral_constant<int, 1>{}, init_tag);
            if constexpr ((BF3_VAR & 36) == 0)
                if (STEADY || c + 3 < n) load_halo(c + 3, hs[PAR ^ 1]);
            if (c == 2 + PAR) BF3_STAMP(4 + 4 * PAR);
            __syncthreads();
            if (c == 2 + PAR) BF3_STAMP(5 + 4 * PAR);
        };
        int c = 0;
        body(0, std::integral_constant<int, 0>{}, std::false_type{}, std::integral_constant<bool, !UPS>{});   // (n >= 1; its fetch was the prologue's)
        c = 1;
        for (; c + 4 < n; c += 2) {
            body(c, std::integral_constant<int, 1>{}, std::true_type{}, std::false_type{});
            body(c + 1, std::integral_constant<int, 0>{}, std::true_type{}, std::false_type{});
        }
        // up to four chunks are left and c is odd: straight-line code (a loop with a run-time buffer parity spills)
        if (c < n) body(c, std::integral_constant<int, 1>{}, std::false_type{}, std::false_type{});
        if (c + 1 < n) body(c + 1, std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});
        if (c + 2 < n) body(c + 2, std::integral_constant<int, 1>{}, std::false_type{}, std::false_type{});
        if (c + 3 < n) body(c + 3, std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});
    }

    BF3_STAMP(10);                               // channel loop done
    if constexpr ((BF3_VAR & 16) != 0) {
        float t = 0.0f;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[x][nb][r];
        if (t == 123.456f) p.out[tid] = t;
        return;
    }
    // (ONE vector load -- lanes 0..3 the bias of the four rounds, lanes 4..7 the embedding -- requested here, after the channel loop (kept across it, it
    //  was a spill), and waited for where it is first used, in the rounds: behind the stores of the item before, the compiler may not turn these into scalar loads any more, and as eight
    //  uniform loads each would be a global load + s_waitcnt vmcnt(0) of its own, 4 us per item)
    const int HWo = p.Hc * p.Wc;
    const int et = fresh_lane(), e_half = et >> 5, e_l31 = et & 31;
    const int ety = et >> 3, etx = et & 7;
    const bool has_res = p.residual != nullptr;
    bool even_w;                                    // uniform: both columns of a tile are inside together, rows are 8-byte aligned
    unsigned ld_off[2][2], st_off[2][2];
    bool pin[2][2];
    __amdgpu_buffer_rsrc_t rso;
    bf3_f2 eres[G::ROUNDS][2];
    float eadd[G::ROUNDS];
    int co0_c, b0_c, slot_c, L_next;
    bool more;
    unsigned stats_base = 0, fin_base = 0;          // (item table: the item's first slot in stats, its first channel in fin_*)
    if constexpr (TAB) {
        // ---- the item's record again, and the next item's with it (both lines are in the scalar cache: the item's top asked for them)
        const bf3_u16 it = bf3_item_fetch(p.items, L);
        const bf3_u16 nx = bf3_item_fetch(p.items, min(L + p.grid, p.nwg - 1));
        const unsigned flags = BF3_IT(it, flags);
        co0_c = (int)BF3_IT(it, co0); b0_c = (int)BF3_IT(it, b0); slot_c = (int)BF3_IT(it, slot);
        stats_base = BF3_IT(it, stats_off); fin_base = BF3_IT(it, fin_off);
        tile_cnt = __uint_as_float(BF3_IT(it, tile_cnt)); inv_cnt = __uint_as_float(BF3_IT(it, inv_cnt));
        even_w = (flags & BF3_IT_EVEN_W) != 0;
        // bias and embedding of the wave's channel in the four rounds: EIGHT scalar loads (constant address space), waited for
        // with the rounds' first LDS traffic -- no vector load whose wait would also be a wait for the residual requests below
        unsigned coc4[G::ROUNDS];
        unsigned ebias[G::ROUNDS], eemb[G::ROUNDS];       // (float bits)
#pragma unroll
        for (int q = 0; q < G::ROUNDS; ++q) {
            coc4[q] = (unsigned)min(co0_c + q * G::RCO + cor, p.Cout - 1);
            ebias[q] = 0u; eemb[q] = 0u;
        }
        typedef const __attribute__((address_space(4))) unsigned* cbits_ptr;
        if (p.bias) {
#pragma unroll
            for (int q = 0; q < G::ROUNDS; ++q) ebias[q] = reinterpret_cast<cbits_ptr>((size_t)p.bias)[coc4[q]];
        }
        if (p.chan_bias) {
            cbits_ptr cb = reinterpret_cast<cbits_ptr>((size_t)p.chan_bias) + BF3_IT(it, cb_off);
#pragma unroll
            for (int q = 0; q < G::ROUNDS; ++q) eemb[q] = cb[coc4[q]];
        }
        // ---- the lanes' pixel offsets.  A tile wholly inside a plane of even width (every item of every UNet layer): affine in
        // the lane, nothing to clamp, every pixel stored; otherwise the clamped offsets and the range-check sentinels
        if ((flags & (BF3_IT_WHOLE | BF3_IT_EVEN_W)) == (BF3_IT_WHOLE | BF3_IT_EVEN_W)) {
            const unsigned o = BF3_IT(it, tile_off) + (unsigned)ety * (8u * (unsigned)p.Wc) + 8u * (unsigned)etx;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    pin[i][j] = true;
                    ld_off[i][j] = st_off[i][j] = o + (unsigned)i * (4u * (unsigned)p.Wc) + 4u * (unsigned)j;
                }
        } else {
            const int eoy = (int)BF3_IT(it, oy0) + 2 * ety, eox = (int)BF3_IT(it, ox0) + 2 * etx;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    pin[i][j] = eoy + i < p.Hc && eox + j < p.Wc;
                    ld_off[i][j] = 4u * (unsigned)(min(eoy + i, p.Hc - 1) * p.Wc + min(eox + j, p.Wc - (even_w ? 2 - j : 1)));
                    st_off[i][j] = pin[i][j] ? ld_off[i][j] : 0x80000000u;
                }
        }
        rso = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)BF3_IT(it, out_off), 0, 4 * p.Cout * HWo, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(has_res ? p.residual + (size_t)BF3_IT(it, out_off) : p.out), 0, 4 * p.Cout * HWo, 0x00020000);
        // ---- the four rounds' residual requests behind ONE decision
#pragma unroll
        for (int q = 0; q < G::ROUNDS; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i) eres[q][i] = bf3_f2{0.0f, 0.0f};
        if (has_res) {
            if (even_w) {
#pragma unroll
                for (int q = 0; q < G::ROUNDS; ++q)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        eres[q][i] = __builtin_bit_cast(bf3_f2, __builtin_amdgcn_raw_buffer_load_b64(rsr, ld_off[i][0], 4u * (coc4[q] * (unsigned)HWo), 0));
            } else {
#pragma unroll
                for (int q = 0; q < G::ROUNDS; ++q)
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        eres[q][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsr, ld_off[i][0], 4u * (coc4[q] * (unsigned)HWo), 0));
                        eres[q][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsr, ld_off[i][1], 4u * (coc4[q] * (unsigned)HWo), 0));
                    }
            }
        }
        // ---- the next item: its first two chunks' halo requested now, staged after the rounds
        L_next = L + p.grid;
        more = (flags & BF3_IT_LAST) == 0;
        if (more) {
            b0 = (int)BF3_IT(nx, b0); co0 = (int)BF3_IT(nx, co0); co_t = co0 >> 6; oy0 = (int)BF3_IT(nx, oy0); ox0 = (int)BF3_IT(nx, ox0);
            gn_base = (int)BF3_IT(nx, gn_off);
            set_sources_item(nx);
            new_tile = (BF3_IT(nx, flags) & BF3_IT_NEW_TILE) != 0;
            if (new_tile) plan(std::false_type{});
            load_halo(0, hs[0]);
            if (n > 1) load_halo(1, hs[1]);
            prefetch_gn();
        }
        // (the eight are first used HERE, behind the requests: pinned, or their sums -- and a wait per load -- move up to the loads)
#pragma unroll
        for (int q = 0; q < G::ROUNDS; ++q) {
            asm volatile("" : "+s"(ebias[q]), "+s"(eemb[q]));
            eadd[q] = (0.0f + __uint_as_float(ebias[q])) + __uint_as_float(eemb[q]);
        }
    } else {
        float eadd_v = 0.0f;
        {
            const int ln = fresh_lane();
            const int coc = min(co0 + (ln & 3) * G::RCO + cor, p.Cout - 1);
            const float* src = ln < 4 ? (p.bias ? p.bias + coc : nullptr)
                                      : (ln < 8 && p.chan_bias ? p.chan_bias + (size_t)b0 * p.chan_bias_stride + coc : nullptr);
            if (src) eadd_v = *src;                      // (one load site: a second assignment behind a pending load would be a wait)
        }
        // ---- output transform: four rounds of 16 channels through LDS, [position][channel][tile]; in a round one wave = one
        // channel x 64 tiles.  Everything global goes through buffer resources: the channel is a scalar offset, the lane's pixel a
        // 32-bit one computed once, and a lane whose pixel is outside the image carries an offset past the image (the range check
        // drops its store) -- no address arithmetic and no exec masks in the rounds.
        const int eoy = oy0 + 2 * ety, eox = ox0 + 2 * etx;
        even_w = (p.Wc & 1) == 0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                pin[i][j] = eoy + i < p.Hc && eox + j < p.Wc;
                // (a lane outside the image re-reads a pixel inside it; with an even width -- the 8-byte residual loads -- the
                //  clamped column is EVEN, Wc - 2, so that the pair it reads ends with the row: ADVICE r03.  The range check of
                //  `rsr` below stays as a second line of defence; it relies on gfx9's raw-buffer rule that the scalar offset
                //  takes part in the check.)
                ld_off[i][j] = 4u * (unsigned)(min(eoy + i, p.Hc - 1) * p.Wc + min(eox + j, p.Wc - (even_w ? 2 - j : 1)));
                st_off[i][j] = pin[i][j] ? ld_off[i][j] : 0x80000000u;      // + the channel offset: still past the image (launch_bf3 checks its size)
            }
        rso = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)b0 * p.Cout * HWo, 0, 4 * p.Cout * HWo, 0x00020000);
        // (range-checked like the output: the 8-byte residual load of a lane clamped to the last column of the last row reads one float
        //  past its image -- past the tensor for the last image; out of range reads return 0 instead)
        const __amdgpu_buffer_rsrc_t rsr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(has_res ? p.residual + (size_t)b0 * p.Cout * HWo : p.out), 0, 4 * p.Cout * HWo, 0x00020000);

#pragma unroll
        for (int q = 0; q < G::ROUNDS; ++q) {
            const int coc = min(co0 + q * G::RCO + cor, p.Cout - 1);
            const unsigned soff = 4u * (unsigned)(coc * HWo);
#pragma unroll
            for (int i = 0; i < 2; ++i) eres[q][i] = bf3_f2{0.0f, 0.0f};
            if (has_res) {
                if (even_w) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        eres[q][i] = __builtin_bit_cast(bf3_f2, __builtin_amdgcn_raw_buffer_load_b64(rsr, ld_off[i][0], soff, 0));
                } else {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        eres[q][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsr, ld_off[i][0], soff, 0));
                        eres[q][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsr, ld_off[i][1], soff, 0));
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < G::ROUNDS; ++q)
            eadd[q] = (0.0f + __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(eadd_v), q))) +
                      __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(eadd_v), 4 + q));
        // ---- the next item: its first two chunks' halo requested now, staged after the rounds
        co0_c = co0; b0_c = b0; slot_c = gy * p.groups_x + gx;
        L_next = L + (int)gridDim.x;
        more = L_next < p.nwg;
        if (more) {
            const int gx_c = gx, gy_c = gy;
            if (img_step) b0 += img_step;
            else decode(L_next);
            set_sources();
            new_tile = gx != gx_c || gy != gy_c;
            if (new_tile) plan(std::false_type{});
            load_halo(0, hs[0]);
            if (n > 1) load_halo(1, hs[1]);
            prefetch_gn();
        }
    }
#pragma unroll
    for (int q = 0; q < G::ROUNDS; ++q) {
        float* const M_lds = M_base + (q & 1) * G::M_ROUND;
        if (q == 0) BF3_STAMP(11);               // round 0 in detail: operands requested, planes written, exchanged, stored
        {
            const int rbase = 8 * (q & 1);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) {
                    const int r = rbase + rr;
                    const int row16 = (r & 3) + 8 * ((r >> 2) & 1) + 4 * e_half;
                    M_lds[(pos * G::RCO + row16) * G::TILES + 32 * nb + e_l31] = acc[q >> 1][nb][r];
                }
        }
        if (q == 0) BF3_STAMP(12);
        __syncthreads();
        if (q == 0) BF3_STAMP(13);
        float mm[4][4];
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) mm[xi >> 2][xi & 3] = M_lds[(xi * G::RCO + cor) * G::TILES + et];
        float sT[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sT[0][j] = mm[0][j] + mm[1][j] + mm[2][j];
            sT[1][j] = mm[1][j] - mm[2][j] - mm[3][j];
        }
        float vv[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            vv[i][0] = sT[i][0] + sT[i][1] + sT[i][2] + eadd[q] + eres[q][i].x;
            vv[i][1] = sT[i][1] - sT[i][2] - sT[i][3] + eadd[q] + eres[q][i].y;
            if (p.relu) { vv[i][0] = fmaxf(vv[i][0], 0.0f); vv[i][1] = fmaxf(vv[i][1], 0.0f); }
        }
        const int co = co0_c + q * G::RCO + cor;
        const bool ok = co < p.Cout;                 // uniform
        const unsigned soff = 4u * (unsigned)(min(co, p.Cout - 1) * HWo);
        // The next item's requests are waited for in front of the LAST round's stores: the compiler's wait is in fact "everything
        // but what was requested after them", stores included -- here the youngest store is a round's exchange and transform
        // old, and the last round's own stores are never waited for.
        if (q == G::ROUNDS - 1) pin_requests();
        // (a channel past the last one stores like a pixel outside the image: to an offset the range check drops -- stores on
        //  every path, so that the compiler's count of the operations behind the next item's requests does not fall to zero)
        if (even_w) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                __builtin_amdgcn_raw_buffer_store_b64(bf3_u2{__float_as_uint(vv[i][0]), __float_as_uint(vv[i][1])}, rso, ok ? st_off[i][0] : 0x80000000u, soff, 0);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[i][0]), rso, ok ? st_off[i][0] : 0x80000000u, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[i][1]), rso, ok ? st_off[i][1] : 0x80000000u, soff, 0);
            }
        }
        if (q == 0) BF3_STAMP(14);
        if (!WINO_TIMING && (p.stats || (!UPS && p.fin_gamma))) {
            // one channel per wave (its 64 lanes = the 64 tiles): (count, sum, M2) of what this workgroup stored of the channel,
            // sums shifted by the first tile's first value
            // (lane 0's value: with the item table as a scalar -- the shuffle's lane address was one more register kept across the channel loop)
            const float K = TAB ? __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(vv[0][0]), 0)) : __shfl(vv[0][0], 0);
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float d0 = pin[i][0] ? vv[i][0] - K : 0.0f, d1 = pin[i][1] ? vv[i][1] - K : 0.0f;
                s1 += d0 + d1;
                s2 = fmaf(d0, d0, fmaf(d1, d1, s2));
            }
            s1 = wave64_sum(s1);
            s2 = wave64_sum(s2);
            if (ok && et == 0) {
                const float p_sum = fmaf(tile_cnt, K, s1), p_m2 = fmaxf(s2 - s1 * s1 * inv_cnt, 0.0f);
                if (p.stats) {
                    const int slots = p.groups_x * p.groups_y;
                    float4* dst = TAB ? reinterpret_cast<float4*>(p.stats) + ((size_t)stats_base + (size_t)((q * G::RCO + cor) * slots))
                                      : reinterpret_cast<float4*>(p.stats) + ((size_t)b0_c * p.Cout + co) * slots + slot_c;
                    *dst = make_float4(tile_cnt, p_sum, p_m2, 0.0f);
                }
                if (!UPS && p.fin_gamma) *reinterpret_cast<bf3_f2*>(smem + G::FIN_OFF + 2 * (q * G::RCO + cor)) = bf3_f2{p_sum, p_m2};
            }
        }
    }
#if WINO_TIMING
    if (!more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    BF3_STAMP(15);                               // the item's end (the last item's: stores retired)
#undef BF3_STAMP_ITEM
    if (!UPS && p.fin_gamma) {          // (not in the nearest-2x instance: conv_finalizes)
        // The tile is the whole image (launcher): the workgroup holds all of the image's values of its 64 channels = eight whole
        // GroupNorm groups of eight.  Channel c's thread merges its group's eight partials in the order and with the operations
        // of gn_finalize_kernel (its lanes 0 .. 7 through the 64-lane butterfly; gn_merge.h) and writes the channel's (scale, shift):
        // the bits sisic_groupnorm_finalize would give, without its launch.
        __syncthreads();
        // (with the item table from the hardware's lane index, as everywhere in the per-item code: the thread index was a register
        //  pair kept across the channel loop for this one use, and the table instances have none to spare)
        const int c = TAB ? wave_u * 64 + fresh_lane() : tid;
        if (c < G::CO_T) {
            const bf3_f2* ps = reinterpret_cast<const bf3_f2*>(smem + G::FIN_OFF) + 8 * (c >> 3);
            double pn[8], s1v[8], m2v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { pn[i] = (double)tile_cnt + (double)0.0f; s1v[i] = (double)ps[i].x + (double)0.0f; m2v[i] = (double)ps[i].y + (double)0.0f; }
            auto tree = [](const double (&v)[8]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); };
            const double nn = tree(pn), sum1 = tree(s1v), sum2 = tree(m2v);
            const double mean = sum1 / nn;
            double bt[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) bt[i] = 0.0 + gn_between_term(tile_cnt, ps[i].x, mean);
            const double between = tree(bt);
            float meanf, rstd;
            gn_mean_rstd(nn, sum1, sum2, between, p.fin_eps, meanf, rstd, mean);
            const int co = co0_c + c;
            float sc, sh;
            gn_affine(p.fin_gamma[co], p.fin_beta[co], meanf, rstd, sc, sh);
            const size_t fi = TAB ? (size_t)fin_base + (size_t)c : (size_t)b0_c * p.Cout + co;
            p.fin_scale[fi] = sc;
            p.fin_shift[fi] = sh;
            if (p.fin_mean_rstd && (c & 7) == 0) {
                p.fin_mean_rstd[2 * ((size_t)b0_c * p.fin_groups + (co >> 3))] = meanf;
                p.fin_mean_rstd[2 * ((size_t)b0_c * p.fin_groups + (co >> 3)) + 1] = rstd;
            }
        }
    }
    if (!more) break;
    L = L_next;
    __syncthreads();                             // the rounds' last LDS reads are done: the padding slots are zeroed and chunk 0 staged over them
  }
}

#define BF3_STAMP_ITEM blockIdx.x
// ---- the 8x8 level: FOUR images of at most 8 x 8 pixels (16 tiles each) per workgroup, input channels split over p.ksplit
// workgroups whose raw partial outputs splitk_reduce_kernel sums (bias, embedding, residual, ReLU and GroupNorm partials move
// into the reduction, as for tile_cfg 90 / 91).  tile_cfg 92.  Same arithmetic, same wave roles as conv_winograd_bf3_kernel:
//   tile t = lane of the output rounds = (image t >> 4, tile row (t >> 2) & 3, tile column t & 3)
//   staging: thread r < 100 of a channel's 128 owns halo element r of ALL FOUR images (10 x 10 each: one lane offset and one
//   LDS offset serve the four, the image is a scalar offset -- also across the concat seam, whose sources have different image
//   strides); an image past the batch stages zeros
struct Bf3QGeom {
    static constexpr int CO_T = 64, NW = 16, THREADS = 1024, TILES = 64, IMGS = 4;
    static constexpr int HH = 10, HWD = 10, HROW = 12, HPL = 6;      // a row: [even columns 0..4, spare][odd columns 0..4, spare]
    static constexpr int HPI = HH * HWD;                           // 100 staged elements per channel and image
    static constexpr int IMG = 2 * HH * HROW + 8;                  // 248 floats per image of a channel pair (+8: the images' tiles on different banks)
    static constexpr int HB1 = IMGS * IMG;                         // 992 floats: one channel PAIR in one buffer
    static constexpr int CPS = 2 * HB1;                            // [channel pair][buffer][image][row][plane][6][2 channels]
    static constexpr int H_FLOATS = (W_CIC / 2) * CPS;             // 7936 floats = 31 KB
    static constexpr int GN_MAX_CH = 512;                          // (scale, shift) of four images x this many channels
    static constexpr int UA_WAVE = 768, UA_BUF = NW * UA_WAVE;
    static constexpr int UA_OFF = H_FLOATS + 2 * IMGS * GN_MAX_CH;
    static constexpr int LOOP_FLOATS = UA_OFF + 2 * UA_BUF;        // 31 + 16 + 96 KB
    static constexpr int RCO = 16, ROUNDS = CO_T / RCO, M_ROUND = 16 * RCO * TILES, EPI_FLOATS = 2 * M_ROUND;
    static constexpr size_t LDS_BYTES = sizeof(float) * (size_t)(LOOP_FLOATS > EPI_FLOATS ? LOOP_FLOATS : EPI_FLOATS);
};

template <int PRO>
__global__ void __launch_bounds__(1024, 4) conv_winograd_bf3q_kernel(const WinoParams p) {
    using G = Bf3QGeom;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const H_lds = smem;
    float* const GN_lds = smem + G::H_FLOATS;                                   // [image][input channel][scale, shift]
    float* const M_base = smem;

    int work;
    {   // XCD-aware bijective remap (conv_mfma.hip)
        const int L = blockIdx.x, nwg = p.nwg;
        const int xcd = L & 7, slot = L >> 3, q = nwg >> 3, r = nwg & 7;
        work = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    }
    int co_t = work % p.n_co_tiles;
    const int rest = work / p.n_co_tiles;
    int ks = rest % p.ksplit, quad = rest / p.ksplit;
    // (the divisions run on the vector unit: without this the scalar offsets derived from them sit in vector registers and
    //  every buffer load gets a waterfall loop, conv_pointwise_bf3.hip)
    asm volatile("" : "+s"(co_t), "+s"(ks), "+s"(quad));
    const int b0 = G::IMGS * quad;
    const int co0 = co_t * G::CO_T;
    const int n = p.nchunks / p.ksplit, c_begin = ks * n;           // this workgroup's chunks: c_begin .. c_begin + n - 1

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int HWin = p.Hin * p.Win, Cin = p.c0 + p.c1;
    float* const UA_lds = smem + G::UA_OFF + wave_u * G::UA_WAVE;
    const unsigned ua_lds_addr = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)UA_lds);

    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in0 + (size_t)b0 * p.c0 * HWin), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in1 ? p.in1 + (size_t)b0 * p.c1 * HWin : p.in0), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.uw), 0, -1, 0x00020000);

    // ---- staging plan
    const int sci = wave_u >> 1;
    const int sl = tid & 127;
    unsigned goff;
    int hoff;
    {
        const bool in = sl < G::HPI;
        const int ec = in ? sl : 0;
        const int yy = ec / G::HWD, xx = ec % G::HWD;
        const int y = yy - 1, x = xx - 1;
        const bool v = in && y >= 0 && y < p.Hc && x >= 0 && x < p.Wc;
        const int slot = yy * G::HROW + (xx & 1) * G::HPL + (xx >> 1);
        goff = v ? 4u * (unsigned)(y * p.Win + x) : 0u;
        hoff = 2 * (v ? slot : (G::HPL - 1) + G::HPL * (sl & 1));
        if (in && !v) {
            float* z = H_lds + (sci >> 1) * G::CPS + 2 * slot + (sci & 1);
#pragma unroll
            for (int i = 0; i < G::IMGS; ++i) {
                z[i * G::IMG] = 0.0f;
                z[G::HB1 + i * G::IMG] = 0.0f;
            }
        }
    }
    // images of the quad that exist (the last quad of a batch that is not a multiple of four); their byte offsets in either
    // source, as scalars (an image past the batch re-reads the last one and stages zeros)
    const int n_img = min(G::IMGS, p.B - b0);
    unsigned io0[G::IMGS], io1[G::IMGS];
#pragma unroll
    for (int i = 0; i < G::IMGS; ++i) {
        io0[i] = 4u * (unsigned)(min(i, n_img - 1) * p.c0 * HWin);
        io1[i] = 4u * (unsigned)(min(i, n_img - 1) * p.c1 * HWin);
        asm volatile("" : "+s"(io0[i]), "+s"(io1[i]));
    }

    const int pos = wave_u, pi = pos >> 2, pj = pos & 3;
    const int ra = (pi == 0) ? 0 : (pi == 2 ? 2 : 1), rb = (pi == 2) ? 1 : (pi == 3 ? 3 : 2);
    const int ca = (pj == 0) ? 0 : (pj == 2 ? 2 : 1), cb = (pj == 2) ? 1 : (pj == 3 ? 3 : 2);
    const float sr = (pi == 1) ? 1.0f : -1.0f, sc = (pj == 1) ? 1.0f : -1.0f;
    // lane = (tile l31 of the block, channel group half): image l31 >> 4 (+ 2 for the second block), tile row, tile column
    const int timg = l31 >> 4, ty = (l31 >> 2) & 3, tx = l31 & 3;
    const int xf_lane = (2 * half) * G::CPS + timg * G::IMG + 2 * ((2 * ty) * G::HROW + tx);
    const int col_a = (ca & 1) * G::HPL + (ca >> 1), col_b = (cb & 1) * G::HPL + (cb >> 1);
    const float* const p_ac = H_lds + xf_lane + 2 * (ra * G::HROW + col_a);
    const float* const p_ae = H_lds + xf_lane + 2 * (ra * G::HROW + col_b);
    const float* const p_bc = H_lds + xf_lane + 2 * (rb * G::HROW + col_a);
    const float* const p_be = H_lds + xf_lane + 2 * (rb * G::HROW + col_b);

    const int n_co32 = p.cout_pad >> 5;
    const unsigned u_lane = 16u * (unsigned)lane;

    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][nb][r] = 0.0f;

    struct HaloRegs {
        float v[G::IMGS];
        bool cval = false;
    };
    HaloRegs hs;
    bf3_u4 ua[2];
    bf3_u2 ul[2];

    auto load_halo = [&](int chunk, HaloRegs& h) {                  // chunk: absolute
        const int c = chunk * W_CIC + sci;
        h.cval = c < Cin;
        const int hcc = min(c, Cin - 1);
        if (hcc < p.c0) {
            const unsigned soff = 4u * (unsigned)(hcc * HWin);
#pragma unroll
            for (int i = 0; i < G::IMGS; ++i)
                h.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs0, goff, soff + io0[i], 0));
        } else {
            const unsigned soff = 4u * (unsigned)((hcc - p.c0) * HWin);
#pragma unroll
            for (int i = 0; i < G::IMGS; ++i)
                h.v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs1, goff, soff + io1[i], 0));
        }
    };
    auto stage_halo = [&](int chunk, int hbuf, const HaloRegs& h) {
        float* dst = H_lds + (sci >> 1) * G::CPS + hbuf * G::HB1 + (sci & 1);
#pragma unroll
        for (int i = 0; i < G::IMGS; ++i) {
            float v = h.v[i];
            const bool keep = h.cval && i < n_img;                  // a channel past the last one / an image past the batch: zeros
            if constexpr (PRO != 0) {
                const bf3_f2 g = *reinterpret_cast<const bf3_f2*>(GN_lds + 2 * (i * G::GN_MAX_CH + chunk * W_CIC + sci));
                v = v * g.x + g.y;                                  // (the table holds zeros where keep is false)
                if constexpr (PRO == 2) v = wsilu(v);
            } else {
                v = keep ? v : 0.0f;
            }
            dst[hoff + i * G::IMG] = v;
        }
    };
    auto fetch_u = [&](int chunk, int ubuf) {
        const unsigned s0 = 3072u * (unsigned)(((chunk * 16 + pos) * (n_co32 >> 1)) + co_t);
        const unsigned dst = ua_lds_addr + 4u * (unsigned)(ubuf * G::UA_BUF);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                         :: "s"(dst + 1024u * (unsigned)k), "v"(u_lane), "s"(rsu), "s"(s0 + 1024u * (unsigned)k) : "memory");
        if constexpr ((BF3_VAR & 1024) != 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                             :: "s"(dst + 4u * (unsigned)G::UA_BUF + 1024u * (unsigned)k), "v"(u_lane), "s"(rsu), "s"(s0 + 1024u * (unsigned)k) : "memory");
        }
    };
    // steady: the previous body issued its four halo loads after the fetch of this chunk and nothing else since
    auto read_u = [&](int ubuf, bool steady) {
        if (!WINO_TIMING && steady) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const float* const src = UA_lds + ubuf * G::UA_BUF;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            ua[x] = *reinterpret_cast<const bf3_u4*>(src + 256 * x + 4 * lane);
            ul[x] = *reinterpret_cast<const bf3_u2*>(src + 512 + 128 * x + 2 * lane);
        }
    };
    auto compute_half = [&](int hbuf, auto nb_tag) {
        constexpr int nb = decltype(nb_tag)::value;
        const int o = hbuf * G::HB1 + nb * (2 * G::IMG);            // tiles 32 .. 63: images 2 and 3
        unsigned hi[2], mid[2], lo[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o0 = o + q * G::CPS;
            const bf3_f2 ac = *reinterpret_cast<const bf3_f2*>(p_ac + o0), ae = *reinterpret_cast<const bf3_f2*>(p_ae + o0);
            const bf3_f2 bc = *reinterpret_cast<const bf3_f2*>(p_bc + o0), be = *reinterpret_cast<const bf3_f2*>(p_be + o0);
            const float v0 = __builtin_fmaf(sc, __builtin_fmaf(sr, be.x, ae.x), __builtin_fmaf(sr, bc.x, ac.x));
            const float v1 = __builtin_fmaf(sc, __builtin_fmaf(sr, be.y, ae.y), __builtin_fmaf(sr, bc.y, ac.y));
            const unsigned h0 = __float_as_uint(v0) & 0xffff0000u, h1 = __float_as_uint(v1) & 0xffff0000u;
            const float r0 = v0 - __uint_as_float(h0), r1 = v1 - __uint_as_float(h1);
            const unsigned m0 = __float_as_uint(r0) & 0xffff0000u, m1 = __float_as_uint(r1) & 0xffff0000u;
            const float l0 = r0 - __uint_as_float(m0), l1 = r1 - __uint_as_float(m1);
            hi[q] = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
            mid[q] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
            lo[q] = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
        }
        const bf3_u4 b_hm = {hi[0], hi[1], mid[0], mid[1]};
        const bf3_u4 b_mh = {mid[0], mid[1], hi[0], hi[1]};
        const bf3_u4 b_lh = {lo[0], lo[1], hi[0], hi[1]};
        if constexpr (BF3_PRIO != 0) __builtin_amdgcn_s_setprio(nb == 0 ? 2 : 0);       // (falling priority, as in conv_winograd_bf3_kernel)
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const bf3_u4 a_hl = {ua[x].x, ua[x].y, ul[x].x, ul[x].y};
            acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_hm), acc[x][nb], 0, 0, 0);
            acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, ua[x]), __builtin_bit_cast(bf3_bf16x8, b_mh), acc[x][nb], 0, 0, 0);
            acc[x][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf3_bf16x8, a_hl), __builtin_bit_cast(bf3_bf16x8, b_lh), acc[x][nb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- first loads; the GroupNorm table of the four images (zeros for channels / images that do not exist)
    load_halo(c_begin, hs);
    fetch_u(c_begin, 0);
    if constexpr (PRO != 0) {
        for (int j = tid; j < G::IMGS * p.nchunks * W_CIC; j += G::THREADS) {
            const int i = j / (p.nchunks * W_CIC), c = j % (p.nchunks * W_CIC);
            const bool cv = c < Cin && i < n_img;
            GN_lds[2 * (i * G::GN_MAX_CH + c)] = cv ? p.gn_scale[(b0 + i) * Cin + c] : 0.0f;
            GN_lds[2 * (i * G::GN_MAX_CH + c) + 1] = cv ? p.gn_shift[(b0 + i) * Cin + c] : 0.0f;
        }
        __syncthreads();
    }
    stage_halo(c_begin, 0, hs);
    if (n > 1) load_halo(c_begin + 1, hs);
    __syncthreads();
    {
        auto body = [&](const int k, auto par_tag) {               // k: chunk index inside this workgroup's range
            constexpr int PAR = decltype(par_tag)::value;
            if constexpr (BF3_PRIO != 0) __builtin_amdgcn_s_setprio(3);
            read_u(PAR, k >= 1 && k + 1 < n);
            compute_half(PAR, std::integral_constant<int, 0>{});
            if (k + 1 < n) {
                stage_halo(c_begin + k + 1, PAR ^ 1, hs);
                fetch_u(c_begin + k + 1, PAR ^ 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (BF3_PRIO != 0) __builtin_amdgcn_s_setprio(1);
            compute_half(PAR, std::integral_constant<int, 1>{});
            if (k + 2 < n) load_halo(c_begin + k + 2, hs);
            __syncthreads();
        };
        int k = 0;
#if (BF3Q_VAR & 1) == 0            // BF3Q_VAR: timing-only builds (wrong results): bit 0 no channel loop, bit 1 no output rounds
        for (; k + 1 < n; k += 2) {
            body(k, std::integral_constant<int, 0>{});
            body(k + 1, std::integral_constant<int, 1>{});
        }
        if (k < n) body(k, std::integral_constant<int, 0>{});
#endif
    }
#if (BF3Q_VAR & 2) != 0
    {
        float t = 0.0f;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[x][nb][r];
        if (t == 123.456f) p.part[tid] = t;
        return;
    }
#endif

    // ---- output rounds: raw partial sums into this workgroup's slab [ks][B][Cout][Hc][Wc]
    const int HWo = p.Hc * p.Wc;
    const int et = lane, eimg = et >> 4, ety = (et >> 2) & 3, etx = et & 3;
    const int eoy = 2 * ety, eox = 2 * etx;
    const int cor = wave_u;
    const bool even_w = (p.Wc & 1) == 0;
    unsigned st_off[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool in = eimg < n_img && eoy + i < p.Hc && eox + j < p.Wc;
            st_off[i][j] = in ? 4u * (unsigned)(eimg * p.Cout * HWo + (eoy + i) * p.Wc + eox + j) : 0x80000000u;
        }
    const __amdgpu_buffer_rsrc_t rso = __builtin_amdgcn_make_buffer_rsrc(
        p.part + ((size_t)ks * p.B + b0) * p.Cout * HWo, 0, 4 * n_img * p.Cout * HWo, 0x00020000);
#pragma unroll
    for (int q = 0; q < G::ROUNDS; ++q) {
        float* const M_lds = M_base + (q & 1) * G::M_ROUND;
        {
            const int rbase = 8 * (q & 1);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) {
                    const int r = rbase + rr;
                    const int row16 = (r & 3) + 8 * ((r >> 2) & 1) + 4 * half;
                    M_lds[(pos * G::RCO + row16) * G::TILES + 32 * nb + l31] = acc[q >> 1][nb][r];
                }
        }
        __syncthreads();
        float mm[4][4];
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) mm[xi >> 2][xi & 3] = M_lds[(xi * G::RCO + cor) * G::TILES + et];
        float sT[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sT[0][j] = mm[0][j] + mm[1][j] + mm[2][j];
            sT[1][j] = mm[1][j] - mm[2][j] - mm[3][j];
        }
        float vv[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            vv[i][0] = sT[i][0] + sT[i][1] + sT[i][2];
            vv[i][1] = sT[i][1] - sT[i][2] - sT[i][3];
        }
        const int co = co0 + q * G::RCO + cor;
        if (co < p.Cout) {
            const unsigned soff = 4u * (unsigned)(co * HWo);
            if (even_w) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    __builtin_amdgcn_raw_buffer_store_b64(bf3_u2{__float_as_uint(vv[i][0]), __float_as_uint(vv[i][1])}, rso, st_off[i][0], soff, 0);
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[i][0]), rso, st_off[i][0], soff, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(vv[i][1]), rso, st_off[i][1], soff, 0);
                }
            }
        }
    }
}

// third packing of U = G g G^T (winograd_pack_bf3_elem, pack_device.h): the A operands of the three MFMAs
__global__ void winograd_pack_bf3_kernel(const float* __restrict__ u_first, int cin_pad, int cout_pad, int cout_pad128,
                                         unsigned* __restrict__ out) {
    const size_t total = (size_t)(cin_pad / 8) * 16 * (cout_pad128 / 64) * 768;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        winograd_pack_bf3_elem(i, u_first, cout_pad, cout_pad128, out);
}

// The geometry's item table (p.items): from the context's cache, or filled now by a kernel on the launch stream -- ordered in
// front of the convolution, legal under stream capture, no host staging.  p.items stays null -- the kernel then derives the
// items itself -- when SISIC_BF3_ITEM_TABLE=0, when an offset of the geometry does not fit 32 bits, when the cache is full
// (tables are never evicted: captured graphs hold their addresses) or when a new geometry is first met during a capture.
static int bf3_item_table(sisic_ctx* ctx, WinoParams& p, hipStream_t s) {
    constexpr size_t MAX_TABLES = 48, MAX_BYTES = size_t(8) << 20;
    const char* e = std::getenv("SISIC_BF3_ITEM_TABLE");      // (read per launch: tests and A/B runs switch it inside one process)
    if (e && std::atoi(e) == 0) return SISIC_OK;
    const double HWin = (double)p.Hin * p.Win, HWo = (double)p.Hc * p.Wc, lim = 4294967296.0;
    const double slots = (double)p.groups_x * p.groups_y;
    if ((double)p.B * std::max(p.c0, p.c1) * HWin >= lim || (double)p.B * p.Cout * HWo >= lim || (double)p.B * (p.c0 + p.c1) >= lim ||
        (double)p.B * std::max(p.chan_bias_stride, 0) >= lim || (double)p.B * round_up(p.Cout, 64) * slots >= lim || p.chan_bias_stride < 0 ||
        (size_t)p.nwg * sizeof(Bf3Item) > MAX_BYTES)
        return SISIC_OK;
    const int key[9] = {p.B, p.Hin, p.Win, p.ups, p.c0, p.c1, p.Cout, p.grid, p.chan_bias_stride};
    std::lock_guard<std::mutex> lock(ctx->bf3_items_mutex);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SISIC_HIP(hipStreamIsCapturing(s, &cap));
    for (auto& it : ctx->bf3_items) {
        if (!std::equal(key, key + 9, it.key)) continue;
        // another stream's launches are not ordered behind the fill until its event has passed
        if (it.fill_done && cap == hipStreamCaptureStatusNone && hipEventQuery(it.fill_done) == hipSuccess) {
            (void)hipEventDestroy(it.fill_done);
            it.fill_done = nullptr;
        }
        if (!it.fill_done || it.fill_stream == s) p.items = it.tab;
        return SISIC_OK;
    }
    if (ctx->bf3_items.size() >= MAX_TABLES || cap != hipStreamCaptureStatusNone) return SISIC_OK;
    sisic_ctx::Bf3Items ent;
    std::copy(key, key + 9, ent.key);
    SISIC_HIP(hipMalloc(reinterpret_cast<void**>(&ent.tab), (size_t)p.nwg * sizeof(Bf3Item)));
    hipLaunchKernelGGL(bf3_item_table_kernel, dim3(cdiv(p.nwg, 256)), dim3(256), 0, s, p, ent.tab);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(ent.tab);
        set_error("conv2d(winograd bf16x3): item table kernel failed to launch");
        return SISIC_EHIP;
    }
    ent.fill_stream = s;
    if (hipEventCreateWithFlags(&ent.fill_done, hipEventDisableTiming) != hipSuccess || hipEventRecord(ent.fill_done, s) != hipSuccess) {
        // (no event: the table is used once the stream has drained)
        if (ent.fill_done) (void)hipEventDestroy(ent.fill_done);
        ent.fill_done = nullptr;
        SISIC_HIP(hipStreamSynchronize(s));
    }
    ctx->bf3_items.push_back(ent);
    p.items = ent.tab;
    return SISIC_OK;
}

template <int PRO, bool UPS>
static int launch_bf3(sisic_ctx* ctx, WinoParams& p, hipStream_t s) {
    using G = Bf3Geom<PRO>;
    p.groups_x = cdiv(p.Wc, 2 * G::TX);
    p.groups_y = cdiv(p.Hc, 2 * G::TY);
    p.groups_b = p.B;
    p.n_co_tiles = cdiv(p.Cout, G::CO_T);
    p.nchunks = cdiv(p.c0 + p.c1, W_CIC);
    p.ksplit = 1;
    const int64_t nwg = (int64_t)p.groups_x * p.groups_y * p.groups_b * p.n_co_tiles;
    SISIC_REQUIRE(nwg > 0 && nwg < (int64_t(1) << 31), "conv2d(winograd bf16x3): grid too large");
    SISIC_REQUIRE((double)round_up(p.c0 + p.c1, 16) * 32.0 * p.cout_pad * 4.0 < 4294967296.0, "conv2d(winograd bf16x3): filter tensor too large for 32-bit offsets");
    SISIC_REQUIRE((double)p.Cout * p.Hc * p.Wc * 4.0 < 2147483648.0, "conv2d(winograd bf16x3): one image of the output is too large for 31-bit offsets");
    SISIC_REQUIRE(p.nchunks * W_CIC <= G::GN_MAX_CH, "conv2d(winograd bf16x3): more than %d input channels", G::GN_MAX_CH);
    p.nwg = (int)nwg;
    // persistent workgroups (one per CU: its LDS lets no second one in) when there are more items than CUs, unless
    // SISIC_BF3_PERSISTENT=0; the grid a multiple of 8 so that an item's XCD is its workgroup's
    static const bool persistent = [] { const char* e = std::getenv("SISIC_BF3_PERSISTENT"); return !e || std::atoi(e) != 0; }();
    const int cus = ctx->num_cus > 0 ? ctx->num_cus & ~7 : 256;
    const int grid = (persistent && p.nwg > cus && cus >= 8) ? cus : p.nwg;
    p.grid = grid;
    p.items = nullptr;
    SISIC_TRY(bf3_item_table(ctx, p, s));
    if (p.items) {
        auto kern = conv_winograd_bf3_kernel<PRO, UPS, true>;
        static std::atomic<uint64_t> lds_opt_in{0};
        SISIC_TRY(ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, lds_opt_in));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(G::THREADS), G::LDS_BYTES, s, p);
    } else {
        auto kern = conv_winograd_bf3_kernel<PRO, UPS, false>;
        static std::atomic<uint64_t> lds_opt_in{0};
        SISIC_TRY(ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, lds_opt_in));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(G::THREADS), G::LDS_BYTES, s, p);
    }
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

template <int PRO>
static int launch_bf3q(sisic_ctx* ctx, WinoParams& p, hipStream_t s) {
    using G = Bf3QGeom;
    p.n_co_tiles = cdiv(p.Cout, G::CO_T);
    p.nchunks = cdiv(p.c0 + p.c1, W_CIC);
    const int64_t nwg = (int64_t)cdiv(p.B, G::IMGS) * p.n_co_tiles * p.ksplit;
    SISIC_REQUIRE(nwg > 0 && nwg < (int64_t(1) << 31), "conv2d(winograd bf16x3, 8x8): grid too large");
    SISIC_REQUIRE(p.nchunks % p.ksplit == 0 && p.nchunks * W_CIC <= G::GN_MAX_CH,
                  "conv2d(winograd bf16x3, 8x8): needs a multiple of %d and at most %d input channels", p.ksplit * W_CIC, G::GN_MAX_CH);
    SISIC_REQUIRE(4.0 * G::IMGS * std::max(p.c0, p.c1) * p.Hin * p.Win < 4294967296.0 && 4.0 * G::IMGS * p.Cout * p.Hc * p.Wc < 2147483648.0,
                  "conv2d(winograd bf16x3, 8x8): tensor too large for 32-bit offsets");
    p.nwg = (int)nwg;
    auto kern = conv_winograd_bf3q_kernel<PRO>;
    static std::atomic<uint64_t> lds_opt_in{0};
    SISIC_TRY(ensure_dynamic_lds(ctx, reinterpret_cast<const void*>(kern), (int)G::LDS_BYTES, lds_opt_in));
    hipLaunchKernelGGL(kern, dim3(p.nwg), dim3(G::THREADS), G::LDS_BYTES, s, p);
    SISIC_HIP(hipGetLastError());
    return SISIC_OK;
}

static int launch_bf3q_pro(sisic_ctx* ctx, WinoParams& p, hipStream_t s) {
    const int pro = (p.gn_scale == nullptr) ? 0 : (p.gn_silu ? 2 : 1);
    if (pro == 2) return launch_bf3q<2>(ctx, p, s);
    if (pro == 1) return launch_bf3q<1>(ctx, p, s);
    return launch_bf3q<0>(ctx, p, s);
}

static int launch_bf3_pro(sisic_ctx* ctx, WinoParams& p, hipStream_t s) {
    const int pro = (p.gn_scale == nullptr) ? 0 : (p.gn_silu ? 2 : 1);
    if (p.ups) {
        if (pro == 2) return launch_bf3<2, true>(ctx, p, s);
        if (pro == 1) return launch_bf3<1, true>(ctx, p, s);
        return launch_bf3<0, true>(ctx, p, s);
    }
    if (pro == 2) return launch_bf3<2, false>(ctx, p, s);
    if (pro == 1) return launch_bf3<1, false>(ctx, p, s);
    return launch_bf3<0, false>(ctx, p, s);
}
