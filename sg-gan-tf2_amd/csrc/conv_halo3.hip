// conv_halo3.hip -- the 3x3 stride-1 "same" convolution with the input halo resident in LDS: forward and data gradient (incl.
// MirrorPadGrad) of the generators' 18 residual-block convs (module.py:210-216), bf16, NHWC; and the lab build's clock stamps.
// conv.hip routes a layer here (halo3_ok) and keeps the kernel that pre-folds the REFLECT side tensor it reads.
#include "conv_internal.h"

#ifdef SGG_LAB
// debug aid (SGG_ABLATE=9): shader-clock and wall-clock timestamps of one block of the halo GEMM, read by sgg_debug_clocks()
__device__ unsigned long long g_dbg_clk[4];
// SGG_ABLATE=8: shader-clock stamps of block 0, per wave, at six points of each of 16 mid-loop tiles
// [wave][tile][point]: 0 loop top, 1 refill DMAs issued, 2 all MFMAs issued, 3 vmcnt(0) passed, 4 lgkmcnt(0) passed, 5 barrier passed
__device__ unsigned long long g_dbg_phase[8][16][6];
#define H3_CLOCKS(i) do { if (dbg_clk) { g_dbg_clk[i] = clock64(); g_dbg_clk[(i) + 1] = wall_clock64(); } } while (0)
#else
#define H3_CLOCKS(i) do {} while (0)
#endif

// -------------------------------------------------------------------------------------------------
// 3x3 stride-1 "same" convolution with the INPUT HALO RESIDENT IN LDS (the 18 residual-block convs of the
// generator, module.py:210-216, are this shape at C = K = 256).
//
// conv_gemm_glds_kernel re-fetches a pixel tile once per tap (9x) from L2; at 256x256 tiles that kernel is bound by
// the L2->LDS stream (DMA-only 62 us vs 49 us of MFMA).  Here a block owns 2 output rows x 128
// columns; per 64-channel chunk the 4 x 130 input pixels it needs sit in LDS once (REFLECT / zero padding resolved
// in the DMA's per-lane source address) and the 9 taps read shifted rows of that image, so the pixel operand costs
// 68 KB instead of 288 KB per chunk and only the weight tiles stream per tap (-38 % L2->LDS bytes overall).
// The halo is single-buffered and refilled row by row while other rows are in use: kernel row r touches halo rows
// r and r+1 only, so row 0 of the next chunk is loaded during r=1, row 1 during r=2, rows 2/3 during r=0/1 of the
// next chunk.  K order: chunk-major, tap-minor.  Weight tiles: the same 2-stage DMA ring as conv_gemm_glds_kernel's (conv.hip).
// -------------------------------------------------------------------------------------------------
#define H3_TW 128
#ifndef H3_ISSUER_HALF
#define H3_ISSUER_HALF 1                               // which half of the waves (0: waves 0-3, 1: waves 4-7) issues the main loop's weight DMAs
#endif
#ifndef H3_HALO_HALF
#define H3_HALO_HALF 1                                 // ... and which half the halo-row DMAs (the other half measured 3-6 % slower:
#endif                                                 //     the non-issuers' early MFMAs are what covers the issuers' DMA phase)
#ifndef H3_GJ
#define H3_GJ 4                                        // pixel fragments per MFMA group of the main loop (x 4 weight fragments = 16 MFMAs)
#endif
#ifndef H3_NORM_AT
#define H3_NORM_AT 1                                   // NORM: after which MFMA group of the step (0..3) the row transform runs
#endif
// Forms of this kernel that were built, measured bit-identical and slower (or no faster), and then REMOVED from the source --
// the numbers stay under profiles/:
//   persistent blocks walking consecutive tiles, next prologue under the epilogue: forward flat, data gradient spills and is
//       15 % slower; one half of the waves lagging half a tile: forward -1 % at best, data gradient 2x slower; halo rows
//       issued late by the non-issuer waves: 2-3.5 % slower; issuers' fragment reads ahead of their DMA issue: data gradient
//       3 % slower; column patches laid out like the halo rows: no bank conflicts, 0.7-1.5 % slower
//       (profiles/r04_persistent_halo_gemm.txt items 1-5, 7, 8, 3; raw lines in profiles/r04_raw_ab_*.txt)
//   8-byte epilogue stores instead of 16-byte ones: 5-9 % slower (profiles/r04_ab_wide_stores_patch_rotation.txt)
//   XOR-keyed halo rows instead of rotated ones: 31-34 % LDS conflict replays (profiles/r03_ab_rotation_swizzle.txt)
//   streaming (nt) halo DMAs / addend loads: the step does not move (profiles/r04_nt_loads.txt)
//   SGPR-base and buffer-descriptor DMA addressing for every source: slower than per-lane addresses
//       (profiles/r03_ab_dma_addressing.txt; see the DMA addressing note in the kernel)
#define H3_PITCH 136                                   // halo row pitch in pixels (130 used; multiple of 8 = one DMA)
#define H3_HALO_BYTES (4 * H3_PITCH * 128)
#define H3_PATCH_ROWS 40                               // 2 tile rows x 2 sides x 9 taps = 36, rounded to whole DMAs
#define H3_LDS (H3_HALO_BYTES + 2 * 256 * 128)
#define H3_LDS_FOLD (H3_LDS + 2 * H3_PATCH_ROWS * 128)

// FOLD = data gradient of a REFLECT-padded conv (MirrorPadGrad folded into the gather, module.py:209-216 backward).
// With pad 1 the mirrored terms reach image rows 1 and H-2 and columns 1 and W-2 only:
//   rows   : output row 1 needs (dy[2] + dy[0]) where it would read dy[2], and only that row of the top tile reads
//            that halo slot (same for dy[H-3] + dy[H-1] in the bottom tile), so the slot is filled from a
//            pre-summed "virtual row" (a.fold, second part) -- no change to the fragment reads;
//   columns: the two pixels per tile row in columns 1 / W-2 read their gather row per tap from a small LDS patch
//            (2 x 2 x 9 rows per chunk, from a.fold's first part, which holds the complete mirrored sums for those
//            pixels) through a per-lane address select in the first / last pixel fragment.
// PAIR: two networks of one shape on a stacked batch, images >= a.nsplit take the second weight set (a compile-time flag so
// that the launches of the paired cycle step show under their own name in a kernel trace: they cover twice the images)
// NORM (forward only): the source is the RAW output of the previous conv and the instance norm + ReLU between the two convs
// (module.py:212-214) is applied to the halo rows after they land in LDS -- by the four waves that issue no DMAs, after their
// MFMAs of the step after the row's DMA, one step before its first use -- so the separate apply pass over the tensor (a read
// and a write of every activation) disappears; the normalised interior rows are written to a.nout from the same registers (the
// weight gradient of this conv reads them in the backward pass), a store stream that runs under the MFMAs.  Same arithmetic
// as in_apply_kernel (x * A + B, max 0, RNE to bf16): the results are bit-identical to the two separate calls.
// SRC: how the source tensor is padded -- 0 zeros (every data gradient; the zero-padded forward), 1 REFLECT (forward),
// 2 REFLECT + normalise on load.  A template parameter because the two paddings address their halo DMAs differently (below).
template <int MODE, bool FOLD, int STATS = 0, bool PAIR = false, int SRC = 0>   // STATS: 0 none, 1 forward norm sums, 2 backward norm sums
__global__ __launch_bounds__(512) void conv3x3_halo_gemm_kernel(ConvArgs a) {
    constexpr bool NORM = SRC == 2;
    static_assert(SRC == 0 || (MODE == MODE_FWD && !FOLD), "REFLECT sources / normalise-on-load exist for the forward conv only");
    constexpr int BN = 256, WGM = 2, WGN = 4, WM = 128, WN = 64, MI = 8, NI = 4, BKB = 128, KK = 2;
    constexpr int QA = 4;                              // weight rows per thread per tile (8 waves x 8 rows x 4)
    constexpr int RPP = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sH = smem;                                   // halo [4][H3_PITCH][128 B]
    char* sB = smem + H3_HALO_BYTES;                   // 2 x [256][128 B]
    char* sPatch = smem + H3_LDS;                      // FOLD: 2 x [H3_PATCH_ROWS][128 B]
    typedef __attribute__((address_space(3))) char lds_char;   // DMA destinations as LDS-space pointers from the start
    lds_char* const lH = (lds_char*)smem;
    lds_char* const lB = lH + H3_HALO_BYTES;
    lds_char* const lPatch = lH + H3_LDS;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int wm = wave / WGN, wn = wave % WGN;
    const int SC = (MODE == MODE_FWD) ? a.C : a.K;     // source channels (GEMM K per tap)
    const int DC = (MODE == MODE_FWD) ? a.K : a.C;
    const int wrow = 9 * SC;
    const int nchunk = SC >> 6;

    const int tilesN = (DC + BN - 1) / BN;
    const int tilesW = a.W / H3_TW, tilesH = a.H >> 1;
    int lid;
    {
        const int b = (int)blockIdx.x, nm = (int)gridDim.x;
        const int q = nm >> 3, rr = nm & 7, xcd = b & 7;
        lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
    }
    struct Tile { int n0, img, h0, w0, tw, th; const char* wmat_n; bool hasL, hasR; };
    auto tile_of = [&](int id) {
        Tile c;
        c.n0 = (id % tilesN) * BN;
        int mt = id / tilesN;
        c.tw = mt % tilesW; mt /= tilesW;
        c.th = mt % tilesH;
        c.img = mt / tilesH;
        c.h0 = c.th * 2; c.w0 = c.tw * H3_TW;
        c.wmat_n = PAIR && c.img >= a.nsplit ? a.wmat2 : a.wmat;
        c.hasL = FOLD && c.tw == 0; c.hasR = FOLD && c.tw == tilesW - 1;
        return c;
    };
    const int tpb = 1;
    bool primed = false;
  for (int it = 0; it < tpb; ++it) {
    const Tile cur = tile_of(lid);
    const int n0 = cur.n0, tw = cur.tw, th = cur.th, img = cur.img, h0 = cur.h0, w0 = cur.w0;
    const char* const wmat_n = cur.wmat_n;
    const bool dbg_clk = SGG_ABLATE_OF(a) == 9 && lid == 0 && tid == 0;
    const int abl = SGG_ABLATE_OF(a) >= 8 ? 0 : SGG_ABLATE_OF(a);    // 8, 9 = full kernel + clock stamps
    H3_CLOCKS(0);

    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    // ---- halo DMA: one wave-instruction = 8 halo pixels x 128 B; a halo row is 17 of them (wave, wave+8, wave+16)
    const int hpos = lane & 7, hsub = lane >> 3;
    constexpr bool mirror = SRC != 0;                                      // (the data gradient always zero-pads dy)
    // DMA addressing: a 64-bit address per lane and piece, zero-padded sources selecting against the zero page.  It costs ~12
    // instructions per piece and parks lane masks in VGPR lanes, and still measured FASTEST in the step: an LDS-DMA piece costs
    // the issuing wave 60-180 cycles whatever surrounds it, so the arithmetic runs in time the wave would wait anyway, and the
    // denser issue of the cheaper forms (uniform SGPR base + 32-bit lane offset; buffer descriptors) only bunches the LDS
    // writes against the other waves' fragment reads (profiles/r03_ab_dma_addressing.txt).  Only the normalise-on-load variant
    // takes the SGPR-base form (SADDR): it needs the ~16 registers.  (What did pay is the padding mode as a template parameter.)
    constexpr bool SADDR = SRC == 2;
    const char* vrows = FOLD ? a.fold + (size_t)a.N * a.H * 18 * SC * 2 : nullptr;   // [N][2][W][SC] after the patches
    // (Walking the channel chunks in a per-block rotated order -- so that the blocks of one XCD do not all want the
    // same weight tile at the same moment -- measured 1-2 % slower: first-touch L2 misses are not what the tiles wait for.)
    // (vw, nw): this wave acts as issuer vw of nw -- all 8 waves in the prologue, 4 issuer waves in the main loop
    // (ln: the lane id the per-lane parts of the addresses are derived from -- `lane` in the main loop, where they are loop
    // invariants hipcc keeps in registers; an OPAQUE copy for the prologues, whose lane masks and offsets would otherwise be
    // hoisted out of the persistent tile loop and stay live -- as spilled SGPRs -- across every main loop)
    auto load_halo_row = [&](const Tile& c, int k, int chunk, int vw, int nw, int ln) {
        const int hpos = ln & 7, hsub = ln >> 3;
        const int h0 = c.h0, w0 = c.w0, img = c.img;          // (the tile being LOADED: the next one under an epilogue)
        int hi = h0 - 1 + k;
        bool rowok = true;
        if (mirror) hi = hi < 0 ? -hi : (hi >= a.H ? 2 * (a.H - 1) - hi : hi);
        else rowok = (unsigned)hi < (unsigned)a.H;
        const char* rowp = a.src + ((size_t)img * a.H + (rowok ? hi : 0)) * a.W * SC * 2 + chunk * 128;
        if (FOLD) {
            if (h0 == 0 && k == 3) rowp = vrows + ((size_t)img * 2 + 0) * a.W * SC * 2 + chunk * 128;
            if (h0 == a.H - 2 && k == 0) rowp = vrows + ((size_t)img * 2 + 1) * a.W * SC * 2 + chunk * 128;
        }
#pragma unroll
        for (int qi = 0; qi < 5; ++qi) {
            const int q = vw + nw * qi;
            if (q >= 17) break;
            const int hp = q * 8 + hsub;                                   // halo column 0..135
            int wi = w0 - 1 + hp;
            bool ok = rowok && hp < H3_TW + 2;
            if (mirror) wi = wi < 0 ? -wi : (wi >= a.W ? 2 * (a.W - 1) - wi : wi);
            else ok = ok && (unsigned)wi < (unsigned)a.W;
            // Swizzle of the halo image.  A ds_read_b128 is serviced in four groups of 16 lanes that pair k-quarter fq = 0 (2) of
            // eight fragment rows with fq = 1 (3) of the other eight; per half bank line (row parity) a group therefore reads
            // chunk c of rows 2(m0 + {0,1,6,7}) and chunk c + 1 of rows 2(m0 + {2,3,4,5}), where m0 moves with the tap column
            // (fragment base = halo column + 0 / 1 / 2).  With the XOR key (r >> 1) & 7 those eight positions are distinct only
            // for even m0 -- the 31-34 % conflict replays of round 2 (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE) on two tap columns
            // of three.  Rotating instead, position = (c + 2 * (r >> 1)) & 7, gives 2 m0 + {0,2,4,6} and 2 m0 + 1 + {4,6,0,2}:
            // all evens and all odds, distinct for EVERY m0 (profiles/r03_ab_rotation_swizzle.txt).  The DMA writes LDS linearly,
            // so the rotation goes on the source address: position hpos of row r holds chunk (hpos - (r & 6)) & 7.
            const int hrow_ = k * H3_PITCH + hp;
            const int schunk = (hpos - (hrow_ & 6)) & 7;
            __attribute__((address_space(3))) void* const ldst = (__attribute__((address_space(3))) void*)(lH + (k * H3_PITCH + q * 8) * 128);
            if (SADDR) {
                // (REFLECT: every halo pixel is an image pixel -- the six filler columns read mirrored pixels nobody uses)
                dma16_to_lds_s(rowp, (uint32_t)(wi * SC * 2 + (schunk << 4)), ldst);
            } else {
                const char* src = ok ? rowp + (size_t)wi * SC * 2 + (schunk << 4) : zero;
                dma16_to_lds(src, ldst);
            }
        }
    };

    // ---- FOLD: column patch, row pe = (tile row * 2 + side) * 9 + tap (halo tap order), 5 DMAs by waves 0..4
    const bool hasL = cur.hasL, hasR = cur.hasR;
    auto load_patch = [&](const Tile& c, int chunk, int vw, int nw, int ln) {
        if (!FOLD) return;
        const int hpos = ln & 7, hsub = ln >> 3;
        const int h0 = c.h0, img = c.img;
        const bool hasL = c.hasL, hasR = c.hasR;
#pragma unroll
        for (int qi = 0; qi < 2; ++qi) {
            const int pw = vw + nw * qi;                                   // patch DMA 0..4
            if (pw >= H3_PATCH_ROWS / 8) break;
            const int pe = pw * 8 + hsub;
            // (XOR-keyed rows: 13 % of the data gradient's LDS cycles are conflict replays where a patch lane replaces a halo lane;
            // rows laid out like the halo's removed them and measured 0.7-1.5 % slower, profiles/r04_persistent_halo_gemm.txt item 3)
            const int tap_h = pe % 9, side = (pe / 9) & 1, tr = pe / 18;
            const int schunk = hpos ^ ((pe >> 1) & 7);
            const bool ok = pe < 36 && (side ? hasR : hasL);
            // a.fold first part: [N][H][2 sides][9 weight taps][SC]; halo tap t pairs with weight tap 8 - t
            const char* src = ok ? a.fold + (((((size_t)img * a.H + h0 + tr) * 2 + side) * 9 + (8 - tap_h)) * SC + chunk * 64) * 2 + (schunk << 4)
                                 : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(lPatch + ((chunk & 1) * H3_PATCH_ROWS + pw * 8) * 128));
        }
    };

    // ---- weight-tile DMA: 32 wave-instructions of 8 rows x 128 B per tile; instruction d covers rows 8d .. 8d+7, lane l row
    // 8d + l/8 at chunk position l%8 (swizzled by the row: key = (l/16 + 4(d&1)) & 7, i.e. the d-even key with bit 2 flipped)
    // One per-lane offset for the whole kernel (row within the 8-row group and the swizzled chunk; d & 1 == vw & 1 because nw is
    // even); DC is a multiple of 8, so an 8-row group is inside the matrix or outside it as a whole: a scalar test.
    const int wl = lane >> 3;
    const int wsw = ((lane & 7) ^ ((lane >> 4) & 7)) << 4;
    const uint32_t wvoff0 = (uint32_t)(wl * wrow * 2 + wsw), wvoff1 = (uint32_t)(wl * wrow * 2 + (wsw ^ 64));
    auto load_w = [&](const Tile& c, int stg, int chunk, int tap, int vw, int nw, int ln) {
        const int wl = ln >> 3;
        const int wsw = ((ln & 7) ^ ((ln >> 4) & 7)) << 4;
        const uint32_t wvoff0 = (uint32_t)(wl * wrow * 2 + wsw), wvoff1 = (uint32_t)(wl * wrow * 2 + (wsw ^ 64));
        const int n0 = c.n0;
        const char* const wmat_n = c.wmat_n;
        const char* const tbase = wmat_n + ((size_t)n0 * wrow + tap * SC + chunk * 64) * 2;
        const uint32_t wvoff = (vw & 1) ? wvoff1 : wvoff0;
        lds_char* sQ = lB + stg * (256 * 128);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = vw + nw * j;
            if (d >= 32) break;
            __attribute__((address_space(3))) void* const ldst = (__attribute__((address_space(3))) void*)(sQ + d * 8 * 128);
            if (!SADDR) {
                const bool ok = n0 + d * 8 + wl < DC;
                const char* src = ok ? wmat_n + (size_t)(n0 + wl) * wrow * 2 + d * ((size_t)8 * wrow * 2) + (tap * SC + chunk * 64) * 2 + (wsw ^ ((d & 1) << 6)) : zero;
                dma16_to_lds(src, ldst);
            } else if (n0 + d * 8 < DC) dma16_to_lds_s(tbase + (size_t)d * 8 * wrow * 2, wvoff, ldst);
            else dma16_to_lds(zero, ldst);
        }
    };

    // ---- NORM: halo row k (just landed, chunk `chunk` of the source channels) -> relu(x * A + B) in place.  A lane owns ONE
    // 16-byte channel group (8 channels: its A / B stay in registers for the row) and walks the row's pixels, 8 per wave pass;
    // rows 1 and 2 are this tile's own image rows: their 128 interior pixels also go to a.nout (whole 128-byte lines).
    float* const sNA = reinterpret_cast<float*>(smem + (FOLD ? H3_LDS_FOLD : H3_LDS));   // A[SC], then B[SC]
    auto norm_row = [&](int k_, int chunk, int vw, int nw) {
        if constexpr (NORM) {
            // (k through an opaque asm: the row's LDS / global addresses are loop invariants otherwise, and hipcc keeps all of
            // them -- four rows x five pieces -- live across the main loop, next to 128 accumulators: scratch spills)
            int k = k_;
            asm volatile("" : "+s"(k));
            const int c8 = lane & 7;
            float A[8], B[8];
            {
                const float* pa = sNA + chunk * 64 + c8 * 8;
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(pa), a1 = *reinterpret_cast<const f32x4*>(pa + 4);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(pa + SC), b1 = *reinterpret_cast<const f32x4*>(pa + SC + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { A[e] = a0[e]; A[4 + e] = a1[e]; B[e] = b0[e]; B[4 + e] = b1[e]; }
            }
            const bool own_row = k == 1 || k == 2;
            char* const orow = a.nout + ((((size_t)img * a.H + h0 + k - 1) * a.W + w0) * SC + chunk * 64 + c8 * 8) * 2;
            auto piece_ptr = [&](int q) -> char* {
                const int hrow_ = k * H3_PITCH + q * 8 + hsub;
                const int pos = (c8 + (hrow_ & 6)) & 7;
                return sH + hrow_ * 128 + (pos << 4);
            };
            // up to five pieces per lane and row (17 pixel groups over 4 waves), in batches of <= 3 with the batch's reads issued
            // together: one LDS latency per batch, and no more than 12 staging registers (the accumulators leave little room)
#pragma unroll
            for (int b0 = 0; b0 < 5; b0 += 3) {
                u32x4 v[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int q = vw + nw * (b0 + u);
                    if (b0 + u < 5 && q < 17) v[u] = ld16(piece_ptr(q));
                }
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int q = vw + nw * (b0 + u);
                    if (b0 + u >= 5 || q >= 17) continue;
                    const int hp = q * 8 + hsub;
                    float xv[8], o[8];
                    ET<bf16>::unpack(v[u], xv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float t = xv[e] * A[e] + B[e]; o[e] = t > 0.f ? t : 0.f; }
                    const u32x4 pk = ET<bf16>::pack(o);
                    st16(piece_ptr(q), pk);
                    if (own_row && hp >= 1 && hp <= H3_TW) st16(orow + (size_t)(hp - 1) * SC * 2, pk);
                }
            }
        }
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    const int fswQ = ((wn * WN + frow) >> 1) & 7;

    if constexpr (NORM) {                                  // the norm's affine form per source channel of this image
        const float* const gm = PAIR && img >= a.nsplit ? a.ngamma2 : a.ngamma;
        const float* const bt = PAIR && img >= a.nsplit ? a.nbeta2 : a.nbeta;
        for (int c = tid; c < SC; c += 512) {
            const float mu = a.nstats[((size_t)img * SC + c) * 2], rs = a.nstats[((size_t)img * SC + c) * 2 + 1];
            const float A = gm[c] * rs;
            sNA[c] = A;
            sNA[SC + c] = bt[c] - mu * A;
        }
    }
    // prologue: whole halo of chunk 0 + weight tile 0
    if (!primed) {
        int lop = lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) load_halo_row(cur, k, 0, wave, 8, lop);
        load_patch(cur, 0, wave, 8, lop);
        load_w(cur, 0, 0, MODE == MODE_FWD ? 0 : 8, wave, 8, lop);
    }
    SGG_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    if constexpr (NORM) {
        // the tile's own rows (1, 2: stored to a.nout) by the waves that issue no DMAs in the main loop, the neighbours' rows by
        // the DMA issuers: those wait for vmcnt(0) at the end of every step and would sit out the stores' round trip to memory
        // there (with the rows dealt to all eight waves the prologue cost 4.7 us per tile)
        if ((wave >> 2) != H3_HALO_HALF) { norm_row(1, 0, wave & 3, 4); norm_row(2, 0, wave & 3, 4); }
        else { norm_row(0, 0, wave & 3, 4); norm_row(3, 0, wave & 3, 4); }
        SGG_WAIT_LGKM0();
        __builtin_amdgcn_s_barrier();
    }

    const int ntiles = abl >= 5 ? 0 : nchunk * 9;
    int chunk = 0, tap = 0;                           // of the tile being multiplied
#ifdef SGG_LAB
    const bool stamp = SGG_ABLATE_OF(a) == 8 && lid == 0 && lane == 0;
#define H3_STAMP(pt) do { if (stamp && t >= 8 && t < 24) g_dbg_phase[wave][t - 8][pt] = clock64(); } while (0)
#else
#define H3_STAMP(pt) do {} while (0)
#endif
    auto main_loop = [&]() {
        auto issue_halo = [&](int vw) -> int {            // returns the number of halo rows issued this tile (0 .. 2); row 0 brings the patch
            int rows = 0;
            if (tap == 0 && chunk > 0) { load_halo_row(cur, 2, chunk, vw, 4, lane); ++rows; }
            if (tap == 3) {
                if (chunk > 0) { load_halo_row(cur, 3, chunk, vw, 4, lane); ++rows; }
                if (chunk + 1 < nchunk) { load_halo_row(cur, 0, chunk + 1, vw, 4, lane); load_patch(cur, chunk + 1, vw, 4, lane); ++rows; }
            }
            if (tap == 6 && chunk + 1 < nchunk) { load_halo_row(cur, 1, chunk + 1, vw, 4, lane); ++rows; }
            return rows;
        };
        for (int t = 0; t < ntiles; ++t) {
            H3_STAMP(0);
            // refill: next weight tile, and the halo rows whose slots are free (see header).  ISSUER WAVES: the CU's vector-memory
            // path takes ~16 cycles per 1 KB DMA instruction, so the ~40 of a tile keep it busy for ~640 cycles; with every wave
            // issuing its share at the head of the tile, all eight sat in issue stalls for that long with the matrix pipes idle
            // (tools/halo_phases.py).  Now waves 4-7 issue ALL the DMAs while waves 0-3 -- their SIMD partners -- go straight to
            // their MFMAs.  (Not the same as splitting each wave's issue in time: waves 4-7 issuing their own share half way
            // through the tile measured 7 % slower; waves 0-3 issuing the halo rows, or 2-4 of the 8 weight DMAs per SIMD pair,
            // AFTER their MFMAs -- in the ~1 000 cycles they wait at the barrier -- measured 2-3 % slower, and so did the same with
            // the wait for them relaxed to one tile later; the issuers' first fragment reads put ahead of their DMA issue cost the
            // data gradient 3 %: profiles/r04_persistent_halo_gemm.txt items 7 and 8.)
            if (abl == 0 || abl == 2) {
                const int vw = wave & 3;
                if ((wave >> 2) == H3_ISSUER_HALF) {           // the weight tile: 8 DMA instructions per issuer wave and tile
                    int ntap = tap + 1, nchk = chunk;
                    if (ntap == 9) { ntap = 0; ++nchk; }
                    if (t + 1 < ntiles) load_w(cur, (t + 1) & 1, nchk, MODE == MODE_FWD ? ntap : 8 - ntap, vw, 4, lane);
                }
                if ((wave >> 2) == H3_HALO_HALF) issue_halo(vw);   // the halo rows (17 instructions each, ~1 row per tile on average)
            }
            H3_STAMP(1);
            const int r = tap / 3, sx = tap - 3 * r;
            // halo offset (r, sx) pairs with weight tap (r, sx) forward and with the flipped tap (2-r, 2-sx) = 8 - tap in
            // the data gradient, so both modes walk the halo rows in the same order (the refill schedule relies on it)
            const int hr = wm + r;                                             // halo row of this wave's output row
            const int hc = frow + sx;                                          // halo column of fragment 0
            const int fswP = (hr * H3_PITCH + hc) & 6;                         // same for every fragment (16 | fragment step)
            const char* bP = sH + (hr * H3_PITCH + hc) * 128;
            const char* bQ = sB + (t & 1) * (256 * 128) + (wn * WN + frow) * 128;
            // FOLD: the lanes holding pixel column 1 (fragment 0) / W-2 (fragment MI-1) read their patch row instead
            const int peL = (wm * 2 + 0) * 9 + tap;
            const int peR = (wm * 2 + 1) * 9 + tap;
            const char* pL = sPatch + ((chunk & 1) * H3_PATCH_ROWS + peL) * 128;
            const char* pR = sPatch + ((chunk & 1) * H3_PATCH_ROWS + peR) * 128;
            const int keyL = (peL >> 1) & 7, keyR = (peR >> 1) & 7;
            const bool isL = hasL && frow == 1, isR = hasR && frow == 14;
            auto ldP = [&](int j, int kk) -> u32x4 {
                const char* p = bP + j * 16 * BKB + (((fq + 4 * kk + fswP) & 7) << 4);
                if (FOLD) {
                    if (j == 0 && isL) p = pL + (((fq + 4 * kk) ^ keyL) << 4);
                    if (j == MI - 1 && isR) p = pR + (((fq + 4 * kk) ^ keyR) << 4);
                }
                return ld16(p);
            };
            if (abl != 2) {
                // Fragment pipeline: the reads are issued in the order the MFMA groups consume them -- k-step 0's weight fragments and the
                // first GJ pixel fragments, then (while group 0 multiplies) the next pixel group and k-step 1's weight fragments -- so the
                // first MFMA waits for 4 + GJ reads, not for the whole burst, and every later group finds its fragments landed.
                // (This needs hipcc to COUNT its waits, which it only does with the DMA and the waits in the forms above.)
                constexpr int GJ = H3_GJ, GPK = MI / GJ, NG = KK * GPK;
                u32x4 fw[KK][NI];
    #pragma unroll
                for (int i = 0; i < NI; ++i) fw[0][i] = ld16(bQ + i * 16 * BKB + (((fq + 0) ^ fswQ) << 4));
                u32x4 fp[2][GJ];
    #pragma unroll
                for (int jj = 0; jj < GJ; ++jj) fp[0][jj] = ldP(jj, 0);
    #pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const int kk = g / GPK, jb = (g % GPK) * GJ;
                    if (g + 1 < NG) {
                        const int kn = (g + 1) / GPK, jn = ((g + 1) % GPK) * GJ;
    #pragma unroll
                        for (int jj = 0; jj < GJ; ++jj) fp[(g + 1) & 1][jj] = ldP(jn + jj, kn);
                    }
                    if (g == 0) {
    #pragma unroll
                        for (int i = 0; i < NI; ++i) fw[1][i] = ld16(bQ + i * 16 * BKB + (((fq + 4) ^ fswQ) << 4));
                    }
                    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                    for (int jj = 0; jj < GJ; ++jj)
    #pragma unroll
                        for (int i = 0; i < NI; ++i)
                            acc[i][jb + jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                __builtin_bit_cast(bf16x8, fw[kk][i]), __builtin_bit_cast(bf16x8, fp[g & 1][jj]), acc[i][jb + jj], 0, 0, 0);
                    if constexpr (NORM) {
                        // Rows land one step after their DMA was issued (the barrier below) and are first read two or more steps later
                        // (see the refill schedule above): the step in between is where they are normalised, by the waves without
                        // DMAs.  WHERE in the step: those waves have the matrix pipe to themselves while their SIMD partners issue the
                        // DMAs (about half of the step's 64 MFMAs), then share it.  The ~1 300 cycles of VALU / LDS work of a row go
                        // in the MIDDLE -- the partner wave, on the critical path, takes the whole pipe meanwhile; after the last
                        // MFMA the same work measured fully exposed (paired launch +20 us).
                        if (g == H3_NORM_AT && (wave >> 2) != H3_HALO_HALF) {
                            __builtin_amdgcn_sched_barrier(0);
                            const int vw = wave & 3;
                            if (tap == 1 && chunk > 0) norm_row(2, chunk, vw, 4);
                            if (tap == 4 && chunk > 0) norm_row(3, chunk, vw, 4);
                            if (tap == 5 && chunk + 1 < nchunk) norm_row(0, chunk + 1, vw, 4);
                            if (tap == 7 && chunk + 1 < nchunk) norm_row(1, chunk + 1, vw, 4);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
            }
            H3_STAMP(2);
            if (!NORM || (wave >> 2) == H3_HALO_HALF || (wave >> 2) == H3_ISSUER_HALF) SGG_WAIT_VM0();   // (NORM: the other waves only have stores in flight)
            H3_STAMP(3);
            SGG_WAIT_LGKM0();
            H3_STAMP(4);
            if (abl < 3) __builtin_amdgcn_s_barrier();
            H3_STAMP(5);
            if (++tap == 9) { tap = 0; ++chunk; }
        }
    };
    main_loop();

    H3_CLOCKS(2);
    if (abl == 6) return;
    auto prime_next = [&]() { primed = false; };
    // Epilogue, one 16-channel group at a time.  STATS 1 (forward): per-channel (sum, sumsq) of the STORED output for the
    // instance norm that follows the conv.  STATS 2 (data gradient): the first pass of the instance-norm BACKWARD that
    // consumes this gradient, (sum g, sum g*xhat) with g = dx * act'(gamma*xhat + beta) and xhat from that norm's input
    // a.nx and statistics a.nstats (norm.hip in_partial_kernel<BWD>).  Each wave reduces its 128 pixels x 64 channels
    // (registers -> 16-lane butterfly, fixed order) and writes one row per channel as pixel chunk (tile, wave row) of the
    // image, so the norm skips its own statistics pass over the tensor.
    const size_t prow = ((size_t)img * a.H + h0 + wm) * a.W + w0;
    if constexpr (STATS != 2) {
        // pixel-major store order: the four 16-channel groups of a pixel go out back to back, so the 128 bytes a wave
        // writes per pixel merge into whole lines in L2 (channel-group-major order cost +47 MB of HBM fetches per launch:
        // partially written lines are read back)
        const float* const bias_n = PAIR && img >= a.nsplit ? a.bias2 : a.bias;   // (picked here, not before the loop: registers)
        float bv[NI][4], s1[NI][4], s2[NI][4];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int dc = n0 + wn * WN + i * 16 + fq * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) { bv[i][e] = (bias_n && dc < DC) ? bias_n[dc + e] : 0.f; s1[i][e] = s2[i][e] = 0.f; }
        }
        // PLAIN path (every call of the step: no activation, bf16 result, bf16 or no addend): the uniform conditions are tested
        // once, and the skip-gradient addend's 32 loads per lane are all issued before the first store -- the fragment registers
        // are dead here.  (With the tests inside the unrolled loops every load was followed by s_waitcnt vmcnt(0): 32 dependent
        // round trips at the tail of a grid that has nothing else to overlap them with.)
        const bool plain = a.act == SGG_ACT_NONE && !(MODE != MODE_FWD && (a.dst_f32 || a.addend_f32));
        if (plain) {
            // A lane holds 4 consecutive channels of one pixel per fragment: 8-byte stores, 32 per lane, and the tail of a grid
            // whose blocks all store at once is store-ISSUE bound.  Fragments 2 jp and 2 jp + 1 trade their halves between lane
            // rows (row_swap16) so that every lane owns 8 consecutive channels of ONE pixel -- lanes of rows 0 / 2 a pixel of the
            // even fragment, rows 1 / 3 one of the odd fragment: 16 stores of 16 bytes (and 16 addend loads instead of 32).  Same
            // values, same roundings, same statistics (taken before the exchange); pixel-major order as before.
            auto run = [&](auto has_add) {
                constexpr bool ADD = decltype(has_add)::value;
                const int jo = fq & 1, cb = (fq >> 1) * 8;
                const size_t e0 = (prow + jo * 16 + frow) * DC + n0 + wn * WN + cb;   // element (fragment pair 0, group 0) of this lane
                const size_t ej2 = (size_t)32 * DC;
                constexpr int NH = 1, JH = MI / 2 / NH;
                if constexpr (!ADD) prime_next();
#pragma unroll
                for (int hb = 0; hb < NH; ++hb) {
                    u32x4 adv[JH][NI];
                    if constexpr (ADD) {
#pragma unroll
                        for (int jq = 0; jq < JH; ++jq)
#pragma unroll
                            for (int i = 0; i < NI; ++i) {
                                adv[jq][i] = zero16();
                                if (n0 + wn * WN + i * 16 + cb < DC) {
                                    const bf16* ap = reinterpret_cast<const bf16*>(a.addend) + e0 + (hb * JH + jq) * ej2 + i * 16;
                                    adv[jq][i] = ld16(ap);
                                }
                            }
                        if (hb == 0) prime_next();
                    }
#pragma unroll
                    for (int jq = 0; jq < JH; ++jq) {
                        const int jp = hb * JH + jq;
#pragma unroll
                        for (int i = 0; i < NI; ++i) {
                            float v0[4], v1[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) { v0[e] = acc[i][2 * jp][e] + bv[i][e]; v1[e] = acc[i][2 * jp + 1][e] + bv[i][e]; }
                            u32x4 pk;
                            if constexpr (ADD) {
                                float ad[8], o[8];
                                ET<bf16>::unpack(adv[jq][i], ad);
#pragma unroll
                                for (int e = 0; e < 4; ++e) { row_swap16(v0[e], v1[e]); o[e] = v0[e] + ad[e]; o[4 + e] = v1[e] + ad[4 + e]; }
                                pk = ET<bf16>::pack(o);
                            } else {
                                const bf16x4 p0 = {(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3]}, p1 = {(bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
                                if (STATS == 1) {
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {           // (fragment order: 2 jp, then 2 jp + 1)
                                        const float r0 = (float)p0[e]; s1[i][e] += r0; s2[i][e] += r0 * r0;
                                    }
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        const float r1 = (float)p1[e]; s1[i][e] += r1; s2[i][e] += r1 * r1;
                                    }
                                }
                                const u32x2 q0 = __builtin_bit_cast(u32x2, p0), q1 = __builtin_bit_cast(u32x2, p1);
                                uint32_t a0 = q0[0], a1 = q0[1], b0 = q1[0], b1 = q1[1];
                                row_swap16(a0, b0); row_swap16(a1, b1);
                                pk = (u32x4){a0, a1, b0, b1};
                            }
                            if (n0 + wn * WN + i * 16 + cb < DC) st16(reinterpret_cast<bf16*>(a.dst) + e0 + jp * ej2 + i * 16, pk);
                        }
                    }
                }
            };
            if (MODE != MODE_FWD && a.addend) run(std::true_type{}); else run(std::false_type{});
        } else {
            prime_next();
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                const size_t dpix = prow + j * 16 + frow;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int dc = n0 + wn * WN + i * 16 + fq * 4;
                    if (dc >= DC) continue;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_apply(acc[i][j][e] + bv[i][e], a.act, a.leak);
                    if (a.addend) {
                        if (MODE != MODE_FWD && a.addend_f32) {
                            const f32x4 ad = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.addend) + dpix * DC + dc);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += ad[e];
                        } else {
                            const bf16* ad = reinterpret_cast<const bf16*>(a.addend) + dpix * DC + dc;
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += (float)ad[e];
                        }
                    }
                    if (MODE != MODE_FWD && a.dst_f32) {      // mixed mode: the data gradient stays f32 on its way to the next norm backward
                        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.dst) + dpix * DC + dc) = (f32x4){v[0], v[1], v[2], v[3]};
                        continue;
                    }
                    bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                    *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(a.dst) + dpix * DC + dc) = pk;
                    if (STATS == 1) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float vr = (float)pk[e]; s1[i][e] += vr; s2[i][e] += vr * vr; }
                    }
                }
            }
        }
        if (STATS == 1) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) {
                        s1[i][e] += __shfl_xor(s1[i][e], off);
                        s2[i][e] += __shfl_xor(s2[i][e], off);
                    }
                }
            if (frow == 0) {
                const int chunks = tilesH * tilesW * 2;
                const int chunk = (th * tilesW + tw) * 2 + wm;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int dc = n0 + wn * WN + i * 16 + fq * 4;
                    if (dc >= DC) continue;
                    float* o = a.stats + (((size_t)img * chunks + chunk) * DC + dc) * 2;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { o[2 * e] = s1[i][e]; o[2 * e + 1] = s2[i][e]; }
                }
            }
        }
    }
    // STATS 2 (data gradient; no bias, no activation -- the entry point passes none).  The norm's input tile (2 rows x 128 pixels x 256
    // channels = 128 KB) is first DMA'd into LDS -- the halo and the weight stages are free now -- with coalesced 16-byte
    // pieces, and each lane then picks its 8-byte (pixel, 4 channels) groups out of LDS: 512-byte pixel rows, 16-byte chunk c
    // of pixel p at position c ^ (p & 31), so the 16 pixels a ds_read_b64 touches hit 16 different chunks.
    // Per lane and channel only two constants stay in registers, the norm's affine form A = gamma*rstd, B = beta - mean*A
    // (the sign of A*x + B is the activation mask, as in in_apply_kernel); the sums are (sum g, sum g*x) and the chunk's
    // second sum is recovered at the end as rstd * (sum g*x - mean * sum g).  Pixel-major store order as above; two pixels'
    // addend loads and LDS reads are in flight at a time.
    if constexpr (STATS == 2) {
        for (int id = wave; id < 128; id += 8) {         // 128 wave-instructions of 2 pixels x 512 B
            const int p = id * 2 + (lane >> 5), pos = lane & 31;
            const int chunk = pos ^ (p & 31);
            const bool ok = n0 + chunk * 8 < DC;
            const char* src = ok ? a.nx + ((((size_t)img * a.H + h0 + (p >> 7)) * a.W + w0 + (p & 127)) * DC + n0 + chunk * 8) * 2 : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(lH + id * 1024));
        }
        float cA[NI][4], cB[NI][4], s1[NI][4], s2[NI][4];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int dc = n0 + wn * WN + i * 16 + fq * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cA[i][e] = cB[i][e] = s1[i][e] = s2[i][e] = 0.f;
                if (dc < DC) {
                    const float mu = a.nstats[((size_t)img * DC + dc + e) * 2], rs = a.nstats[((size_t)img * DC + dc + e) * 2 + 1];
                    cA[i][e] = a.ngamma[dc + e] * rs;
                    cB[i][e] = a.nbeta[dc + e] - mu * cA[i][e];
                }
            }
        }
        SGG_WAIT_VM0();
        __builtin_amdgcn_s_barrier();
        const size_t e0 = (prow + frow) * DC + n0 + wn * WN + fq * 4;
        const size_t ej = (size_t)16 * DC;
        act_dispatch(a.nact, [&](auto nact_c) {
            constexpr int NACT = decltype(nact_c)::value;
            auto run = [&](auto has_add) {
                constexpr bool ADD = decltype(has_add)::value;
#pragma unroll
                for (int j0 = 0; j0 < MI; j0 += 2) {
                    bf16x4 adv[2][NI], xq[2][NI];
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int i = 0; i < NI; ++i) {
                            const int j = j0 + jj, dc = n0 + wn * WN + i * 16 + fq * 4;
                            const int pl = wm * 128 + j * 16 + frow, cl = wn * WN + i * 16 + fq * 4;      // tile pixel, tile channel
                            xq[jj][i] = *reinterpret_cast<const bf16x4*>(smem + (size_t)pl * 512 + (((cl >> 3) ^ (pl & 31)) << 4) + (cl & 7) * 2);
                            if constexpr (ADD) {
                                adv[jj][i] = (bf16x4){(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
                                if (dc < DC) adv[jj][i] = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const bf16*>(a.addend) + e0 + j * ej + i * 16);
                            }
                        }
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int i = 0; i < NI; ++i) {
                            const int j = j0 + jj, dc = n0 + wn * WN + i * 16 + fq * 4;
                            if (dc >= DC) continue;
                            float v[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e];
                            if constexpr (ADD) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] += (float)adv[jj][i][e];
                            }
                            bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                            *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(a.dst) + e0 + j * ej + i * 16) = pk;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float xv = (float)xq[jj][i][e];
                                const float g = (float)pk[e] * act_grad_c<NACT>(cA[i][e] * xv + cB[i][e], a.nleak);
                                s1[i][e] += g; s2[i][e] += g * xv;
                            }
                        }
                }
            };
            if (a.addend) run(std::true_type{}); else run(std::false_type{});
        });
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    s1[i][e] += __shfl_xor(s1[i][e], off);
                    s2[i][e] += __shfl_xor(s2[i][e], off);
                }
            }
        if (frow == 0) {
            const int chunks = tilesH * tilesW * 2;
            const int chunk = (th * tilesW + tw) * 2 + wm;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int dc = n0 + wn * WN + i * 16 + fq * 4;
                if (dc >= DC) continue;
                float* o = a.stats + (((size_t)img * chunks + chunk) * DC + dc) * 2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float mu = a.nstats[((size_t)img * DC + dc + e) * 2], rs = a.nstats[((size_t)img * DC + dc + e) * 2 + 1];
                    o[2 * e] = s1[i][e]; o[2 * e + 1] = rs * (s2[i][e] - mu * s1[i][e]);
                }
            }
        }
    }
  }   // tile loop
}

// shapes the halo-resident kernel takes: 3x3, stride 1, pad 1 on a same-size output, bf16, 64 | source channels,
// 128 | W, even H; REFLECT only forward (the REFLECT data gradient needs the mirrored border terms)
// (a question about the shape alone: plan_conv never splits K for a shape this kernel takes)
bool halo3_ok(const sgg_conv_desc* d, int mode) {
    const int en = sgg_config().halo3;
    if (!en || d->dtype != SGG_BF16) return false;
    if (d->R != 3 || d->S != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 || d->Ho != d->H || d->Wo != d->W) return false;
    if (d->W % H3_TW || (d->H & 1) || d->H < 4) return false;
    const int SC = mode == MODE_FWD ? d->C : d->K;
    if (SC % 64) return false;
    // one image of the source and one tile's weight rows below 1 GiB.  The bound dates from a DMA addressing form that is gone
    // (the kernel's addresses are 64-bit); it stays because it decides which kernel a shape is dispatched to
    constexpr int64_t kMaxBytes = (int64_t)1 << 30;
    if ((int64_t)d->H * d->W * SC * 2 >= kMaxBytes || (int64_t)256 * 9 * SC * 2 >= kMaxBytes) return false;
    return mode == MODE_FWD || mode == MODE_DGRAD;
}

#define H3_NORM_MAXC 512                               // NORM: the A / B table behind the tiles holds this many source channels
template <int MODE, bool FOLD, int STATS = 0, bool PAIR = false, int SRC = 0>
static int launch_halo3_t(const ConvArgs& a, hipStream_t s) {
    auto kern = conv3x3_halo_gemm_kernel<MODE, FOLD, STATS, PAIR, SRC>;
    constexpr int lds = (FOLD ? H3_LDS_FOLD : H3_LDS) + (SRC == 2 ? H3_NORM_MAXC * 8 : 0);
    SGG_LDS_ATTR(kern, lds);
    const int DC = MODE == MODE_FWD ? a.K : a.C;
    int64_t blocks = (int64_t)a.N * (a.H / 2) * (a.W / H3_TW) * ((DC + 255) / 256);
    sgg_launch_timed(kern, dim3((unsigned)blocks), dim3(512), (unsigned)lds, s, a);
    return sgg_check_launch();
}

// the kernel variant for these arguments: FOLD (REFLECT data gradient), STATS, PAIR (two weight sets) and SRC (padding / normalise on load)
int launch_halo3(const ConvArgs& a, int mode, hipStream_t s) {
    if (mode == MODE_DGRAD) {
        const bool pair = a.wmat2 != nullptr;
        if (a.stats && (pair || a.dst_f32 || a.addend_f32)) return SGG_EUNSUPPORTED;   // (the norm-backward sums have no paired / mixed form)
        if (a.reflect) {
            if (a.stats) return launch_halo3_t<MODE_DGRAD, true, 2>(a, s);
            return pair ? launch_halo3_t<MODE_DGRAD, true, 0, true>(a, s) : launch_halo3_t<MODE_DGRAD, true>(a, s);
        }
        if (a.stats) return launch_halo3_t<MODE_DGRAD, false, 2>(a, s);
        if (pair) return launch_halo3_t<MODE_DGRAD, false, 0, true>(a, s);
    }
    if (mode == MODE_FWD) {
        if (a.nout) {
            if (!a.stats || !a.reflect || a.C > H3_NORM_MAXC) return SGG_EUNSUPPORTED;
            return a.wmat2 ? launch_halo3_t<MODE_FWD, false, 1, true, 2>(a, s) : launch_halo3_t<MODE_FWD, false, 1, false, 2>(a, s);
        }
        if (a.reflect) {
            if (a.wmat2) return a.stats ? launch_halo3_t<MODE_FWD, false, 1, true, 1>(a, s) : launch_halo3_t<MODE_FWD, false, 0, true, 1>(a, s);
            return a.stats ? launch_halo3_t<MODE_FWD, false, 1, false, 1>(a, s) : launch_halo3_t<MODE_FWD, false, 0, false, 1>(a, s);
        }
        if (a.wmat2) return a.stats ? launch_halo3_t<MODE_FWD, false, 1, true>(a, s) : launch_halo3_t<MODE_FWD, false, 0, true>(a, s);
        if (a.stats) return launch_halo3_t<MODE_FWD, false, 1>(a, s);
    }
    if (mode == MODE_DGRAD) return launch_halo3_t<MODE_DGRAD, false>(a, s);
    return mode == MODE_FWD ? launch_halo3_t<MODE_FWD, false>(a, s) : SGG_EUNSUPPORTED;
}

size_t halo3_stats_chunks(const sgg_conv_desc* d) { return (size_t)(d->H / 2) * (d->W / H3_TW) * 2; }
int halo3_norm_maxc() { return H3_NORM_MAXC; }

#ifdef SGG_LAB
extern "C" {
// lab build only: the per-phase stamps of SGG_ABLATE=8 (768 values)
int sgg_debug_phases(unsigned long long* out768) {
    if (!out768) return SGG_EINVAL;
    return hipMemcpyFromSymbol(out768, HIP_SYMBOL(g_dbg_phase), sizeof(g_dbg_phase)) == hipSuccess ? SGG_OK : SGG_ELAUNCH;
}
// lab build only (not part of include/sggan.h): timestamps left by the halo GEMM under SGG_ABLATE=9 and the wall-clock rate (kHz)
int sgg_debug_clocks(unsigned long long* out5) {
    if (!out5) return SGG_EINVAL;
    if (hipMemcpyFromSymbol(out5, HIP_SYMBOL(g_dbg_clk), 4 * sizeof(unsigned long long)) != hipSuccess) return SGG_ELAUNCH;
    int khz = 0, dev = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    out5[4] = (unsigned long long)khz;
    return SGG_OK;
}
}
#endif
