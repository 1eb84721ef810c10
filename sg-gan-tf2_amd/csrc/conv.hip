// conv.hip -- implicit-GEMM convolution on gfx950 MFMA tiles.
//
// Replaces: tf.keras.layers.Conv2D / Conv2DTranspose and the
// tf.pad(...,"REFLECT") in front of them (module.py:210-216,230-264,284-311) and their
// gradients (gen_tape/disc_tape.gradient, model.py:196-197).
//
// The generic GEMM, conv_gemm_glds_kernel, in two modes; all NHWC with channels padded to 8 so every gather is a 16-byte chunk:
//   FWD    y[pixel][k]   = sum_{tap,c} x~[pixel,tap][c] * Wf[k][tap,c]       (gather over x)
//   DGRAD  dx[pixel][c]  = sum_{tap,k} dy[pixel,tap][k] * Wd[c][tap,k]       (transposed gather; the
//          stride-2 case is split into stride^2 output-parity classes so each block only visits the
//          taps that hit its pixels; REFLECT reads the border pixels' gather rows pre-folded from a side tensor)
// Conv2DTranspose forward IS the DGRAD GEMM of the equivalent conv (plus bias), its data gradient IS
// the FWD GEMM, its weight gradient IS the conv's with the operand roles swapped.
// Beside it: the kernels that keep a layer's halo in LDS (stride-2 3x3, the narrow 7x7 layers, D's first conv) and
// conv_border_fold_kernel, the small second launch that adds REFLECT's mirrored terms behind two of them.
//
// Tiles: LDS rows are 128-byte K-slices (64 bf16 / 32 f32) XOR-swizzled on the 16-byte
// chunk index so the ds_read_b128 fragment reads are bank-conflict free; MFMA 16x16x32 bf16 (or 16x16x4 f32 on
// the parity path, consuming the same 16-byte fragments with a k-permutation that A and B share).
// The weight fragment is the MFMA A operand and the pixel fragment the B operand, so the accumulator holds
// D[cout][pixel]: each lane owns 4 consecutive output channels of one pixel = one 8/16-byte NHWC store.
//
// The 3x3 stride-1 kernel with the input halo resident in LDS (the residual blocks' convs, the step's largest kernel family)
// is a translation unit of its own, conv_halo3.hip, and so are the weight gradients (kernels, plan and launch layer),
// conv_wgrad.hip; conv_internal.h holds what the three files share.  Every extern "C" entry point is here.
#include "conv_internal.h"

// Kernel-selection switches.  The shipped library always returns the defaults below and never reads the environment;
// only the lab build (-DSGG_LAB, `python sg-gan-tf2_amd/build.py --lab` -> libsggan_lab.so, used by tools/) lets
// SGG_* environment variables override them for A/B timing and ablation runs.
const SggConfig& sgg_config() {
#ifdef SGG_LAB
    static const SggConfig cfg = [] {
        SggConfig c;
        auto rd = [](const char* n, int dflt) { const char* e = getenv(n); return e ? atoi(e) : dflt; };
        c.halo3 = rd("SGG_HALO3", c.halo3);                       // 3x3 stride-1 convs through the LDS-resident halo GEMM
        c.s2halo = rd("SGG_S2HALO", c.s2halo);                    // stride-2 data gradient / transposed conv, all parity classes per block
        c.w9 = rd("SGG_W9", c.w9);                                // all-taps 3x3 weight gradient
        c.w9s2 = rd("SGG_W9S2", c.w9s2);                          // ... its stride-2 variant
        c.stem_dgrad_halo = rd("SGG_STEM_DGRAD_HALO", c.stem_dgrad_halo);
        c.n7 = rd("SGG_N7", c.n7);                                // 7x7 64<->3 layers: (channel, tap column) in the GEMM N dimension
        c.wgrad_rowfast = rd("SGG_WGRAD_ROWFAST", c.wgrad_rowfast);
        c.in_fused_maxhw = rd("SGG_IN_FUSED_MAXHW", c.in_fused_maxhw);
        c.ablate = rd("SGG_ABLATE", 0);                           // timing experiments: skips work, results are WRONG
        return c;
    }();
    return cfg;
#else
    static const SggConfig cfg;
    return cfg;
#endif
}

template <typename T>
__device__ inline u32x4 chunk_add(const u32x4& a, const u32x4& b) {
    float fa[ET<T>::VEC], fb[ET<T>::VEC];
    ET<T>::unpack(a, fa);
    ET<T>::unpack(b, fb);
#pragma unroll
    for (int i = 0; i < ET<T>::VEC; ++i) fa[i] += fb[i];
    return ET<T>::pack(fa);
}

// candidate padded-grid coordinates that reflect onto h (MirrorPadGrad preimages); returns count, fills j[3]
__device__ inline int reflect_preimages(int h, int H, int p, int* j) {
    int n = 0;
    j[n++] = h + p;
    if (h >= 1 && h <= p) j[n++] = p - h;
    if (h >= H - 1 - p && h <= H - 2) j[n++] = p + 2 * (H - 1) - h;
    return n;
}

// -------------------------------------------------------------------------------------------------
// Border fold: the second, small launch of a REFLECT data gradient whose main kernel (conv_halo_narrow_in_kernel or
// conv_halo_fwd_kernel with mirrored taps) treated the padding as zeros.  It visits only the pixels MirrorPadGrad adds mirrored
// terms to -- rows 1..p, H-1-p..H-2 (all columns), then the same columns of the remaining rows -- gathers the MIRRORED preimages
// of each (pixel, tap) from dy, multiplies by Wd[c][tap,k] and ADDS the product to the dx the main launch stored.
// 64 pixels x BN channels per block of 4 waves, register-staged through one LDS stage; few (pixel, tap) pairs have a mirrored
// source, so K-tiles in which no row of the block has one are skipped.  The bands must be disjoint: H, W > 2p + 1 (launch_border).
// Rounding: the dx it reads back is already rounded to the storage type, and the sum is rounded again -- in bf16 the band's
// values are bf16(bf16(dx_zero_padded) + mirrored terms), not the once-rounded dx the N7 and generic routes give for the same
// layer (include/sggan.h states it at sgg_conv2d_bwd_data; tests/test_gpu_conv_rounding.py pins both values).  f32: exact sums stay exact.
// -------------------------------------------------------------------------------------------------
template <typename T, int BN, int WGM>
__global__ __launch_bounds__(256) void conv_border_fold_kernel(ConvArgs a) {
    constexpr int VEC = ET<T>::VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int BM = 64;
    constexpr int WGN = 4 / WGM;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int MI = WM / 16, NI = WN / 16;
    constexpr int PA = BM / 32;                 // pixel-tile chunks per thread
    constexpr int QA = (BN + 31) / 32;          // weight-tile chunks per thread
    static_assert(WM % 16 == 0 && WN % 16 == 0, "tile shape");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sP = smem;                    // [BM][128]
    char* sQ = smem + BM * 128;         // [BN][128]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int wm = wave / WGN, wn = wave % WGN;
    const int SC = a.K, DC = a.C;                            // reduction channels (dy), destination channels (dx)
    const int cpv = SC / VEC;                                // 16-byte chunks per tap
    const int wrow = a.R * a.S * SC;                         // weight row length (elements)
    const int p = a.pad_t, p2 = 2 * p;
    const int Bimg = p2 * a.W + (a.H - p2) * p2;             // border pixels per image
    const int M = a.N * Bimg;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (m0 >= M) return;

    // m -> (image, h, w): the 2p border ROW bands first, then the 2p border COLUMNS of the remaining rows
    auto decode = [&](int m, int& n, int& h, int& w) {
        n = m / Bimg;
        int q = m - n * Bimg;
        if (q < p2 * a.W) {
            int hi = q / a.W;
            w = q - hi * a.W;
            h = hi < p ? 1 + hi : a.H - 1 - p + (hi - p);
        } else {
            q -= p2 * a.W;
            int hh = q / p2, wi = q - hh * p2;
            h = hh == 0 ? 0 : (hh == a.H - p2 - 1 ? a.H - 1 : p + hh);
            w = wi < p ? 1 + wi : a.W - 1 - p + (wi - p);
        }
    };

    // per-thread staging rows: row = (tid>>3) + 32*i, chunk column c = tid&7
    const int cc0 = tid & 7;
    int rn[PA], rh[PA], rw[PA];                              // image (-1: past the last pixel) and destination h / w
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        int m = m0 + (tid >> 3) + 32 * i;
        rn[i] = -1;
        if (m < M) decode(m, rn[i], rh[i], rw[i]);
    }

    // tap iterator of this thread's chunk column (shared by all its rows)
    int t_cc, t_r, t_s;
    { int ti = cc0 / cpv; t_cc = cc0 - ti * cpv; t_r = ti / a.S; t_s = ti - t_r * a.S; }
    const int ktiles = (a.R * a.S * cpv + 7) / 8;

    u32x4 regP[PA], regQ[QA];
    bool anyP = false;                                       // did this thread load anything for the tile

    auto load_tile = [&]() {
        anyP = false;
        const bool tapok = t_r < a.R;
        // weights
#pragma unroll
        for (int i = 0; i < QA; ++i) {
            int row = (tid >> 3) + 32 * i, dc = n0 + row;
            regQ[i] = zero16();
            if (tapok && row < BN && dc < DC)
                regQ[i] = ld16(a.wmat + ((size_t)dc * wrow + (size_t)(t_r * a.S + t_s) * SC + t_cc * VEC) * ES);
        }
        // pixels: the sum over the MIRRORED preimages only (the direct term was written by the main launch)
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            regP[i] = zero16();
            if (!tapok || rn[i] < 0) continue;
            int jh[3], jw[3];
            int nh = reflect_preimages(rh[i], a.H, a.pad_t, jh);
            int nw = reflect_preimages(rw[i], a.W, a.pad_l, jw);
            bool first = true;
            for (int ia = 0; ia < nh; ++ia)
                for (int ib = 0; ib < nw; ++ib) {
                    if (ia == 0 && ib == 0) continue;
                    int ho = jh[ia] - t_r, wo = jw[ib] - t_s;
                    if ((unsigned)ho < (unsigned)a.Ho && (unsigned)wo < (unsigned)a.Wo) {
                        u32x4 v = ld16(a.src + (((size_t)rn[i] * a.Ho + ho) * a.Wo + wo) * SC * ES + t_cc * 16);
                        regP[i] = first ? v : chunk_add<T>(regP[i], v);
                        first = false;
                    }
                }
            anyP |= !first;
        }
        // advance the tap iterator by one K-tile (8 chunks)
        t_cc += 8;
        while (t_cc >= cpv) { t_cc -= cpv; if (++t_s == a.S) { t_s = 0; ++t_r; } }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            int row = (tid >> 3) + 32 * i;
            st16(sP + row * 128 + ((cc0 ^ ((row >> 1) & 7)) << 4), regP[i]);
        }
#pragma unroll
        for (int i = 0; i < QA; ++i) {
            int row = (tid >> 3) + 32 * i;
            if (row < BN) st16(sQ + row * 128 + ((cc0 ^ ((row >> 1) & 7)) << 4), regQ[i]);
        }
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4, fsw = frow >> 1;   // fragment row / k-chunk / swizzle key

    auto compute_tile = [&]() {
        const char* bP = sP + (wm * WM + frow) * 128;
        const char* bQ = sQ + (wn * WN + frow) * 128;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int off = (((fq + 4 * kk) ^ fsw) << 4);
            u32x4 fp[MI], fw[NI];
#pragma unroll
            for (int j = 0; j < MI; ++j) fp[j] = ld16(bP + j * 16 * 128 + off);
#pragma unroll
            for (int i = 0; i < NI; ++i) fw[i] = ld16(bQ + i * 16 * 128 + off);
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j) {
                    if constexpr (sizeof(T) == 2) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8, fw[i]), __builtin_bit_cast(bf16x8, fp[j]), acc[i][j], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                __uint_as_float(fw[i][e]), __uint_as_float(fp[j][e]), acc[i][j], 0, 0, 0);
                    }
                }
        }
    };

    for (int kt = 0; kt < ktiles; ++kt) {
        load_tile();
        if (!__syncthreads_or(anyP ? 1 : 0)) continue;       // also fences the previous tile's LDS reads
        store_tile();
        __syncthreads();
        compute_tile();
    }

    // ---- epilogue: lane holds D[channel = 4*fq + e][pixel = frow] of each 16x16 tile; add it to what the main launch wrote ----
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        int m = m0 + wm * WM + j * 16 + frow;
        if (m >= M) continue;
        int n, h, w;
        decode(m, n, h, w);
        const size_t dpix = ((size_t)n * a.H + h) * a.W + w;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            int dc = n0 + wn * WN + i * 16 + fq * 4;
            if (dc >= DC) continue;
            float v[4];
            T* o = reinterpret_cast<T*>(a.dst) + dpix * DC + dc;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + (float)o[e];
            if constexpr (sizeof(T) == 2) {
                bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                *reinterpret_cast<bf16x4*>(o) = pk;
            } else {
                *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// The generic GEMM kernel: direct-to-LDS staging (global_load_lds_dwordx4), single 32 KB LDS stage, ~4 blocks per CU.
//
// Each wave-instruction writes 1 KiB = 8 tile rows x 128 B linearly (LDS dest = wave-uniform base + lane*16), so the
// XOR swizzle is applied on the SOURCE side: lane (row, pos) fetches logical chunk pos ^ swz(row) and the fragment
// reads look chunk j up at position j ^ swz(row) (same involution).  Out-of-range taps / rows read a 16-byte zero
// page instead of branching.  Two LDS stages: the DMA of tile t+1 is in flight while tile t is multiplied.
// Tiles up to 256x256 with 8 waves (one block per CU): 128 FLOP per staged byte keeps the L2->LDS stream under
// what the memory side delivers (PMC: the 128x128 variant was bound there at ~9 TB/s of L2 reads, 93 % hits).
// -------------------------------------------------------------------------------------------------

template <typename T, int MODE, int BM, int BN, int WGM, int NW, int BKB, int NS>
__global__ __launch_bounds__(NW * 64) void conv_gemm_glds_kernel(ConvArgs a_in) {
    // grouped launch (a.grp == 2): blockIdx.z = group * classes + parity class; group 1 is the second network's call
    ConvArgs a = a_in;
    const int zclasses = (MODE == MODE_DGRAD) ? a.stride * a.stride : 1;
    const int zgrp = (int)blockIdx.z / zclasses, zcls = (int)blockIdx.z - zgrp * zclasses;
    if (zgrp) {
        a.src += a.net_src; a.dst += a.net_dst; a.wmat = a.wmat2; a.bias = a.bias2;
        if (a.addend) a.addend += a.net_add;
        if (a.partial) a.partial = reinterpret_cast<float*>(reinterpret_cast<char*>(a.partial) + a.net_part);
    }
    constexpr int VEC = ET<T>::VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int WGN = NW / WGM;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int MI = WM / 16, NI = WN / 16;
    constexpr int CPR = BKB / 16;               // 16-byte chunks per LDS row (8: 128-byte K-slices, 4: 64-byte)
    constexpr int RPW = 64 / CPR;               // tile rows per 1-KiB wave-instruction
    constexpr int RPP = NW * RPW;               // tile rows staged per pass
    constexpr int PA = BM / RPP;
    constexpr int QA = (BN + RPP - 1) / RPP;
    constexpr int BNR = QA * RPP;               // weight-tile rows incl. padding
    constexpr int STAGE = (BM + BNR) * BKB;     // bytes per LDS stage
    constexpr int LPT = PA + QA;                // DMA instructions per thread per K-tile
    constexpr int KK = BKB / 64;                // 32-element MFMA k-steps per K-tile
    static_assert(BKB == 128 || BKB == 64, "row bytes");
    static_assert(NS >= 2 && (NS - 2) * LPT <= 63, "stages / vmcnt range");
    static_assert(MODE == MODE_FWD || MODE == MODE_DGRAD, "mode");
    static_assert(BM % RPP == 0 && WM % 16 == 0 && WN % 16 == 0 && WGM * WGN == NW, "tile shape");

    extern __shared__ __attribute__((aligned(16))) char smem[];   // NS stages of { P [BM][BKB], Q [BNR][BKB] }

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int wm = wave / WGN, wn = wave % WGN;
    const int st = (MODE == MODE_DGRAD) ? a.stride : 1;
    const int ph = (MODE == MODE_DGRAD) ? zcls / a.stride : 0;
    const int pw = (MODE == MODE_DGRAD) ? zcls % a.stride : 0;
    const int nr = ph < a.R ? (a.R - ph + st - 1) / st : 0;
    const int ns = pw < a.S ? (a.S - pw + st - 1) / st : 0;
    const int SC = (MODE == MODE_FWD) ? a.C : a.K;
    const int DC = (MODE == MODE_FWD) ? a.K : a.C;
    const int cpv = SC / VEC;
    const int wrow = a.R * a.S * SC;

    // ---- pixel space of this block ----
    int hbase = 0, wbase = 0, Hc, Wc;
    if (MODE == MODE_FWD) { Hc = a.Ho; Wc = a.Wo; }
    else {
        hbase = ((ph - a.pad_t) % st + st) % st;
        wbase = ((pw - a.pad_l) % st + st) % st;
        Hc = hbase < a.H ? (a.H - hbase + st - 1) / st : 0;
        Wc = wbase < a.W ? (a.W - wbase + st - 1) / st : 0;
    }
    const int M = a.N * Hc * Wc;
    const int tilesN = (DC + BN - 1) / BN;
    // 1-D grid over (M-tile, N-tile) pairs, N fastest, so the N-tiles of one pixel tile run back to back; blocks are
    // remapped so that each XCD (blocks b, b+8, ... share one) walks a CONTIGUOUS range of pixel tiles: the halo rows
    // that neighbouring tiles re-read then hit that XCD's private L2 (speed only; any placement is correct).
    int lid;
    {
        const int b = (int)blockIdx.x, nm = (int)gridDim.x;
        const int q = nm >> 3, rr = nm & 7, xcd = b & 7;
        lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
    }
    const int m0 = (lid / tilesN) * BM, n0 = (lid % tilesN) * BN;
    if (m0 >= M) return;

    auto decode = [&](int m, int& n, int& h, int& w) {
        n = m / (Hc * Wc);
        int rem = m - n * (Hc * Wc);
        int hp = rem / Wc;
        h = hbase + st * hp; w = wbase + st * (rem - hp * Wc);
    };

    // swizzle key of a tile row: 128-byte rows: (row>>1)&7; 64-byte rows: (-(row>>2))&3  (both make every 16-lane
    // ds_read_b128 group hit 16 distinct 16-byte slots of the 256-byte bank line)
    auto swz = [](int row) { return CPR == 8 ? ((row >> 1) & 7) : ((-(row >> 2)) & 3); };
    // staging rows of this thread: row = tid/CPR + RPP*i at LDS position tid%CPR; logical chunk = pos ^ swz(row),
    // and swz(row) is the same for every pass i (RPP is a multiple of 16)
    const int srow0 = tid / CPR;
    const int lcc = (tid % CPR) ^ swz(srow0);
    int rn[PA], rh[PA], rw[PA];
    const bool fold = (MODE == MODE_DGRAD) && a.reflect;     // REFLECT data-gradient: MirrorPadGrad terms on the border
    unsigned bmask = 0;                                       // rows of this thread that receive mirrored terms
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        int m = m0 + srow0 + RPP * i;
        if (m < M) {
            int n, h, w;
            decode(m, n, h, w);
            rn[i] = n;
            if (fold) {
                // border pixel -> its row in the pre-folded side tensor (same enumeration as fold_gather_kernel)
                const int p = a.pad_t, p2 = 2 * p;
                const bool all = a.H <= p2 + 1 || a.W <= p2 + 1;
                const bool rowband = (h >= 1 && h <= p) || (h >= a.H - 1 - p && h <= a.H - 2);
                const bool colband = (w >= 1 && w <= p) || (w >= a.W - 1 - p && w <= a.W - 2);
                if (all || rowband || colband) {
                    int q, Bimg;
                    if (all) { Bimg = a.H * a.W; q = h * a.W + w; }
                    else {
                        Bimg = p2 * a.W + (a.H - p2) * p2;
                        if (rowband) q = (h <= p ? h - 1 : p + h - (a.H - 1 - p)) * a.W + w;
                        else {
                            int hh = h == 0 ? 0 : (h == a.H - 1 ? a.H - p2 - 1 : h - p);
                            int wi = w <= p ? w - 1 : p + w - (a.W - 1 - p);
                            q = p2 * a.W + hh * p2 + wi;
                        }
                    }
                    bmask |= 1u << i;
                    rh[i] = n * Bimg + q; rw[i] = 0;
                    continue;
                }
            }
            if (MODE == MODE_FWD) { rh[i] = h * a.stride - a.pad_t; rw[i] = w * a.stride - a.pad_l; }
            else { rh[i] = (h + a.pad_t - ph) / st; rw[i] = (w + a.pad_l - pw) / st; }
        } else rn[i] = -1;
    }

    // split-K (a.ksplit > 1): blockIdx.y selects a contiguous range of K-tiles; partial sums go to f32 slabs
    const int ktot = (nr * ns * cpv + CPR - 1) / CPR;
    const int kper = (ktot + a.ksplit - 1) / a.ksplit;
    const int kt0 = (int)blockIdx.y * kper;
    const int ktiles = SGG_ABLATE_OF(a) >= 5 ? 0 : max(0, min(ktot, kt0 + kper) - kt0);   // ablate 5/6: no main loop
    int t_cc, t_ri, t_si;
    { int q0 = lcc + kt0 * CPR; int ti = q0 / cpv; t_cc = q0 - ti * cpv; t_ri = ns ? ti / ns : nr; t_si = ns ? ti - t_ri * ns : 0; }
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    // Source addresses are kept per tap: the row/weight base pointers are rebuilt only when this thread's chunk
    // column moves to another tap (every SC/(VEC*CPR) K-tiles); within a tap a K-tile costs one 64-bit add per DMA.
    const char* pbase[PA];
    const char* qbase[QA];
    unsigned pok = 0, qok = 0;
    bool tapchg = true;
    auto rebuild = [&]() {
        const bool tapok = t_ri < nr;
        const int r = ph + st * t_ri, s = pw + st * t_si;
        pok = 0; qok = 0;
#pragma unroll
        for (int i = 0; i < QA; ++i) {
            int dc = n0 + srow0 + RPP * i;
            qbase[i] = zero;
            if (tapok && dc < DC) { qbase[i] = a.wmat + ((size_t)dc * wrow + (size_t)(r * a.S + s) * SC) * ES; qok |= 1u << i; }
        }
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            pbase[i] = zero;
            if (!tapok || rn[i] < 0) continue;
            if (MODE == MODE_FWD) {
                int hi = rh[i] + r, wi = rw[i] + s;
                bool ok = true;
                if (a.reflect) {
                    hi = hi < 0 ? -hi : (hi >= a.H ? 2 * (a.H - 1) - hi : hi);
                    wi = wi < 0 ? -wi : (wi >= a.W ? 2 * (a.W - 1) - wi : wi);
                } else ok = (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
                if (ok) { pbase[i] = a.src + (((size_t)rn[i] * a.H + hi) * a.W + wi) * SC * ES; pok |= 1u << i; }
            } else if (fold && ((bmask >> i) & 1u)) {
                // MirrorPadGrad: border pixels gather from the side tensor, whose row (pixel, tap) already
                // holds the sum over the mirrored preimages (fold_gather_kernel)
                pbase[i] = a.fold + ((size_t)rh[i] * (a.R * a.S) + (r * a.S + s)) * SC * ES; pok |= 1u << i;
            } else {
                int ho = rh[i] - t_ri, wo = rw[i] - t_si;
                if ((unsigned)ho < (unsigned)a.Ho && (unsigned)wo < (unsigned)a.Wo) {
                    pbase[i] = a.src + (((size_t)rn[i] * a.Ho + ho) * a.Wo + wo) * SC * ES; pok |= 1u << i;
                }
            }
        }
    };
    auto stage_tile = [&](int stg) {
        char* sP = smem + stg * STAGE;
        char* sQ = sP + BM * BKB;
        if (tapchg) { rebuild(); tapchg = false; }
        const int coff = t_cc * 16;
#pragma unroll
        for (int i = 0; i < QA; ++i) {
            const char* src = qbase[i] + (((qok >> i) & 1u) ? coff : 0);
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sQ + (wave * RPW + RPP * i) * BKB));
        }
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const char* src = pbase[i] + (((pok >> i) & 1u) ? coff : 0);
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sP + (wave * RPW + RPP * i) * BKB));
        }
        t_cc += CPR;
        while (t_cc >= cpv) { t_cc -= cpv; tapchg = true; if (++t_si == ns) { t_si = 0; ++t_ri; } }
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    const int fswP = swz(wm * WM + frow), fswQ = swz(wn * WN + frow);   // tile bases are multiples of 16: key per lane

    // NS-stage ring: NS-1 tiles are in flight by DMA while one is multiplied; counted vmcnt leaves NS-2 of them
    // outstanding across the (raw) barrier -- a __syncthreads() there would drain the whole queue.
    auto wait_tiles = [&](bool steady) {
        if (steady) sgg_wait_vm<(NS - 2) * LPT>();
        else SGG_WAIT_VM0();
    };
    for (int t = 0; t < NS - 1; ++t)
        if (t < ktiles) stage_tile(t);
    wait_tiles(ktiles >= NS - 1);
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < ktiles; ++kt) {
        const int cur = kt % NS;
        const bool refill = kt + NS - 1 < ktiles;
        if (refill && (SGG_ABLATE_OF(a) == 0 || SGG_ABLATE_OF(a) == 2)) stage_tile((kt + NS - 1) % NS);
        const char* bP = smem + cur * STAGE + (wm * WM + frow) * BKB;
        const char* bQ = smem + cur * STAGE + BM * BKB + (wn * WN + frow) * BKB;
        if (SGG_ABLATE_OF(a) != 2) {
            // Fragment pipeline: all weight fragments of the tile up front, pixel fragments in groups of GJ that are
            // fetched one group ahead of the MFMAs that consume them, so the ~100-cycle LDS latency hides behind
            // GJ*NI MFMAs instead of stalling every 8 (what hipcc emitted for the plain j-loop).
            constexpr int GJ = MI >= 4 ? 4 : MI;             // pixel fragments per group
            constexpr int GPK = MI / GJ;                      // groups per k-step
            constexpr int NG = KK * GPK;
            u32x4 fw[KK][NI];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                for (int i = 0; i < NI; ++i) fw[kk][i] = ld16(bQ + i * 16 * BKB + (((fq + 4 * kk) ^ fswQ) << 4));
            u32x4 fp[2][GJ];
#pragma unroll
            for (int jj = 0; jj < GJ; ++jj) fp[0][jj] = ld16(bP + jj * 16 * BKB + ((fq ^ fswP) << 4));
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int kk = g / GPK, jb = (g % GPK) * GJ;
                if (g + 1 < NG) {
                    const int kn = (g + 1) / GPK, jn = ((g + 1) % GPK) * GJ;
#pragma unroll
                    for (int jj = 0; jj < GJ; ++jj)
                        fp[(g + 1) & 1][jj] = ld16(bP + (jn + jj) * 16 * BKB + (((fq + 4 * kn) ^ fswP) << 4));
                }
                __builtin_amdgcn_sched_barrier(0);           // keep the prefetch ABOVE this group's MFMAs
#pragma unroll
                for (int jj = 0; jj < GJ; ++jj)
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        if constexpr (sizeof(T) == 2) {
                            acc[i][jb + jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                __builtin_bit_cast(bf16x8, fw[kk][i]), __builtin_bit_cast(bf16x8, fp[g & 1][jj]), acc[i][jb + jj], 0, 0, 0);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[i][jb + jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                    __uint_as_float(fw[kk][i][e]), __uint_as_float(fp[g & 1][jj][e]), acc[i][jb + jj], 0, 0, 0);
                        }
                    }
            }
        }
        wait_tiles(refill);
        SGG_WAIT_LGKM0();
        if (SGG_ABLATE_OF(a) < 3) __builtin_amdgcn_s_barrier();
    }

    // bias of this lane's 4 output channels per channel tile, fetched once (a per-store load would put a full
    // L2 round trip in front of every one of the NI*MI stores)
    if (SGG_ABLATE_OF(a) == 6) return;
    float bv[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int dc = n0 + wn * WN + i * 16 + fq * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[i][e] = (a.bias && a.ksplit <= 1 && dc < DC) ? a.bias[dc + e] : 0.f;
    }
    // uniform conditions (split-K, activation, addend) are tested once, outside the unrolled store loops
    auto epilogue = [&](auto mode_c) {
        constexpr int EP = decltype(mode_c)::value;               // -1: split-K partial; else 2 * ACT + (addend ? 1 : 0)
        if constexpr (EP >= 0 && sizeof(T) == 2 && MI % 2 == 0) {
            // 16-byte stores (see conv3x3_halo_gemm_kernel's epilogue): pixel fragments 2 jp and 2 jp + 1 trade halves between lane
            // rows, a lane then owns 8 consecutive channels of one GEMM row -- half the store instructions, same values
            const int jo = fq & 1, cb = (fq >> 1) * 8;
#pragma unroll
            for (int jp = 0; jp < MI / 2; ++jp) {
                const int m = m0 + wm * WM + (2 * jp + jo) * 16 + frow;
                const bool mok = m < M;
                size_t dpix = (size_t)m;
                if (!(MODE == MODE_FWD || st == 1)) {
                    int n, h, w;
                    decode(mok ? m : 0, n, h, w);
                    dpix = ((size_t)n * a.H + h) * a.W + w;
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int dc = n0 + wn * WN + i * 16 + cb;
                    const bool ok = mok && dc < DC;
                    float v0[4], v1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v0[e] = act_apply_c<EP / 2>(acc[i][2 * jp][e] + bv[i][e], a.leak);
                        v1[e] = act_apply_c<EP / 2>(acc[i][2 * jp + 1][e] + bv[i][e], a.leak);
                    }
                    u32x4 pk;
                    if constexpr (EP & 1) {
                        pk = row_swap16_add_pack(v0, v1, ok ? ld16(reinterpret_cast<const bf16*>(a.addend) + dpix * DC + dc) : zero16());
                    } else {
                        const bf16x4 p0 = {(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3]}, p1 = {(bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
                        pk = row_swap16_pack(p0, p1);
                    }
                    if (ok) st16(reinterpret_cast<bf16*>(a.dst) + dpix * DC + dc, pk);
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            int m = m0 + wm * WM + j * 16 + frow;
            if (m >= M) continue;
            size_t dpix;
            if (MODE == MODE_FWD || st == 1) dpix = (size_t)m;       // stride 1: destination pixel index == GEMM row
            else {
                int n, h, w;
                decode(m, n, h, w);
                dpix = ((size_t)n * a.H + h) * a.W + w;
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                int dc = n0 + wn * WN + i * 16 + fq * 4;
                if (dc >= DC) continue;
                if constexpr (EP < 0) {                              // f32 partial; bias/activation are applied by the reducer
                    float* o = a.partial + ((size_t)blockIdx.y * a.pdst + dpix) * DC + dc;
                    *reinterpret_cast<f32x4*>(o) = acc[i][j];
                } else {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_apply_c<EP / 2>(acc[i][j][e] + bv[i][e], a.leak);
                    if constexpr (EP & 1) {                          // + skip-connection gradient (module.py:217 backward)
                        const T* ad = reinterpret_cast<const T*>(a.addend) + dpix * DC + dc;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += (float)ad[e];
                    }
                    T* o = reinterpret_cast<T*>(a.dst) + dpix * DC + dc;
                    if constexpr (sizeof(T) == 2) {
                        bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                        *reinterpret_cast<bf16x4*>(o) = pk;
                    } else {
                        *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
                    }
                }
            }
        }
    };
    if (a.ksplit > 1) epilogue(std::integral_constant<int, -1>{});
    else act_dispatch(a.act, [&](auto act_c) {
        constexpr int ACT = decltype(act_c)::value;
        if (a.addend) epilogue(std::integral_constant<int, 2 * ACT + 1>{});
        else epilogue(std::integral_constant<int, 2 * ACT>{});
    });
}

// -------------------------------------------------------------------------------------------------
// 3x3 STRIDE-2 data gradient / Conv2DTranspose forward with the dy halo resident in LDS and all four output-parity
// classes computed by one block (module.py:230-236 backward, :254-258 forward; D's module.py:284-294 backward).
//
// The generic kernel gives every parity class its own blocks with 128x64 tiles: K loops of 2-8 tiles, 43 FLOP per staged
// byte, and every dy pixel fetched once per tap.  Here a block owns an 8 x 32 tile of dy pixels = a 16 x 64 tile of
// output pixels x 64 output channels: per 64-channel chunk of dy the 10 x 34 halo is staged once (double-buffered
// across chunks) and the nine taps -- 4 + 2 + 2 + 1 over the classes -- read shifted rows of it; weights stream per
// kernel row (3 taps, 24 KB) through a 2-stage ring.  3.6x fewer L2->LDS bytes, no per-class prologue.
// Wave w owns dy row w of the tile (two 16-pixel fragments) x all 64 channels x 4 classes = 32 MFMA tiles.
// Output pixel (2i+a, 2j+b) of class (a,b) takes tap (r,s) with a = (r+pad_t)&1, b = (s+pad_l)&1 from dy pixel
// (i + (a+pad_t-r)/2, j + (b+pad_l-s)/2), zero outside dy.
// -------------------------------------------------------------------------------------------------
#define S2_TI 8
#define S2_TJ 32
#define S2_PITCH 40                                    // halo row pitch in pixels (34 used)
#define S2_HALO_BYTES ((S2_TI + 2) * S2_PITCH * 128)   // 51200
#define S2_WSTAGE (3 * 64 * 128)                       // one kernel row of taps x 64 output channels x 128 B
#define S2_LDS (2 * S2_HALO_BYTES + 2 * S2_WSTAGE)    // 151552

// (the norm statistics of a Conv2DTranspose forward are a launch of their own, deconv_s2_stats_kernel: the kernel sits at 251 VGPRs and
// every form of a statistics epilogue inside it spilled)
template <int PT, int PL>                              // pad_t, pad_l (0 or 1): compile-time so that each tap's class is static
__global__ __launch_bounds__(512) void deconv_s2_halo_kernel(ConvArgs a, int total_tiles, int tiles_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sH = smem;                                   // 2 x halo [10][40][128 B]
    char* sW = smem + 2 * S2_HALO_BYTES;               // 2 x [3 taps][64 c][128 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int SC = a.K, DC = a.C;                      // dy channels (reduction), dx channels
    const int wrow = 9 * SC, nchunk = SC >> 6;
    const int tilesN = DC >> 6, tilesJ = a.Wo / S2_TJ, tilesI = a.Ho / S2_TI;
    // Persistent blocks: block `lid` (XCD-contiguous numbering) walks tiles lid*tiles_per_block ... in order, so the
    // prologue of a tile (halo + first weights) is fetched under the last stage of the previous one and the output
    // stores of a tile drain under the next tile's MFMAs; consecutive tiles share halo columns (L2 hits).
    int lid;
    {
        const int b = (int)blockIdx.x, nm = (int)gridDim.x;
        const int q = nm >> 3, rr = nm & 7, xcd = b & 7;
        lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
    }
    const int t_beg = lid * tiles_per_block;
    const int t_end = min(total_tiles, t_beg + tiles_per_block);
    if (t_beg >= t_end) return;
    struct Tile { int img, i0, j0, n0; };
    auto decode = [&](int t) {
        Tile T;
        T.n0 = (t % tilesN) * 64;
        int mt = t / tilesN;
        T.j0 = (mt % tilesJ) * S2_TJ; mt /= tilesJ;
        T.i0 = (mt % tilesI) * S2_TI;
        T.img = mt / tilesI;
        return T;
    };
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int hpos = lane & 7, hsub = lane >> 3;

    // halo of one 64-channel chunk: 10 rows x 5 DMAs of 8 pixels; wave w issues q = w, w+8, ...
    auto load_halo = [&](int buf, const Tile& T, int chunk) {
        char* dstb = sH + buf * S2_HALO_BYTES;
#pragma unroll
        for (int it = 0; it < 7; ++it) {
            const int q = wave + 8 * it;
            if (q >= (S2_TI + 2) * 5) break;
            const int k = q / 5, cg = q - 5 * k;
            const int hp = cg * 8 + hsub;
            const int hi = T.i0 - 1 + k, wi = T.j0 - 1 + hp;
            const bool ok = hp < S2_TJ + 2 && (unsigned)hi < (unsigned)a.Ho && (unsigned)wi < (unsigned)a.Wo;
            // rotation swizzle of the halo rows (conflict-free fragment reads for every tap shift; see conv3x3_halo_gemm_kernel)
            const int hrow_ = k * S2_PITCH + hp;
            const int schunk = (hpos - (hrow_ & 6)) & 7;
            const char* src = ok ? a.src + ((((size_t)T.img * a.Ho + hi) * a.Wo + wi) * SC + chunk * 64) * 2 + (schunk << 4) : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(dstb + (k * S2_PITCH + cg * 8) * 128));
        }
    };
    // weights of kernel row r, chunk: 3 taps x 64 rows x 128 B = 24 DMAs of 8 rows; wave w issues 3w..3w+2
    auto load_w = [&](int stg, const Tile& T, int chunk, int r) {
        char* dstb = sW + stg * S2_WSTAGE;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int q = wave * 3 + it;                // 0..23: tap column s = q / 8, rows 8*(q%8)..
            const int sx = q >> 3, row = (q & 7) * 8 + hsub;
            const int key = (((sx * 64 + row) >> 1) & 7);
            const char* wm = T.img >= a.nsplit ? a.wmat2 : a.wmat;      // stacked batch of two networks: per-image weights
            const char* src = wm + ((size_t)(T.n0 + row) * wrow + (size_t)(r * 3 + sx) * SC + chunk * 64) * 2 + ((hpos ^ key) << 4);
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(dstb + q * 1024));
        }
    };

    f32x4 acc[4][2][4];                                // [class][pixel fragment][channel tile]
    const int frow = lane & 15, fq = lane >> 4;
    Tile cur = decode(t_beg);
    load_halo(0, cur, 0);
    load_w(0, cur, 0, 0);
    SGG_WAIT_VM0();
    __builtin_amdgcn_s_barrier();

    const int nqc = (t_end - t_beg) * nchunk;          // (tile, chunk) pairs of this block
    int chunk = 0, tcur = t_beg;
    for (int qc = 0; qc < nqc; ++qc) {
        if (chunk == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[c][j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        // the (tile, chunk) after this one
        const bool more = qc + 1 < nqc;
        const bool last_chunk = chunk + 1 == nchunk;
        const Tile nxt = (more && last_chunk) ? decode(tcur + 1) : cur;
        const int nchk = last_chunk ? 0 : chunk + 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int st = qc * 3 + r;
            if (r < 2) load_w((st + 1) & 1, cur, chunk, r + 1);
            else if (more) load_w((st + 1) & 1, nxt, nchk, 0);
            if (r == 0 && more) load_halo((qc + 1) & 1, nxt, nchk);     // that buffer was last read in pair qc-1
            const int ar = (r + PT) & 1, dr = (ar + PT - r) / 2;          // class row parity, dy row offset (compile time)
            const char* hb = sH + (qc & 1) * S2_HALO_BYTES;
            const char* wb = sW + (st & 1) * S2_WSTAGE;
#pragma unroll
            for (int sx = 0; sx < 3; ++sx) {
                const int bs = (sx + PL) & 1, ds = (bs + PL - sx) / 2;
                const int cls = ar * 2 + bs;
                const int hrow = (wave + dr + 1) * S2_PITCH + (ds + 1) + frow;   // halo pixel of fragment 0, this lane
                const int fswP = hrow & 6;
                const char* bP = hb + hrow * 128;
                const int wr = sx * 64 + frow;
                const int fswQ = (wr >> 1) & 7;
                const char* bQ = wb + wr * 128;
                u32x4 fw[2][4], fp[2][2];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) fw[kk][i] = ld16(bQ + i * 16 * 128 + (((fq + 4 * kk) ^ fswQ) << 4));
#pragma unroll
                    for (int j = 0; j < 2; ++j) fp[kk][j] = ld16(bP + j * 16 * 128 + (((fq + 4 * kk + fswP) & 7) << 4));
                }
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            acc[cls][j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fw[kk][i]),
                                                                                      __builtin_bit_cast(bf16x8, fp[kk][j]), acc[cls][j][i], 0, 0, 0);
            }
            SGG_WAIT_VM0();
            SGG_WAIT_LGKM0();
            __builtin_amdgcn_s_barrier();
        }
        if (last_chunk) {
            // epilogue of tile `cur`; the stores drain while the next tile is multiplied
            float bv[4][4];
            const float* const bias_t = cur.img >= a.nsplit ? a.bias2 : a.bias;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[i][e] = bias_t ? bias_t[cur.n0 + i * 16 + fq * 4 + e] : 0.f;
            auto epilogue = [&](auto act_c) {
                constexpr int ACT = decltype(act_c)::value;
                auto store_tile = [&](auto add_c) {
                    constexpr bool ADD = decltype(add_c)::value;
                    // 16-byte stores: the two pixel fragments of a class trade halves between lane rows (row_swap16, see the
                    // 3x3 halo GEMM's epilogue) -- 16 store instructions per wave and tile instead of 32; the layers this
                    // kernel serves move more output bytes per FLOP than any other GEMM of the step
                    const int jo = fq & 1, cb = (fq >> 1) * 8;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int h = 2 * (cur.i0 + wave) + (c >> 1);
                        const int w = 2 * (cur.j0 + jo * 16 + frow) + (c & 1);
                        const size_t dpix = ((size_t)cur.img * a.H + h) * a.W + w;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int dc = cur.n0 + i * 16 + cb;
                            float v0[4], v1[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v0[e] = act_apply_c<ACT>(acc[c][0][i][e] + bv[i][e], a.leak);
                                v1[e] = act_apply_c<ACT>(acc[c][1][i][e] + bv[i][e], a.leak);
                            }
                            u32x4 pk;
                            if constexpr (ADD) {
                                pk = row_swap16_add_pack(v0, v1, ld16(reinterpret_cast<const bf16*>(a.addend) + dpix * DC + dc));
                            } else {
                                const bf16x4 p0 = {(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3]}, p1 = {(bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
                                pk = row_swap16_pack(p0, p1);
                            }
                            st16(reinterpret_cast<bf16*>(a.dst) + dpix * DC + dc, pk);
                        }
                    }
                };
                if (a.addend) store_tile(std::true_type{});
                else store_tile(std::false_type{});
            };
            act_dispatch(a.act, epilogue);
            cur = nxt; ++tcur; chunk = 0;
        } else ++chunk;
    }
}

// Instance-norm statistics of a Conv2DTranspose forward's STORED bf16 output (sgg_deconv2d_fwd_stats): one block per (image, 16 x 64
// output-pixel tile of deconv_s2_halo_kernel, 64 channels) writes that tile's (sum, sumsq) row of channels n0 .. n0 + 63.  The sums are
// formed in the order the tile's own epilogue formed them when it carried them: wave w reads output rows 2w, 2w+1 of the tile; lane
// (frow, fq) adds parity classes c = 0..3 x pixel fragments j = 0..1 of channels 16 i + 4 fq + e, a 16-lane butterfly (fixed order) gives
// one (sum, sumsq) per channel and wave, and 128 threads add the eight waves' rows in wave order.
__global__ __launch_bounds__(512) void deconv_s2_stats_kernel(ConvArgs a) {
    __shared__ float sS[8 * 64 * 2];                   // [wave][channel][sum, sumsq]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int DC = a.C;
    const int tilesN = DC >> 6, tilesJ = a.Wo / S2_TJ, tilesI = a.Ho / S2_TI;
    int t = (int)blockIdx.x;
    const int n0 = (t % tilesN) * 64; t /= tilesN;
    const int j0 = (t % tilesJ) * S2_TJ; t /= tilesJ;
    const int i0 = (t % tilesI) * S2_TI;
    const int img = t / tilesI;
    const bf16* y = reinterpret_cast<const bf16*>(a.dst);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        const int dc = n0 + i * 16 + fq * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int h = 2 * (i0 + wave) + (c >> 1);
                const int w = 2 * (j0 + j * 16 + frow) + (c & 1);
                const bf16x4 v = *reinterpret_cast<const bf16x4*>(y + (((size_t)img * a.H + h) * a.W + w) * DC + dc);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float r = (float)v[e];
                    s1[e] += r; s2[e] += r * r;
                }
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                s1[e] += __shfl_xor(s1[e], off);
                s2[e] += __shfl_xor(s2[e], off);
            }
        }
        if (frow == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float* o = sS + ((wave * 64) + i * 16 + fq * 4 + e) * 2;
                o[0] = s1[e]; o[1] = s2[e];
            }
        }
    }
    __syncthreads();
    if (tid < 128) {
        const int ch = tid >> 1, which = tid & 1;
        float acc = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) acc += sS[(w8 * 64 + ch) * 2 + which];
        const int chunks = tilesI * tilesJ;
        const int chunk = (i0 / S2_TI) * tilesJ + j0 / S2_TJ;
        a.stats[(((size_t)img * chunks + chunk) * DC + n0 + ch) * 2 + which] = acc;
    }
}

// (a question about the shape alone, like halo3_ok: plan_conv never splits K for a shape this kernel takes)
static bool s2halo_ok(const sgg_conv_desc* d) {
    const SggConfig& cfg = sgg_config();
    if (!cfg.s2halo || d->dtype != SGG_BF16 || cfg.ablate || d->pad_mode == SGG_PAD_REFLECT) return false;
    if (d->R != 3 || d->S != 3 || d->stride != 2 || d->H != 2 * d->Ho || d->W != 2 * d->Wo) return false;
    if (d->pad_t != 0 || d->pad_l != 0) return false;     // TF 'SAME' with an even input pads bottom/right only
    return d->K % 64 == 0 && d->C % 64 == 0 && d->Wo % S2_TJ == 0 && d->Ho % S2_TI == 0;
}

template <int PT, int PL>
static int launch_s2halo_p(const ConvArgs& a, hipStream_t s) {
    auto kern = deconv_s2_halo_kernel<PT, PL>;
    SGG_LDS_ATTR(kern, S2_LDS);
    const int total = (int)((int64_t)a.N * (a.Ho / S2_TI) * (a.Wo / S2_TJ) * (a.C / 64));
    const int tpb = (total + 255) / 256;               // one persistent block per CU
    const int blocks = (total + tpb - 1) / tpb;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), S2_LDS, s, a, total, tpb);
    return sgg_check_launch();
}
static int launch_s2halo(const ConvArgs& a, hipStream_t s) {
    if (!a.stats) return launch_s2halo_p<0, 0>(a, s);
    if (a.addend || a.act != SGG_ACT_NONE) return SGG_EUNSUPPORTED;      // the statistics serve a layer followed by a norm
    const int rc = launch_s2halo_p<0, 0>(a, s);
    if (rc != SGG_OK) return rc;
    const int blocks = a.N * (a.Ho / S2_TI) * (a.Wo / S2_TJ) * (a.C / 64);
    hipLaunchKernelGGL(deconv_s2_stats_kernel, dim3((unsigned)blocks), dim3(512), 0, s, a);
    return sgg_check_launch();
}

// Side tensor of the FOLD variant: [N][H][2 sides][9 taps][K] complete mirrored gather rows of the pixels in columns
// 1 and W-2, then [N][2][W][K] virtual rows dy[2]+dy[0] and dy[H-3]+dy[H-1]   (pad 1)
template <typename T>
__global__ __launch_bounds__(256) void fold_halo_gather_kernel(const char* dy, char* fold, int N, int H, int W, int K) {
    constexpr int VEC = ET<T>::VEC;
    const int cpv = K / VEC;
    const int64_t npatch = (int64_t)N * H * 18 * cpv, total = npatch + (int64_t)N * 2 * W * cpv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
        if (i < npatch) {
            int ch = (int)(i % cpv);
            int64_t t = i / cpv;
            int tap = (int)(t % 9); t /= 9;
            int side = (int)(t & 1); t >>= 1;
            int h = (int)(t % H), n = (int)(t / H);
            int w = side ? W - 2 : 1, r = tap / 3, s = tap - 3 * r;
            int jh[3], jw[3];
            int nh = reflect_preimages(h, H, 1, jh), nw = reflect_preimages(w, W, 1, jw);
            for (int ia = 0; ia < nh; ++ia)
                for (int ib = 0; ib < nw; ++ib) {
                    int ho = jh[ia] - r, wo = jw[ib] - s;
                    if ((unsigned)ho < (unsigned)H && (unsigned)wo < (unsigned)W) {
                        float v[VEC];
                        ET<T>::unpack(ld16(dy + ((((size_t)n * H + ho) * W + wo) * K + (size_t)ch * VEC) * sizeof(T)), v);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) acc[e] += v[e];
                    }
                }
        } else {
            int64_t t = i - npatch;
            int ch = (int)(t % cpv); t /= cpv;
            int w = (int)(t % W); t /= W;
            int which = (int)(t & 1), n = (int)(t >> 1);
            int ha = which ? H - 3 : 2, hb = which ? H - 1 : 0;
            float va[VEC], vb[VEC];
            ET<T>::unpack(ld16(dy + ((((size_t)n * H + ha) * W + w) * K + (size_t)ch * VEC) * sizeof(T)), va);
            ET<T>::unpack(ld16(dy + ((((size_t)n * H + hb) * W + w) * K + (size_t)ch * VEC) * sizeof(T)), vb);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = va[e] + vb[e];
        }
        st16(fold + (size_t)i * 16, ET<T>::pack(acc));
    }
}

// -------------------------------------------------------------------------------------------------
// Narrow-output convolution (Cout <= 16, stride 1, same-size output): the generator head, 7x7 64->3 at full
// resolution (module.py:262-264).  As an implicit GEMM it would re-read every input pixel once per tap (49x) from
// L2 for a 16-wide output tile; here the block keeps the input HALO of its 16x32-pixel output tile in LDS (one
// DMA pass, REFLECT/zero padding resolved in the DMA's per-lane source address) and all taps read shifted rows of
// it.  Weights stream through a small double-buffered LDS ring, one kernel row of taps at a time.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(512) void conv_halo_fwd_kernel(ConvArgs a, int flip) {   // flip: weight taps mirrored (data gradient)
    constexpr int VEC = ET<T>::VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int CCH = 128 / ES;                       // channels per halo pass (one 128-byte LDS row per pixel)
    constexpr int WBUF = HALO_MAXR * 16 * 128;          // one kernel row of taps: [s][16 couts][128 B]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sW = smem;                                    // [2][WBUF]
    char* sH = smem + 2 * WBUF;                         // halo [(TH+R-1)*(TW+S-1)][128 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int HWd = HALO_TW + a.S - 1, HHd = HALO_TH + a.R - 1, HP = HHd * HWd;
    const int tilesW = a.W / HALO_TW, tilesH = a.H / HALO_TH;
    int b = blockIdx.x;
    const int tw = b % tilesW; b /= tilesW;
    const int th = b % tilesH;
    const int n = b / tilesH;
    const int y0 = th * HALO_TH, x0 = tw * HALO_TW;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int wrow = a.R * a.S * a.C;                   // weight row length (elements)
    const int pos = tid & 7, lsw = (tid >> 4) & 7;      // LDS position / swizzle key of rows (tid>>3) + 64*i
    const int lcc = pos ^ lsw;                          // logical 16-byte chunk this thread fetches

    auto stage_halo = [&](int cc) {
        for (int base = 0; base < HP; base += 64) {     // 64 halo pixels (8 per wave-instruction) per pass
            int hp = base + (tid >> 3);
            const char* src = zero;
            if (hp < HP) {
                int hy = hp / HWd, hx = hp - hy * HWd;
                int yi = y0 - a.pad_t + hy, xi = x0 - a.pad_l + hx;
                bool ok = true;
                if (a.reflect) {
                    yi = yi < 0 ? -yi : (yi >= a.H ? 2 * (a.H - 1) - yi : yi);
                    xi = xi < 0 ? -xi : (xi >= a.W ? 2 * (a.W - 1) - xi : xi);
                } else ok = (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
                if (ok) src = a.src + ((((size_t)n * a.H + yi) * a.W + xi) * a.C + cc * CCH) * ES + lcc * 16;
            }
            if (base + wave * 8 < HP + 8)                // wave-uniform: skip instructions wholly past the halo
                dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sH + (base + wave * 8) * 128));
        }
    };
    auto stage_weights = [&](int buf, int r, int cc) {   // taps (r, 0..S-1): rows = s*16 + cout
        for (int base = 0; base < a.S * 16; base += 64) {
            int row = base + (tid >> 3);
            const char* src = zero;
            if (row < a.S * 16) {
                int s = row >> 4, k = row & 15;
                const int tap = flip ? (a.R - 1 - r) * a.S + (a.S - 1 - s) : r * a.S + s;
                if (k < a.K) src = a.wmat + ((size_t)k * wrow + (size_t)tap * a.C + cc * CCH) * ES + lcc * 16;
            }
            if (base + wave * 8 < a.S * 16)
                dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sW + buf * WBUF + (base + wave * 8) * 128));
        }
    };

    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fq = lane >> 4;

    const int nchunks = a.C / CCH;
    for (int cc = 0; cc < nchunks; ++cc) {
        __syncthreads();                                 // previous pass has finished reading the halo
        stage_halo(cc);
        stage_weights(0, 0, cc);
        SGG_WAIT_VM0();
        __syncthreads();
        for (int r = 0; r < a.R; ++r) {
            const int cur = r & 1;
            if (r + 1 < a.R) stage_weights(cur ^ 1, r + 1, cc);
            for (int s = 0; s < a.S; ++s) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int wr = s * 16 + frow;
                    u32x4 fw = ld16(sW + cur * WBUF + wr * 128 + ((((fq + 4 * kk) ^ ((wr >> 1) & 7))) << 4));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int y = 2 * wave + (j >> 1), x = (j & 1) * 16 + frow;
                        const int hp = (y + r) * HWd + x + s;
                        u32x4 fp = ld16(sH + hp * 128 + ((((fq + 4 * kk) ^ ((hp >> 1) & 7))) << 4));
                        if constexpr (sizeof(T) == 2) {
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fw), __builtin_bit_cast(bf16x8, fp), acc[j], 0, 0, 0);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(fw[e]), __uint_as_float(fp[e]), acc[j], 0, 0, 0);
                        }
                    }
                }
            }
            SGG_WAIT_VM0();
            __syncthreads();
        }
    }

    // D[cout = 4*fq + e][pixel = frow]
    const int dc = fq * 4;
    if (dc < a.K) {
        float bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = a.bias ? a.bias[dc + e] : 0.f;
        act_dispatch(a.act, [&](auto act_c) {
            constexpr int ACT = decltype(act_c)::value;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = y0 + 2 * wave + (j >> 1), x = x0 + (j & 1) * 16 + frow;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = act_apply_c<ACT>(acc[j][e] + bv[e], a.leak);
                T* o = reinterpret_cast<T*>(a.dst) + (((size_t)n * a.H + y) * a.W + x) * a.K + dc;
                if constexpr (sizeof(T) == 2) {
                    bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                    *reinterpret_cast<bf16x4*>(o) = pk;
                } else *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
            }
        });
    }
}

// -------------------------------------------------------------------------------------------------
// 7x7, 64 -> 3 channels at full resolution (bf16): the generator head forward (module.py:262-264) and, with mirrored
// taps, the main part of the stem's data gradient (module.py:230-232 backward).
//
// conv_halo_fwd_kernel above puts the 3 output channels in a 16-wide MFMA dimension (13 of 16 columns wasted) and
// reads one LDS fragment per MFMA.  Here the GEMM N dimension carries (output channel, tap COLUMN) = 3 x 7 = 21 -> 32
// and only the tap ROW stays in the reduction:
//     D[q][(co, s)] = sum_{r, c} halo[y + r][q][c] * w[r][s][c][co]          (q = halo column, K = 7 x 64)
//     out[y][p][co] = sum_s D[p + s][(co, s)]                                (a shifted sum, done through LDS)
// i.e. 140 MFMAs per 64 output pixels instead of 392, and one fragment read per 2 MFMAs.  The weight fragments (28 per
// lane) live in registers for the whole block.  One block = 8 output rows x 64 columns, one wave per row; the 14 x 70
// pixel input halo (128 B per pixel) is DMA'd once, REFLECT / zero padding resolved in the per-lane source address.
// -------------------------------------------------------------------------------------------------
#define N7_TH 8
#define N7_TW 64
#define N7_PITCH 72                                     // halo row pitch in pixels (70 used; 9 DMAs of 8)
#define N7_ROWS (N7_TH + 6)
#define N7_LDS (N7_ROWS * N7_PITCH * 128 + 2048)
#define N7_ZP 68                                        // floats per (co, s) row of the shifted-sum buffer

struct N7Args {
    const char* src;     // (N,H,W,64) bf16
    const char* wmat;    // [dest channel][49 taps][64] bf16 (w_fwd of the head / w_dgrad of the stem)
    const float* bias;   // per dest channel or nullptr
    void* dst;           // bf16 (N,Ho,Wo,8)  or  f32 (N,Ho,Wo,4) when dst_f32
    int N, H, W, Ho, Wo, pt, pl, K, reflect, flip, act, dst_f32;
    float leak;
};

__global__ __launch_bounds__(512) void conv7_narrow_out_kernel(N7Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) char lds_char;
    lds_char* const lH = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tilesW = (a.Wo + N7_TW - 1) / N7_TW, tilesH = (a.Ho + N7_TH - 1) / N7_TH;
    const int ntiles = a.N * tilesH * tilesW;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int frow = lane & 15, fq = lane >> 4;
    // ---- weight fragments into registers, once per (persistent) block: 28 x 16 B per lane.  B operand: lane supplies
    // k = 8*(lane/16).., column n = nt*16 + lane%16
    u32x4 wr[7][2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int nn = nt * 16 + frow, co = nn >> 3, sc = nn & 7;
        const bool ok = co < a.K && co < 3 && sc < 7;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const int tap = a.flip ? (6 - r) * 7 + (6 - sc) : r * 7 + sc;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                wr[r][kk][nt] = ok ? ld16(a.wmat + (((size_t)co * 49 + tap) * 64 + kk * 32 + fq * 8) * 2) : zero16();
        }
    }
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int b = tile;
    const int tw = b % tilesW; b /= tilesW;
    const int th = b % tilesH;
    const int n = b / tilesH;
    const int y0 = th * N7_TH, x0 = tw * N7_TW;
    __syncthreads();                                    // the previous tile's shifted-sum buffer (in the halo region) is done

    // ---- halo DMA: 14 rows x 9 instructions of 8 pixels; instruction id = row * 9 + i, dealt round-robin to the waves
    {
        const int hsub = lane >> 3, hpos = lane & 7;
        for (int id = wave; id < N7_ROWS * 9; id += 8) {
            const int hy = id / 9, hx = (id - hy * 9) * 8 + hsub;
            int yi = y0 - a.pt + hy, xi = x0 - a.pl + hx;
            bool ok = hx < N7_TW + 6;
            if (a.reflect) {
                yi = yi < 0 ? -yi : (yi >= a.H ? 2 * (a.H - 1) - yi : yi);
                xi = xi < 0 ? -xi : (xi >= a.W ? 2 * (a.W - 1) - xi : xi);
                ok = ok && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;   // (tiles past the image edge)
            } else ok = ok && (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
            const int hp = hy * N7_PITCH + hx;
            const int key = (hp >> 1) & 7;
            const char* src = ok ? a.src + ((((size_t)n * a.H + yi) * a.W + xi) * 64) * 2 + ((hpos ^ key) << 4) : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(lH + (hy * N7_PITCH + (id - hy * 9) * 8) * 128));
        }
    }
    f32x4 acc[5][2];
#pragma unroll
    for (int qf = 0; qf < 5; ++qf)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[qf][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    SGG_WAIT_VM0();
    __syncthreads();

    // ---- D[q][(co,s)] for this wave's output row: A operand = halo pixels (lane: pixel frow, chunk fq), B = weights
    const char* sH = smem;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const int hrow = wave + r;
        const int key = ((hrow * 4) + (frow >> 1)) & 7;             // (hp >> 1) & 7 with hp = hrow*72 + qf*16 + frow
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const char* base = sH + ((size_t)(hrow * N7_PITCH + frow)) * 128 + (((kk * 4 + fq) ^ key) << 4);
#pragma unroll
            for (int qf = 0; qf < 5; ++qf) {
                const u32x4 px = ld16(base + qf * 16 * 128);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[qf][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, px), __builtin_bit_cast(bf16x8, wr[r][kk][nt]),
                                                                          acc[qf][nt], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                                 // every wave is done with the halo: reuse it for Z

    // ---- shifted sum: Z[(co,s)][p] = D[p + s][(co,s)], then out[p][co] = sum_s Z[(co,s)][p] (fixed order)
    float* Z = reinterpret_cast<float*>(smem) + (size_t)wave * (21 * N7_ZP);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int nn = nt * 16 + frow, co = nn >> 3, sc = nn & 7;
        if (co < 3 && sc < 7) {
#pragma unroll
            for (int qf = 0; qf < 5; ++qf)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int pcol = qf * 16 + fq * 4 + e - sc;
                    if ((unsigned)pcol < (unsigned)N7_TW) Z[(co * 7 + sc) * N7_ZP + pcol] = acc[qf][nt][e];
                }
        }
    }
    SGG_WAIT_LGKM0();
    __builtin_amdgcn_wave_barrier();
    const int y = y0 + wave, x = x0 + lane;
    float o[3];
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        float v = 0.f;
#pragma unroll
        for (int sc = 0; sc < 7; ++sc) v += Z[(co * 7 + sc) * N7_ZP + lane];
        o[co] = (co < a.K) ? v + (a.bias ? a.bias[co] : 0.f) : 0.f;
    }
    act_dispatch(a.act, [&](auto act_c) {
#pragma unroll
        for (int co = 0; co < 3; ++co) if (co < a.K) o[co] = act_apply_c<decltype(act_c)::value>(o[co], a.leak);
    });
    if (y < a.Ho && x < a.Wo) {
        const size_t pix = ((size_t)n * a.Ho + y) * a.Wo + x;
        if (a.dst_f32) {
            reinterpret_cast<f32x4*>(a.dst)[pix] = (f32x4){o[0], o[1], o[2], 0.f};
        } else {
            u32x4 pk = zero16();
            const bf16 b0 = (bf16)o[0], b1 = (bf16)o[1], b2 = (bf16)o[2];
            pk[0] = (uint32_t)__builtin_bit_cast(uint16_t, b0) | ((uint32_t)__builtin_bit_cast(uint16_t, b1) << 16);
            pk[1] = (uint32_t)__builtin_bit_cast(uint16_t, b2);
            st16(reinterpret_cast<char*>(a.dst) + pix * 16, pk);
        }
    }
  }
}

// MirrorPadGrad for REFLECT pad 3 (tf.pad backward in front of the stem, module.py:230): dxp is the data gradient on the
// PADDED grid (N, H+6, W+6, 4) f32; every image pixel sums its (up to 2 x 2) mirror pre-images in fixed order and is
// rounded to bf16 once.
// addend (nullable, (N,H,W,8) bf16 like dx): added before the one rounding (a gradient join folded into the store).
__global__ __launch_bounds__(256) void pad3_fold_kernel(const f32x4* dxp, const char* addend, char* dx, int N, int H, int W) {
    const int64_t total = (int64_t)N * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const int64_t t = i / W;
        const int h = (int)(t % H), n = (int)(t / H);
        int jh[3], jw[3];
        const int nh = reflect_preimages(h, H, 3, jh), nw = reflect_preimages(w, W, 3, jw);
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        for (int ih = 0; ih < nh; ++ih)
            for (int iw = 0; iw < nw; ++iw) {
                const f32x4 d = dxp[((size_t)n * (H + 6) + jh[ih]) * (W + 6) + jw[iw]];
                v0 += d[0]; v1 += d[1]; v2 += d[2];
            }
        if (addend) {
            const bf16x4 ad = *reinterpret_cast<const bf16x4*>(addend + (size_t)i * 16);
            v0 += (float)ad[0]; v1 += (float)ad[1]; v2 += (float)ad[2];
        }
        u32x4 pk = zero16();
        const bf16 b0 = (bf16)v0, b1 = (bf16)v1, b2 = (bf16)v2;
        pk[0] = (uint32_t)__builtin_bit_cast(uint16_t, b0) | ((uint32_t)__builtin_bit_cast(uint16_t, b1) << 16);
        pk[1] = (uint32_t)__builtin_bit_cast(uint16_t, b2);
        st16(dx + (size_t)i * 16, pk);
    }
}

// head forward: 7x7 stride 1, 64 -> <= 3 channels (stored in 8), bf16, same-size output
// -------------------------------------------------------------------------------------------------
// Data gradient of the discriminator's first conv (module.py:284: 3x3, stride 2, SAME, 3(8) -> 64 channels): dx has 8 channels,
// dy 64.  As an implicit GEMM (conv_gemm_glds_kernel<DGRAD, 256x16>) the layer ran at 11 TFLOP/s, 162 us for both discriminators'
// 16 images -- all of it gather overhead: the work is 0.45 GMAC against 50 MB of traffic (~10 us).  Here a wave owns two dx rows
// (2m, 2m+1) x 32 columns (both column parities of 16 column pairs j): with even H, W (TF 'SAME' pads bottom / right only) the
// stride-2 taps that reach them are
//     row 2m  : r = 0 from dy row m,  r = 2 from dy row m-1        column 2j  : s = 0 from dy column j,  s = 2 from column j-1
//     row 2m+1: r = 1 from dy row m                                 column 2j+1: s = 1 from dy column j
// i.e. four fragments of 16 dy pixels (rows m-1 / m, columns j-1.. / j..), loaded straight from global memory in the MFMA operand
// layout (a pixel's 64 channels are the reduction: 2 k-steps), feed 9 tap products: D[channel][pixel] += W_tap[channel][k] dy[k][pixel].
// The 9 x 2 weight fragments stay in registers while a wave walks its share of the work items.  No LDS, no barrier.
// Two networks on one stacked batch: images >= nsplit take w2.
// -------------------------------------------------------------------------------------------------
struct S2NArgs {
    const char* dy;      // (N,Ho,Wo,64) bf16
    const char* w;       // w_dgrad [8][9*64] bf16 (rows = dx channels)
    const char* w2;
    char* dx;            // (N,H,W,8) bf16
    const char* addend;  // nullable, like dx: added to the result before its one rounding (a gradient join folded into the store)
    int N, nsplit, H, W, Ho, Wo, items, items_per_wave;
};

template <bool ADD>
__global__ __launch_bounds__(256) void conv3x3s2_narrow_dgrad_kernel(S2NArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int frow = lane & 15, fq = lane >> 4;
    const int gw = blockIdx.x * 4 + wave;
    const int it0 = gw * a.items_per_wave, it1 = min(a.items, it0 + a.items_per_wave);
    const int jblocks = (a.Wo + 15) >> 4, mrows = a.Ho;
    int cur_net = -1;
    u32x4 wr[9][2];
    for (int it = it0; it < it1; ++it) {
        int b = it;
        const int jb = b % jblocks; b /= jblocks;
        const int m = b % mrows;
        const int n = b / mrows;
        const int net = n >= a.nsplit ? 1 : 0;
        if (net != cur_net) {                               // (a wave's items are consecutive: at most one switch)
            cur_net = net;
            const char* wm = net ? a.w2 : a.w;
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    wr[t][kk] = frow < 8 ? ld16(wm + (((size_t)frow * 9 + t) * 64 + kk * 32 + fq * 8) * 2) : zero16();
        }
        // dy fragments: [row m-1 / m][column shift -1 / 0][k-step]
        u32x4 fy[2][2][2];
        const int j = jb * 16 + frow;
#pragma unroll
        for (int ry = 0; ry < 2; ++ry)
#pragma unroll
            for (int sx = 0; sx < 2; ++sx) {
                const int yo = m - 1 + ry, xo = j - 1 + sx;
                const bool ok = yo >= 0 && (unsigned)xo < (unsigned)a.Wo;
                const char* src = a.dy + ((((size_t)n * a.Ho + (ok ? yo : 0)) * a.Wo + (ok ? xo : 0)) * 64 + fq * 8) * 2;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) fy[ry][sx][kk] = ok ? ld16(src + kk * 64) : zero16();
            }
        f32x4 acc[2][2];                                    // [dx row parity][dx column parity]
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) acc[py][px] = (f32x4){0.f, 0.f, 0.f, 0.f};
        auto mac = [&](int py, int px, int r, int sx_tap, int ry, int sx) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                acc[py][px] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wr[r * 3 + sx_tap][kk]),
                                                                      __builtin_bit_cast(bf16x8, fy[ry][sx][kk]), acc[py][px], 0, 0, 0);
        };
        // (dx row parity, dx column parity) <- tap (r, s) from fragment (dy row m-1+ry, column shift sx); fixed order
        mac(0, 0, 0, 0, 1, 1); mac(0, 0, 0, 2, 1, 0); mac(0, 0, 2, 0, 0, 1); mac(0, 0, 2, 2, 0, 0);
        mac(0, 1, 0, 1, 1, 1); mac(0, 1, 2, 1, 0, 1);
        mac(1, 0, 1, 0, 1, 1); mac(1, 0, 1, 2, 1, 0);
        mac(1, 1, 1, 1, 1, 1);
        // D[channel = 4 fq + e][pixel = frow]: lanes fq < 2 hold the 8 channels of column pair j
        if (fq < 2 && j < a.Wo) {
            bf16x4 ad[2][2];
            if (ADD) {
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 2; ++px)
                        ad[py][px] = *reinterpret_cast<const bf16x4*>(a.addend + ((((size_t)n * a.H + 2 * m + py) * a.W + 2 * j + px) * 8 + fq * 4) * 2);
            }
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    f32x4 v = acc[py][px];
                    if (ADD) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += (float)ad[py][px][e];
                    }
                    const bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                    *reinterpret_cast<bf16x4*>(a.dx + ((((size_t)n * a.H + 2 * m + py) * a.W + 2 * j + px) * 8 + fq * 4) * 2) = pk;
                }
        }
    }
}

static bool s2n_dgrad_ok(const sgg_conv_desc* d) {
    return d->dtype == SGG_BF16 && d->pad_mode == SGG_PAD_ZERO && d->R == 3 && d->S == 3 && d->stride == 2 && d->C == 8 && d->K == 64 &&
           d->pad_t == 0 && d->pad_l == 0 && d->H == 2 * d->Ho && d->W == 2 * d->Wo;
}
static int launch_s2n_dgrad(const sgg_conv_desc* d, const void* dy, const void* w, const void* w2, int nsplit, const void* addend, void* dx, hipStream_t s) {
    S2NArgs q;
    q.dy = (const char*)dy; q.w = (const char*)w; q.w2 = (const char*)(w2 ? w2 : w); q.dx = (char*)dx; q.addend = (const char*)addend;
    q.N = d->N; q.nsplit = w2 ? nsplit : d->N; q.H = d->H; q.W = d->W; q.Ho = d->Ho; q.Wo = d->Wo;
    q.items = d->N * d->Ho * ((d->Wo + 15) / 16);
    const int waves = 256 * 16;                          // 16 waves per CU, each walking a contiguous run of items
    q.items_per_wave = (q.items + waves - 1) / waves;
    const int blocks = ((q.items + q.items_per_wave - 1) / q.items_per_wave + 3) / 4;
    if (addend) hipLaunchKernelGGL(conv3x3s2_narrow_dgrad_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, q);
    else hipLaunchKernelGGL(conv3x3s2_narrow_dgrad_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, q);
    return sgg_check_launch();
}

// conv7_narrow_out_kernel runs the head's forward (conv7_head_ok) and the stem's data gradient (conv7_stem_ok): as a conv over
// dy that is the head's shape with mirrored taps, on the padded grid (f32, folded onto the image by pad3_fold_kernel)
static size_t n7_dgrad_ws(const sgg_conv_desc* d) { return (size_t)d->N * (d->H + 6) * (d->W + 6) * 16; }

static int launch_n7(const N7Args& a, hipStream_t s) {
    SGG_LDS_ATTR(conv7_narrow_out_kernel, N7_LDS);
    const int64_t tiles = (int64_t)a.N * ((a.Ho + N7_TH - 1) / N7_TH) * ((a.Wo + N7_TW - 1) / N7_TW);
    const int64_t per = (tiles + 255) / 256;            // persistent blocks, one per CU, equal tile counts
    const int64_t blocks = (tiles + per - 1) / per;
    hipLaunchKernelGGL(conv7_narrow_out_kernel, dim3((unsigned)blocks), dim3(512), N7_LDS, s, a);
    return sgg_check_launch();
}

static bool halo_fwd_ok(const sgg_conv_desc* d) {
    const int cch = d->dtype == SGG_BF16 ? 64 : 32;
    return d->K <= 16 && d->stride == 1 && d->R <= HALO_MAXR && d->S <= HALO_MAXR && d->Ho == d->H && d->Wo == d->W &&
           d->H % HALO_TH == 0 && d->W % HALO_TW == 0 && d->C % cch == 0;
}

template <typename T>
static int launch_halo_fwd_t(const sgg_conv_desc* d, const ConvArgs& a, int flip, hipStream_t s) {
    size_t lds = 2 * (size_t)HALO_MAXR * 16 * 128 + (size_t)(HALO_TH + d->R - 1) * (HALO_TW + d->S - 1) * 128 + 1024;
    auto kern = conv_halo_fwd_kernel<T>;
    SGG_LDS_ATTR(kern, 160 * 1024);
    dim3 grid((unsigned)(d->N * (d->H / HALO_TH) * (d->W / HALO_TW)));
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, a, flip);
    return sgg_check_launch();
}

// data gradient of a narrow-INPUT conv (the stem, 3->64 7x7; cycle mode back-propagates into the fake image): as a
// convolution over dy it is the head's shape (64 -> <= 16 channels), so it runs conv_halo_fwd_kernel with mirrored taps
// and zero padding; REFLECT's MirrorPadGrad terms are then added to the border pixels by launch_border
static bool halo_dgrad_narrow_ok(const sgg_conv_desc* d) {
    const int en = sgg_config().stem_dgrad_halo;
    const int cch = d->dtype == SGG_BF16 ? 64 : 32;
    return en && d->C <= 16 && d->stride == 1 && d->R <= HALO_MAXR && d->S <= HALO_MAXR && d->R == d->S &&
           d->Ho == d->H && d->Wo == d->W && d->pad_t == (d->R - 1) / 2 && d->pad_l == (d->S - 1) / 2 &&
           d->H % HALO_TH == 0 && d->W % HALO_TW == 0 && d->K % cch == 0;
}

// Narrow-INPUT convolution (8 source channels = one 16-byte chunk per pixel, 64 output channels, stride 1, same-size):
// the generator stem 7x7 3(8)->64 forward (module.py:230-232) and the data-gradient of the head 7x7 64->3(8).  As an
// implicit GEMM every (pixel, tap) is a separate 16-byte DMA element; here the source halo of a 16x32 tile (13 KB) and
// the whole weight matrix (64 x 49*8, 53 KB) sit in LDS, each lane picks the chunk of ITS tap out of the halo, and
// persistent blocks amortise the weight load.  flip = data-gradient (taps mirrored, zero fill).
template <typename T>
__global__ __launch_bounds__(512) void conv_halo_narrow_in_kernel(ConvArgs a, int ntiles, int flip) {
    constexpr int VEC = ET<T>::VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int SCH = 8;                              // source channels
    constexpr int CPV = SCH / VEC;                      // 16-byte chunks per (pixel, tap): 1 bf16, 2 f32
    constexpr int PXB = SCH * ES;                       // bytes per halo pixel
    constexpr int DCH = 64;                             // destination channels
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int taps = a.R * a.S;
    const int kch = taps * CPV;                         // real 16-byte chunks per weight row
    const int ksteps = (kch + 3) / 4;
    const int wpitch = ((ksteps * 4) | 1) * 16;         // odd chunk count per row: conflict-free fragment reads
    char* sW = smem;                                    // [64][wpitch]
    char* sH = smem + DCH * wpitch;                     // halo [(TH+R-1)*(TW+S-1)][PXB]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int HWd = HALO_TW + a.S - 1, HHd = HALO_TH + a.R - 1, HP = HHd * HWd;
    const int tilesW = a.W / HALO_TW, tilesH = a.H / HALO_TH;
    const int frow = lane & 15, fq = lane >> 4;

    // weights: rows = destination channels, zero beyond the real K
    for (int idx = tid; idx < DCH * ksteps * 4; idx += 512) {
        int row = idx / (ksteps * 4), ch = idx - row * (ksteps * 4);
        u32x4 v = zero16();
        if (ch < kch) v = ld16(a.wmat + ((size_t)row * taps * SCH) * ES + ch * 16);
        st16(sW + row * wpitch + ch * 16, v);
    }
    // origin of the source halo relative to the tile: fwd reads (y - p + r), the data-gradient (y + p - r)
    const int oy = flip ? a.pad_t - (a.R - 1) : -a.pad_t, ox = flip ? a.pad_l - (a.S - 1) : -a.pad_l;
    // per 16-byte k-chunk q: byte offset of its tap inside the halo, ((tr * HWd + ts) * PXB + sub * 16); chunks past the last
    // tap read tap 0 (their weights are zero)
    int* sTap = reinterpret_cast<int*>(sH + (size_t)HP * PXB);
    float* sS = reinterpret_cast<float*>(sTap + ksteps * 4);      // [8 waves][64 channels][2]: norm-statistics epilogue (a.stats)
    for (int q = tid; q < ksteps * 4; q += 512) {
        int tap = q / CPV, sub = q - tap * CPV;
        if (tap >= taps) { tap = 0; sub = 0; }
        int tr = tap / a.S, ts = tap - tr * a.S;
        if (flip) { tr = a.R - 1 - tr; ts = a.S - 1 - ts; }
        sTap[q] = (tr * HWd + ts) * PXB + sub * 16;
    }

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int b = tile;
        const int tw = b % tilesW; b /= tilesW;
        const int th = b % tilesH;
        const int n = b / tilesH;
        const int y0 = th * HALO_TH, x0 = tw * HALO_TW;
        __syncthreads();                                // previous tile's halo reads are done; weights are visible
        for (int idx = tid; idx < HP * CPV; idx += 512) {
            int hp = idx / CPV, sub = idx - hp * CPV;
            int hy = hp / HWd, hx = hp - hy * HWd;
            int yi = y0 + oy + hy, xi = x0 + ox + hx;
            bool ok = true;
            if (a.reflect && !flip) {
                yi = yi < 0 ? -yi : (yi >= a.H ? 2 * (a.H - 1) - yi : yi);
                xi = xi < 0 ? -xi : (xi >= a.W ? 2 * (a.W - 1) - xi : xi);
            } else ok = (unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W;
            u32x4 v = zero16();
            if (ok) v = ld16(a.src + (((size_t)n * a.H + yi) * a.W + xi) * PXB + sub * 16);
            st16(sH + hp * PXB + sub * 16, v);
        }
        __syncthreads();

        f32x4 acc[4][4];                                // [cout frag][pixel frag]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < ksteps; ++ks) {
            const int qq = ks * 4 + fq;                  // this lane's 16-byte k-chunk
            // halo byte offset of this lane's tap (tr, ts, sub): a table built once per block (the two integer divisions and the
            // flip per k-step and lane made this loop VALU-issue bound: PMC showed the matrix pipes 34 % busy, 44 % of wave cycles
            // issue-stalled)
            const int toff = sTap[qq];
            u32x4 fw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fw[i] = ld16(sW + (i * 16 + frow) * wpitch + qq * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = 2 * wave + (j >> 1), x = (j & 1) * 16 + frow;
                u32x4 fp = ld16(sH + (y * HWd + x) * PXB + toff);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (sizeof(T) == 2) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fw[i]), __builtin_bit_cast(bf16x8, fp), acc[i][j], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(fw[i][e]), __uint_as_float(fp[e]), acc[i][j], 0, 0, 0);
                    }
                }
            }
        }
        float bv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[i][e] = a.bias ? a.bias[i * 16 + fq * 4 + e] : 0.f;
        act_dispatch(a.act, [&](auto act_c) {
            constexpr int ACT = decltype(act_c)::value;
            if constexpr (sizeof(T) == 2) {
                // 16-byte stores (the two 16-column fragments of a tile row trade halves between lane rows, see conv3x3_halo_gemm_kernel) and,
                // with a.stats, the (sum, sumsq) rows of the stored output for the instance norm behind the stem (module.py:230-233):
                // wave butterfly -> the eight waves' rows through LDS -> ONE partial row per (image, 16 x 32 tile)
                auto ep = [&](auto st_c) {
                    constexpr bool ST = decltype(st_c)::value;
                    const int jo = fq & 1, cb = (fq >> 1) * 8;
                    float s1[4][4], s2[4][4];
                    if constexpr (ST) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int e = 0; e < 4; ++e) s1[i][e] = s2[i][e] = 0.f;
                    }
#pragma unroll
                    for (int jp = 0; jp < 2; ++jp) {
                        const int y = y0 + 2 * wave + jp, x = x0 + jo * 16 + frow;
                        const size_t dpix = ((size_t)n * a.H + y) * a.W + x;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float v0[4], v1[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v0[e] = act_apply_c<ACT>(acc[i][2 * jp][e] + bv[i][e], a.leak);
                                v1[e] = act_apply_c<ACT>(acc[i][2 * jp + 1][e] + bv[i][e], a.leak);
                            }
                            const bf16x4 p0 = {(bf16)v0[0], (bf16)v0[1], (bf16)v0[2], (bf16)v0[3]}, p1 = {(bf16)v1[0], (bf16)v1[1], (bf16)v1[2], (bf16)v1[3]};
                            if constexpr (ST) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) { const float r0 = (float)p0[e]; s1[i][e] += r0; s2[i][e] += r0 * r0; }
#pragma unroll
                                for (int e = 0; e < 4; ++e) { const float r1 = (float)p1[e]; s1[i][e] += r1; s2[i][e] += r1 * r1; }
                            }
                            st16(reinterpret_cast<bf16*>(a.dst) + dpix * DCH + i * 16 + cb, row_swap16_pack(p0, p1));
                        }
                    }
                    if constexpr (ST) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
#pragma unroll
                                for (int off = 1; off < 16; off <<= 1) {
                                    s1[i][e] += __shfl_xor(s1[i][e], off);
                                    s2[i][e] += __shfl_xor(s2[i][e], off);
                                }
                            }
                        if (frow == 0) {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    float* o = sS + (wave * 64 + i * 16 + fq * 4 + e) * 2;
                                    o[0] = s1[i][e]; o[1] = s2[i][e];
                                }
                        }
                        __syncthreads();
                        if (tid < 128) {
                            const int ch = tid >> 1, which = tid & 1;
                            float t = 0.f;
#pragma unroll
                            for (int w8 = 0; w8 < 8; ++w8) t += sS[(w8 * 64 + ch) * 2 + which];
                            a.stats[(((size_t)n * (tilesH * tilesW) + th * tilesW + tw) * DCH + ch) * 2 + which] = t;
                        }
                        // (the next tile's rows are written behind the two barriers at the head of its loop iteration)
                    }
                };
                if (a.stats) ep(std::true_type{}); else ep(std::false_type{});
                return;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int y = y0 + 2 * wave + (j >> 1), x = x0 + (j & 1) * 16 + frow;
                const size_t dpix = ((size_t)n * a.H + y) * a.W + x;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int dc = i * 16 + fq * 4;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_apply_c<ACT>(acc[i][j][e] + bv[i][e], a.leak);
                    T* o = reinterpret_cast<T*>(a.dst) + dpix * DCH + dc;
                    if constexpr (sizeof(T) == 2) {
                        bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                        *reinterpret_cast<bf16x4*>(o) = pk;
                    } else *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
                }
            }
        });
    }
}

// src_ch / dst_ch: channel counts of the gathered tensor and of the result for the direction in question
static bool halo_narrow_in_ok(const sgg_conv_desc* d, int src_ch, int dst_ch) {
    return src_ch == 8 && dst_ch == 64 && d->stride == 1 && d->R <= HALO_MAXR && d->S <= HALO_MAXR &&
           d->Ho == d->H && d->Wo == d->W && d->H % HALO_TH == 0 && d->W % HALO_TW == 0;
}

template <typename T>
static int launch_halo_narrow_in_t(const sgg_conv_desc* d, const ConvArgs& a, int flip, hipStream_t s) {
    const int cpv = 8 / (16 / (int)sizeof(T));
    const int ksteps = (d->R * d->S * cpv + 3) / 4;
    size_t lds = (size_t)64 * (((ksteps * 4) | 1) * 16) + (size_t)(HALO_TH + d->R - 1) * (HALO_TW + d->S - 1) * 8 * sizeof(T)
                 + (size_t)ksteps * 4 * sizeof(int)                        // + the tap-offset table
                 + (size_t)8 * 64 * 2 * sizeof(float);                     // + the statistics epilogue's per-wave rows
    auto kern = conv_halo_narrow_in_kernel<T>;
    SGG_LDS_ATTR(kern, 160 * 1024);
    int ntiles = d->N * (d->H / HALO_TH) * (d->W / HALO_TW);
    int blocks = ntiles < 512 ? ntiles : 512;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), lds, s, a, ntiles, flip);
    return sgg_check_launch();
}

// Side tensor for the REFLECT data-gradient: for every border pixel (the pixels MirrorPadGrad adds mirrored terms
// to) and every tap, the gather row the GEMM needs = sum of dy over all preimages of the pixel's padded position.
// fold[b][tap][k], b enumerating border pixels per image: the 2p border ROW bands first (all columns), then the
// 2p border COLUMNS of the remaining rows (or every pixel when the bands overlap).
__host__ __device__ inline int fold_border_per_image(int H, int W, int p) {
    int p2 = 2 * p;
    return (H <= p2 + 1 || W <= p2 + 1) ? H * W : p2 * W + (H - p2) * p2;
}

template <typename T>
__global__ __launch_bounds__(256) void fold_gather_kernel(const char* dy, char* fold, int N, int H, int W, int K, int R, int S, int p, int Ho, int Wo) {
    constexpr int VEC = ET<T>::VEC;
    const int cpv = K / VEC, taps = R * S, p2 = 2 * p;
    const bool all = H <= p2 + 1 || W <= p2 + 1;
    const int Bimg = fold_border_per_image(H, W, p);
    const int64_t total = (int64_t)N * Bimg * taps * cpv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int ch = (int)(i % cpv);
        int64_t t = i / cpv;
        int tap = (int)(t % taps);
        int b = (int)(t / taps);
        int n = b / Bimg, q = b - n * Bimg, h, w;
        if (all) { h = q / W; w = q - h * W; }
        else if (q < p2 * W) { int hi = q / W; w = q - hi * W; h = hi < p ? 1 + hi : H - 1 - p + (hi - p); }
        else {
            q -= p2 * W;
            int hh = q / p2, wi = q - hh * p2;
            h = hh == 0 ? 0 : (hh == H - p2 - 1 ? H - 1 : p + hh);
            w = wi < p ? 1 + wi : W - 1 - p + (wi - p);
        }
        int r = tap / S, s = tap - r * S;
        int jh[3], jw[3];
        int nh = reflect_preimages(h, H, p, jh), nw = reflect_preimages(w, W, p, jw);
        float acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
        for (int ia = 0; ia < nh; ++ia)
            for (int ib = 0; ib < nw; ++ib) {
                int ho = jh[ia] - r, wo = jw[ib] - s;
                if ((unsigned)ho < (unsigned)Ho && (unsigned)wo < (unsigned)Wo) {
                    float v[VEC];
                    ET<T>::unpack(ld16(dy + ((((size_t)n * Ho + ho) * Wo + wo) * K + (size_t)ch * VEC) * sizeof(T)), v);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[e] += v[e];
                }
            }
        st16(fold + (size_t)i * 16, ET<T>::pack(acc));
    }
}

// HWIO f32 -> [Kpad][R*S*Cpad] and [Cpad][R*S*Kpad] in dtype T, zero padded
template <typename T>
__global__ void pack_weights_kernel(const float* w, int taps, int C, int K, int Cpad, int Kpad, T* wf, T* wd) {
    int64_t total = (int64_t)taps * Cpad * Kpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int k = (int)(i % Kpad);
        int64_t t = i / Kpad;
        int c = (int)(t % Cpad), tap = (int)(t / Cpad);
        float v = (c < C && k < K) ? w[((size_t)tap * C + c) * K + k] : 0.f;
        if (wf) wf[((size_t)k * taps + tap) * Cpad + c] = (T)v;
        if (wd) wd[((size_t)c * taps + tap) * Kpad + k] = (T)v;
    }
}

// every conv layer of a network in ONE launch (blockIdx.y = layer): after each optimizer step all packed weights are stale,
// and 16 separate 8-us launches per network were pure launch latency.  SCALED: every element of item i times scale[i] in f32 before
// the one rounding to T (sgg_pack_conv_weights_batch_scaled: a spectrally normalised network packs W / sigma)
template <typename T, bool SCALED>
__global__ __launch_bounds__(256) void pack_weights_batch_kernel(const sgg_pack_item* items, const float* scale) {
    // (tap, 64 c, 64 k) tiles: w[tap][c][k] is read along k, w_dgrad[c][tap][k] written along k, and w_fwd[k][tap][c] -- the
    // transposed layout -- written along c out of an LDS tile.  (One thread per element wrote w_fwd as 2-byte scatters, one
    // cache line per lane: 83 us for a generator's 11.4 M parameters, 1.1 TB/s.)
    __shared__ float tile[64][65];
    const sgg_pack_item it = items[blockIdx.y];
    const int taps = it.taps, C = it.C, K = it.K, Cpad = it.Cpad, Kpad = it.Kpad;
    const float* w = it.w;
    T* wf = (T*)it.w_fwd;
    T* wd = (T*)it.w_dgrad;
    float sc = 1.f;
    if constexpr (SCALED) sc = scale[blockIdx.y];
    const int tc = (Cpad + 63) / 64, tk = (Kpad + 63) / 64;
    const int ntiles = taps * tc * tk;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int kt = t % tk, ct = (t / tk) % tc, tap = t / (tk * tc);
        const int k = kt * 64 + lx;
        for (int cy = ly; cy < 64; cy += 4) {
            const int c = ct * 64 + cy;
            float v = (c < C && k < K) ? w[((size_t)tap * C + c) * K + k] : 0.f;
            if constexpr (SCALED) v = v * sc;
            tile[cy][lx] = v;
            if (wd && c < Cpad && k < Kpad) wd[((size_t)c * taps + tap) * Kpad + k] = (T)v;
        }
        __syncthreads();
        if (wf) {
            const int c = ct * 64 + lx;
            for (int ky = ly; ky < 64; ky += 4) {
                const int kk = kt * 64 + ky;
                if (c < Cpad && kk < Kpad) wf[((size_t)kk * taps + tap) * Cpad + c] = (T)tile[lx][ky];
            }
        }
        __syncthreads();
    }
}

static bool desc_ok(const sgg_conv_desc* d) {
    if (!d) return false;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->R <= 0 || d->S <= 0) return false;
    if (d->C <= 0 || d->K <= 0 || d->C % SGG_CPAD || d->K % SGG_CPAD) return false;
    if (d->stride != 1 && d->stride != 2) return false;
    if (d->dtype != SGG_F32 && d->dtype != SGG_BF16) return false;
    if (d->pad_mode == SGG_PAD_REFLECT) {
        if (d->stride != 1 || d->pad_t != d->pad_l || d->pad_t >= d->H || d->pad_t >= d->W) return false;
        if (d->Ho != d->H + 2 * d->pad_t - d->R + 1 || d->Wo != d->W + 2 * d->pad_l - d->S + 1) return false;
    } else if (d->pad_mode != SGG_PAD_ZERO) return false;
    if (d->pad_t < 0 || d->pad_l < 0) return false;
    // every output window must start inside the (leading-)padded input
    if ((int64_t)(d->Ho - 1) * d->stride - d->pad_t >= d->H || (int64_t)(d->Wo - 1) * d->stride - d->pad_l >= d->W) return false;
    if ((int64_t)d->N * d->H * d->W >= (1ll << 31) / 2 || (int64_t)d->N * d->Ho * d->Wo >= (1ll << 31) / 2) return false;
    return true;
}

// REFLECT data gradient behind a main launch that padded with zeros: add the mirrored terms to the border pixels of dx
// (conv_border_fold_kernel); few pixels and short K loops, hence the small tiles
template <typename T>
static int launch_border_t(const ConvArgs& a, hipStream_t s) {
    const int64_t M = (int64_t)a.N * fold_border_per_image(a.H, a.W, a.pad_t);
    const unsigned mtiles = (unsigned)((M + 63) / 64);
    if (a.C > 16) {
        hipLaunchKernelGGL((conv_border_fold_kernel<T, 64, 2>), dim3(mtiles, (unsigned)((a.C + 63) / 64)), dim3(256), (64 + 64) * 128, s, a);
    } else {
        hipLaunchKernelGGL((conv_border_fold_kernel<T, 16, 4>), dim3(mtiles, 1), dim3(256), (64 + 16) * 128, s, a);
    }
    return sgg_check_launch();
}
static int launch_border(const sgg_conv_desc* d, const ConvArgs& a, hipStream_t s) {
    // The kernel enumerates the border as disjoint row and column bands, which needs H, W > 2p + 1.  Both callers tile the image
    // 16 x 32 at the same output size, where desc_ok's REFLECT rule leaves p = (R - 1) / 2 <= 3: a smaller image never gets here.
    if (a.H <= 2 * a.pad_t + 1 || a.W <= 2 * a.pad_t + 1) return SGG_EUNSUPPORTED;
    return d->dtype == SGG_BF16 ? launch_border_t<bf16>(a, s) : launch_border_t<float>(a, s);
}

// out[p][c] = act(sum_s partial[s][p][c] + bias[c])  (fixed order -> deterministic)
struct SplitKGroup { const float* bias2; size_t net_part, net_dst, net_add; };   // second group of a grouped launch (blockIdx.y == 1)
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* partial, const float* bias, const char* addend, char* out, int64_t nvec4,
                                                            int DC, int ksplit, size_t slab, int act, float leak, SplitKGroup g2) {
    if (blockIdx.y) {
        partial = reinterpret_cast<const float*>(reinterpret_cast<const char*>(partial) + g2.net_part);
        bias = g2.bias2; out += g2.net_dst;
        if (addend) addend += g2.net_add;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 s4 = *reinterpret_cast<const f32x4*>(partial + i * 4);
        for (int sp = 1; sp < ksplit; ++sp) s4 += *reinterpret_cast<const f32x4*>(partial + sp * slab + i * 4);
        int c = (int)((i * 4) % DC);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s4[e] + (bias ? bias[c + e] : 0.f);
        act_dispatch(act, [&](auto act_c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act_apply_c<decltype(act_c)::value>(v[e], leak);
        });
        if (addend) {
            const T* ad = reinterpret_cast<const T*>(addend) + i * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)ad[e];
        }
        if constexpr (sizeof(T) == 2) {
            bf16x4 pk = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
            *reinterpret_cast<bf16x4*>(out + i * 8) = pk;
        } else *reinterpret_cast<f32x4*>(out + i * 16) = (f32x4){v[0], v[1], v[2], v[3]};
    }
}

// split-K factor for layers whose output is too small to fill the chip (D's tail: 5x13..15x31 maps, K = 4608)
static int conv_ksplit(int64_t Mmax, int DC, int classes, int ktot_max) {
    int64_t bm = 128, bn = DC >= 128 ? 128 : (DC > 16 ? 64 : 16);
    int64_t blocks = ((Mmax + bm - 1) / bm) * ((DC + bn - 1) / bn) * classes;
    if (blocks >= 192 || ktot_max < 16) return 1;
    int64_t ks = (256 + blocks - 1) / blocks;
    if (ks > ktot_max / 4) ks = ktot_max / 4;
    if (ks > 16) ks = 16;
    return ks < 2 ? 1 : (int)ks;
}

template <typename T, int MODE, int BM, int BN, int WGM, int NW, int BKB = 128, int NS = 2>
static int launch_glds_cfg(const ConvArgs& a, int64_t Mmax, int DC, int classes, hipStream_t s) {
    constexpr int RPP = NW * (64 / (BKB / 16));
    constexpr size_t lds = (size_t)NS * (size_t)(BM + (BN + RPP - 1) / RPP * RPP) * BKB;
    auto kern = conv_gemm_glds_kernel<T, MODE, BM, BN, WGM, NW, BKB, NS>;
    SGG_LDS_ATTR(kern, (int)lds);
    const int64_t tilesN = (DC + BN - 1) / BN;
    int64_t blocks = (Mmax + BM - 1) / BM * tilesN;
    dim3 grid((unsigned)blocks, (unsigned)a.ksplit, (unsigned)(classes * a.grp));
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), lds, s, a);
    return sgg_check_launch();
}

// -------------------------------------------------------------------------------------------------
// The launch layer of the forward and the data gradient.  plan_conv() states every decision about a call once: the kernel, the
// split, the workspace, how a grouped call runs and which fused forms the shape has (the table is in DESIGN.md section 3).
// run_conv() validates a ConvCall, asks the plan, checks the workspace and launches; the 15 launch exports fill a ConvCall,
// the 12 queries return fields of the plan.  (The weight gradients have their own plan, plan_wgrad in conv_wgrad.hip.)

// The generic GEMM's block tile for `DC` result channels and `Mmax` rows per parity class (an sgg_route)
static int glds_route(const sgg_conv_desc* d, int dir, int DC, int64_t Mmax) {
    // big square tiles (8 waves, 1 block per CU) when there is enough work to fill the chip with them
    // (a 4-stage ring of 64-byte K-slices was measured 3-5 % slower on the residual conv and is not built)
    if (DC >= 256 && Mmax * ((DC + 255) / 256) >= 256 * 160) return SGG_ROUTE_GLDS_256x256;
    // short reductions (<= 16 K-tiles: the 64-channel stride-2 layers c2 forward / d2 data gradient / D.h1 forward): a
    // 256x128 block is alone on its CU and spends a third of its life in prologue and epilogue; two 128x128 blocks per
    // CU cover each other: 93.7 -> 84.4 us (c2), 25.3 -> 22.7 us (D.h1); the 4-wave 128x64 tile (three blocks): 115 us
    if (DC >= 128 && (dir == MODE_FWD ? d->R * d->S * d->C : d->R * d->S * d->K) <= 1024) return SGG_ROUTE_GLDS_128x128;
    if (DC >= 128 && Mmax * ((DC + 127) / 128) >= 256 * 160) return SGG_ROUTE_GLDS_256x128;
    // 128x128 with 8 waves (2 per SIMD, two blocks per CU): the 4-wave variant ran at one wave per SIMD with
    // nothing to cover its LDS latencies (D.h3 data gradient 86 -> 60 us, D.h2 forward 36 -> 23 us)
    if (DC >= 128) return SGG_ROUTE_GLDS_128x128;
    if (DC > 16) return SGG_ROUTE_GLDS_128x64;
    return SGG_ROUTE_GLDS_256x16;
}

// Kernels taken AHEAD of the GEMM planner by the conv entries (an sgg_route), 0: the GEMM planner decides.  A transposed conv
// takes none.  stats: the call emits statistics rows -- forward (sum, sumsq), data gradient the norm-backward sums
static int conv_fwd_head_route(const sgg_conv_desc* d, bool stats) {
    if (halo_narrow_in_ok(d, d->C, d->K)) return SGG_ROUTE_HALO_NARROW_IN;   // narrow input (stem): halo + whole weight matrix resident in LDS
    if (stats) return 0;                                           // (the other two have no statistics epilogue)
    if (conv7_head_ok(d)) return SGG_ROUTE_N7;                     // the 7x7 head: (channel, tap column) in the GEMM N dimension
    if (halo_fwd_ok(d)) return SGG_ROUTE_HALO_FWD;                 // narrow output at full resolution: input halo resident in LDS
    return 0;
}
// addend: a skip gradient is joined in the epilogue
static int conv_dgrad_head_route(const sgg_conv_desc* d, bool addend, bool stats) {
    if (!addend && halo_narrow_in_ok(d, d->K, d->C)) return SGG_ROUTE_HALO_NARROW_IN;   // data-gradient of a narrow-OUTPUT conv (the head): dy has 8 channels
    if (!stats && s2n_dgrad_ok(d)) return SGG_ROUTE_S2N;
    if (!stats && conv7_stem_ok(d)) return SGG_ROUTE_N7;         // (addend: joined in the fold pass, before its one rounding)
    if (!addend && halo_dgrad_narrow_ok(d)) return SGG_ROUTE_HALO_DGRAD_NARROW;
    return 0;
}

static size_t fold_bytes(const sgg_conv_desc* d) {
    if (d->pad_mode != SGG_PAD_REFLECT) return 0;
    size_t es = d->dtype == SGG_BF16 ? 2 : 4;
    return align_up((size_t)d->N * fold_border_per_image(d->H, d->W, d->pad_t) * d->R * d->S * d->K * es, 256);
}

// How a grouped call (two networks' call sites of one shape, sgg_*_group2) runs
enum {
    GROUP_ONE_LAUNCH = 0,    // the generic GEMM with grp = 2: the grid's z dimension doubles, each group is exactly the single launch
    GROUP_STACKED,           // a kernel that picks the weights per image (HALO3, S2HALO, S2N): the single launch on 2N images, split at N
    GROUP_TWO_CALLS          // the head routes and the REFLECT data gradient (its fold tensor is per call): two single calls
};

struct ConvPlan {
    int route;               // the kernel a call runs (an sgg_route): a head route, or the GEMM planner's with the SGG_ROUTE_SPLITK bit
    int gemm;                // the GEMM planner's route for the shape: == route unless a head route is taken ahead of it
    int DC, classes, ksplit; // result channels, parity classes and split factor (1: none) of the GEMM
    int64_t Mmax;            // its rows per class
    size_t pdst;             // destination pixels (slab stride)
    size_t fold_bytes;       // workspace, first part: the pre-folded gather rows of a REFLECT data gradient on the GEMM
    size_t splitk_bytes;     //            second part: the split-K slabs
    size_t ws_bytes;         // what a single call on `route` needs; a grouped call: twice that
    int group;               // GROUP_*
    // the fused forms of this direction
    size_t stats_chunks;     // statistics rows per image (0: no such epilogue)
    bool mixed, pair, normload;
};

// dir: the GEMM direction the call runs.  deconv: a transposed conv (it plans the opposite direction of the equivalent conv and
// takes no head route).  addend, stats: see the head routes.
static ConvPlan plan_conv(const sgg_conv_desc* d, int dir, bool addend, bool stats, bool deconv = false) {
    ConvPlan p{};
    const int vec = d->dtype == SGG_BF16 ? 8 : 4, st = d->stride;
    int ktot_max;
    if (dir == MODE_FWD) {
        p.DC = d->K; p.classes = 1; p.Mmax = (int64_t)d->N * d->Ho * d->Wo; p.pdst = (size_t)p.Mmax;
        ktot_max = (d->R * d->S * (d->C / vec) + 7) / 8;
    } else {
        p.DC = d->C; p.classes = st * st;
        p.Mmax = (int64_t)d->N * ((d->H + st - 1) / st) * ((d->W + st - 1) / st);
        p.pdst = (size_t)d->N * d->H * d->W;
        ktot_max = (((d->R + st - 1) / st) * ((d->S + st - 1) / st) * (d->K / vec) + 7) / 8;
    }
    // shapes the halo-resident kernels take are never split (they only occur at sizes that fill the chip; it also
    // keeps the small parity-test shapes on the same kernels as the full-size layers)
    const bool s2 = dir == MODE_DGRAD && s2halo_ok(d), h3 = halo3_ok(d, dir);
    p.ksplit = (s2 || h3) ? 1 : conv_ksplit(p.Mmax, p.DC, p.classes, ktot_max);
    p.gemm = (s2 ? SGG_ROUTE_S2HALO : h3 ? SGG_ROUTE_HALO3 : glds_route(d, dir, p.DC, p.Mmax)) | (p.ksplit > 1 ? SGG_ROUTE_SPLITK : 0);
    const int head = deconv ? 0 : dir == MODE_FWD ? conv_fwd_head_route(d, stats) : conv_dgrad_head_route(d, addend, stats);
    p.route = head ? head : p.gemm;
    p.fold_bytes = dir == MODE_DGRAD ? fold_bytes(d) : 0;
    p.splitk_bytes = p.ksplit > 1 ? (size_t)p.ksplit * p.pdst * p.DC * sizeof(float) : 0;
    p.ws_bytes = !head ? p.fold_bytes + p.splitk_bytes : (head == SGG_ROUTE_N7 && dir == MODE_DGRAD) ? n7_dgrad_ws(d) : 0;
    p.group = head == SGG_ROUTE_S2N ? GROUP_STACKED : (head || p.fold_bytes) ? GROUP_TWO_CALLS : (s2 || h3) ? GROUP_STACKED : GROUP_ONE_LAUNCH;
    // The forms hang on the GEMM planner's kernel, also where a head route runs the plain call of the shape.  (A 3x3 layer of
    // <= 16 channels and 128 | W has both HALO_DGRAD_NARROW and these forms; no network has such a layer.)
    if (deconv) {
        if (s2) p.stats_chunks = (size_t)(d->Ho / S2_TI) * (d->Wo / S2_TJ);   // a row per 16 x 64 output tile (deconv_s2_stats_kernel)
    } else if (head == SGG_ROUTE_HALO_NARROW_IN && dir == MODE_FWD) {
        if (d->dtype == SGG_BF16) p.stats_chunks = (size_t)(d->H / HALO_TH) * (d->W / HALO_TW);   // the stem: a row per 16 x 32 tile
    } else if (h3) p.stats_chunks = halo3_stats_chunks(d);           // a row per (2 x 128 tile, tile row)
    p.mixed = h3 && dir == MODE_DGRAD;
    p.pair = d->N >= 2 && (deconv ? s2 : halo3_ok(d, MODE_FWD) && halo3_ok(d, MODE_DGRAD));
    p.normload = h3 && dir == MODE_FWD && d->pad_mode == SGG_PAD_REFLECT && d->C <= halo3_norm_maxc();
    return p;
}
// What the *_workspace queries report.  They do not know the operands, and an addend moves a head shape's data gradient to the
// GEMM, so a shape whose head route needs no workspace reports the GEMM's.
static size_t plan_ws_query(const ConvPlan& p) {
    return p.route == SGG_ROUTE_N7 && p.ws_bytes ? p.ws_bytes : p.fold_bytes + p.splitk_bytes;
}

// One call of any of the 15 entries.  `form` says which operands below are required and which epilogue is wanted.
enum {
    FORM_STATS = 1,          // stats: (sum, sumsq) rows of the stored output
    FORM_NORM_BWD = 2,       // stats: the norm-backward sums of the data gradient, from nx / nstats / ngamma / nbeta / nact / nleak
    FORM_MIXED = 4,          // data gradient: dst is f32, and so is the addend when addend_f32
    FORM_PAIR = 8,           // a stacked batch of two networks: images >= nsplit use w2 / bias2 (/ ngamma2 / nbeta2)
    FORM_NORMLOAD = 16,      // forward: src is raw, relu(instnorm(src)) from nstats / ngamma / nbeta is applied on load and written to nout
    FORM_GROUP = 32,         // sgg_*_group2: d is ONE network's call, the tensors hold 2N images, the second network uses w2 / bias2
    FORM_DECONV = 64         // a transposed conv
};
struct ConvCall {
    int form;
    const void* src; const void* w; const float* bias; void* dst; const void* addend;
    int act; float leak;
    const void* w2; const float* bias2; int nsplit;
    float* stats;
    const void* nx; const float* nstats; const float* ngamma; const float* nbeta; int nact; float nleak;
    void* nout; const float* ngamma2; const float* nbeta2;
    int addend_f32;
    void* ws; size_t ws_bytes; void* stream;
};
static ConvCall conv_call(int form, const void* src, const void* w, const float* bias, void* dst, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c{};
    c.form = form; c.src = src; c.w = w; c.bias = bias; c.dst = dst; c.act = SGG_ACT_NONE; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
    return c;
}
static void conv_call_pair(ConvCall& c, const void* w2, const float* bias2, int nsplit) {
    c.w2 = w2; c.bias2 = bias2; c.nsplit = nsplit;
}

static bool conv_call_ok(const sgg_conv_desc* d, const ConvCall& c) {
    const int f = c.form;
    if (!desc_ok(d) || ((f & FORM_DECONV) && d->pad_mode != SGG_PAD_ZERO)) return false;
    if (!c.src || !c.w || !c.dst) return false;
    if ((f & (FORM_STATS | FORM_NORM_BWD)) && !c.stats) return false;
    if ((f & FORM_NORM_BWD) && (!c.nx || !c.nstats || !c.ngamma || !c.nbeta)) return false;
    if ((f & FORM_NORMLOAD) && (!c.nstats || !c.ngamma || !c.nbeta || !c.nout || (c.w2 && (!c.ngamma2 || !c.nbeta2)))) return false;
    if ((f & (FORM_PAIR | FORM_GROUP)) && !c.w2) return false;
    if ((f & FORM_PAIR) && (c.nsplit <= 0 || c.nsplit >= d->N)) return false;
    return true;
}

static ConvArgs make_args(const sgg_conv_desc* d, const ConvCall& c) {
    ConvArgs a;
    a.src = (const char*)c.src; a.wmat = (const char*)c.w; a.bias = c.bias; a.dst = (char*)c.dst; a.addend = (const char*)c.addend; a.fold = nullptr;
    a.stats = c.stats; a.nx = (const char*)c.nx; a.nstats = c.nstats; a.ngamma = c.ngamma; a.nbeta = c.nbeta; a.nact = c.nact; a.nleak = c.nleak;
    a.nout = (char*)c.nout; a.ngamma2 = c.ngamma2; a.nbeta2 = c.nbeta2;
    a.partial = nullptr; a.ksplit = 1; a.pdst = 0;
    a.wmat2 = (const char*)c.w2; a.bias2 = c.bias2; a.nsplit = 0x7fffffff;
    a.grp = 1; a.net_src = a.net_dst = a.net_add = a.net_part = 0;
    a.dst_f32 = (c.form & FORM_MIXED) != 0; a.addend_f32 = c.addend_f32;
    a.ablate = sgg_config().ablate;
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.K = d->K; a.R = d->R; a.S = d->S; a.stride = d->stride;
    a.pad_t = d->pad_t; a.pad_l = d->pad_l; a.Ho = d->Ho; a.Wo = d->Wo; a.reflect = d->pad_mode == SGG_PAD_REFLECT;
    a.act = c.act; a.leak = c.leak;
    return a;
}

// conv7_narrow_out_kernel's arguments: the head's forward, or the stem's data gradient on the PADDED grid (a zero-padded "full"
// correlation of dy with the mirrored taps, f32, into ws)
static N7Args n7_args(const sgg_conv_desc* d, int dir, const ConvCall& c) {
    const bool fwd = dir == MODE_FWD;
    N7Args q;
    q.src = (const char*)c.src; q.wmat = (const char*)c.w; q.bias = fwd ? c.bias : nullptr; q.dst = fwd ? c.dst : c.ws;
    q.N = d->N; q.H = d->H; q.W = d->W; q.Ho = fwd ? d->Ho : d->H + 6; q.Wo = fwd ? d->Wo : d->W + 6; q.pt = q.pl = fwd ? 3 : 6; q.K = 3;
    q.reflect = fwd && d->pad_mode == SGG_PAD_REFLECT; q.flip = !fwd; q.act = fwd ? c.act : SGG_ACT_NONE; q.leak = fwd ? c.leak : 0.f; q.dst_f32 = !fwd;
    return q;
}

// ---- one dtype switch per kernel family
static int launch_halo_narrow_in(const sgg_conv_desc* d, const ConvArgs& a, int flip, hipStream_t s) {
    return d->dtype == SGG_BF16 ? launch_halo_narrow_in_t<bf16>(d, a, flip, s) : launch_halo_narrow_in_t<float>(d, a, flip, s);
}
static int launch_halo_fwd(const sgg_conv_desc* d, const ConvArgs& a, int flip, hipStream_t s) {
    return d->dtype == SGG_BF16 ? launch_halo_fwd_t<bf16>(d, a, flip, s) : launch_halo_fwd_t<float>(d, a, flip, s);
}
template <typename T, int MODE>
static int launch_glds(const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
    switch (p.gemm & ~SGG_ROUTE_SPLITK) {
    case SGG_ROUTE_GLDS_256x256:
        return launch_glds_cfg<T, MODE, 256, 256, 2, 8, 128, 2>(a, p.Mmax, p.DC, p.classes, s);
    case SGG_ROUTE_GLDS_256x128:
        // three LDS stages (48 KB each): its layers (c2 forward, d2 data gradient, D.h1 forward) gather their pixel operand from HBM
        // with 9 short K-tiles per block; two tiles in flight instead of one: 96.8 -> 93.4 us (c2), 26.4 -> 25.3 us (D.h1)
        return launch_glds_cfg<T, MODE, 256, 128, 4, 8, 128, 3>(a, p.Mmax, p.DC, p.classes, s);
    case SGG_ROUTE_GLDS_128x128:
        return launch_glds_cfg<T, MODE, 128, 128, 2, 8>(a, p.Mmax, p.DC, p.classes, s);
    case SGG_ROUTE_GLDS_128x64:
        return launch_glds_cfg<T, MODE, 128, 64, 4, 4>(a, p.Mmax, p.DC, p.classes, s);
    case SGG_ROUTE_GLDS_256x16:
        return launch_glds_cfg<T, MODE, 256, 16, 4, 4>(a, p.Mmax, p.DC, p.classes, s);
    default: return SGG_EUNSUPPORTED;                    // (plan_conv names no other GEMM route)
    }
}
// the GEMM planner's kernel
static int launch_gemm(const sgg_conv_desc* d, int dir, const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
    if (p.gemm == SGG_ROUTE_S2HALO) return launch_s2halo(a, s);
    if (p.gemm == SGG_ROUTE_HALO3) return launch_halo3(a, dir, s);
    if (d->dtype == SGG_BF16) return dir == MODE_FWD ? launch_glds<bf16, MODE_FWD>(a, p, s) : launch_glds<bf16, MODE_DGRAD>(a, p, s);
    return dir == MODE_FWD ? launch_glds<float, MODE_FWD>(a, p, s) : launch_glds<float, MODE_DGRAD>(a, p, s);
}
// the side tensor of a REFLECT data gradient on the GEMM: the gather rows of the border pixels, pre-folded, which ONE GEMM
// launch then reads like any other source (the LDS-resident 3x3 kernel reads a smaller one of its own layout)
static int launch_fold_gather(const sgg_conv_desc* d, const ConvPlan& p, const void* dy, void* fold, hipStream_t s) {
    const size_t es = d->dtype == SGG_BF16 ? 2 : 4;
    const bool halo3 = p.gemm == SGG_ROUTE_HALO3;
    const int64_t total = halo3 ? ((int64_t)d->N * d->H * 18 + (int64_t)d->N * 2 * d->W) * d->K * es / 16
                                : (int64_t)d->N * fold_border_per_image(d->H, d->W, d->pad_t) * d->R * d->S * d->K * es / 16;
    int blocks = (int)((total + 255) / 256); if (blocks > 8192) blocks = 8192;
    if (halo3) hipLaunchKernelGGL(fold_halo_gather_kernel<bf16>, dim3(blocks), dim3(256), 0, s, (const char*)dy, (char*)fold, d->N, d->H, d->W, d->K);
    else if (d->dtype == SGG_BF16) hipLaunchKernelGGL(fold_gather_kernel<bf16>, dim3(blocks), dim3(256), 0, s, (const char*)dy, (char*)fold, d->N, d->H, d->W, d->K, d->R, d->S, d->pad_t, d->Ho, d->Wo);
    else hipLaunchKernelGGL(fold_gather_kernel<float>, dim3(blocks), dim3(256), 0, s, (const char*)dy, (char*)fold, d->N, d->H, d->W, d->K, d->R, d->S, d->pad_t, d->Ho, d->Wo);
    return sgg_check_launch();
}
static int launch_splitk_reduce(const sgg_conv_desc* d, const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
    const int64_t nvec4 = (int64_t)p.pdst * p.DC / 4;
    int blocks = (int)((nvec4 + 255) / 256); if (blocks > 2048) blocks = 2048;
    const SplitKGroup g2{a.bias2, a.net_part, a.net_dst, a.net_add};
    if (d->dtype == SGG_BF16) hipLaunchKernelGGL(splitk_reduce_kernel<bf16>, dim3(blocks, a.grp), dim3(256), 0, s, (const float*)a.partial, a.bias, a.addend, a.dst, nvec4, p.DC, p.ksplit, p.pdst * p.DC, a.act, a.leak, g2);
    else hipLaunchKernelGGL(splitk_reduce_kernel<float>, dim3(blocks, a.grp), dim3(256), 0, s, (const float*)a.partial, a.bias, a.addend, a.dst, nvec4, p.DC, p.ksplit, p.pdst * p.DC, a.act, a.leak, g2);
    return sgg_check_launch();
}

// Every conv launch entry.  Before anything is launched, in this order: SGG_EINVAL (descriptor, required pointers, nsplit),
// SGG_EUNSUPPORTED (the shape or dtype has no such form), SGG_EWORKSPACE (ws is NULL or shorter than the plan's total).
static int run_conv(const sgg_conv_desc* d, int dir, const ConvCall& c) {
    const int f = c.form;
    if (!conv_call_ok(d, c)) return SGG_EINVAL;
    const ConvPlan p = plan_conv(d, dir, c.addend != nullptr, (f & (FORM_STATS | FORM_NORM_BWD)) != 0, (f & FORM_DECONV) != 0);
    if ((f & FORM_NORM_BWD) && c.nact == SGG_ACT_TANH) return SGG_EUNSUPPORTED;
    if (((f & (FORM_STATS | FORM_NORM_BWD)) && !p.stats_chunks) || ((f & FORM_MIXED) && !p.mixed) || ((f & FORM_PAIR) && !p.pair) ||
        ((f & FORM_NORMLOAD) && !p.normload)) return SGG_EUNSUPPORTED;
    const bool group = (f & FORM_GROUP) != 0;
    const size_t need = p.ws_bytes * (group ? 2 : 1);
    if (need && (!c.ws || c.ws_bytes < need)) return SGG_EWORKSPACE;
    hipStream_t s = (hipStream_t)c.stream;

    // the second network of a grouped call reads / writes at these byte offsets (dir DGRAD: src is the conv's output side)
    const size_t es = d->dtype == SGG_BF16 ? 2 : 4;
    const size_t in_bytes = (size_t)d->N * d->H * d->W * d->C * es, out_bytes = (size_t)d->N * d->Ho * d->Wo * d->K * es;
    const size_t net_src = dir == MODE_FWD ? in_bytes : out_bytes, net_dst = dir == MODE_FWD ? out_bytes : in_bytes;
    if (group && p.group == GROUP_TWO_CALLS) {
        ConvCall one = c;
        one.form = f & ~FORM_GROUP;
        conv_call_pair(one, nullptr, nullptr, 0);
        const int rc = run_conv(d, dir, one);
        if (rc) return rc;
        one.src = (const char*)c.src + net_src; one.w = c.w2; one.bias = c.bias2; one.dst = (char*)c.dst + net_dst;
        if (c.addend) one.addend = (const char*)c.addend + net_dst;
        return run_conv(d, dir, one);
    }
    const bool stacked = group && p.group == GROUP_STACKED;
    sgg_conv_desc ds = *d;
    if (stacked) ds.N = 2 * d->N;
    ConvArgs a = make_args(&ds, c);
    if (stacked) a.nsplit = d->N;
    else if (group) { a.grp = 2; a.net_src = net_src; a.net_dst = a.net_add = net_dst; }
    else if (c.w2) a.nsplit = c.nsplit;

    switch (p.route) {
    case SGG_ROUTE_HALO_NARROW_IN:                       // forward of a narrow-INPUT conv (the stem), data gradient of a narrow-OUTPUT one (the head)
    case SGG_ROUTE_HALO_DGRAD_NARROW: {
        int rc;
        if (p.route == SGG_ROUTE_HALO_NARROW_IN) rc = launch_halo_narrow_in(d, a, dir == MODE_DGRAD, s);
        else {
            ConvArgs h = a;                              // the same computation written as a forward conv over dy
            h.C = d->K; h.K = d->C; h.reflect = 0;
            rc = launch_halo_fwd(d, h, 1, s);
        }
        if (rc || dir == MODE_FWD || !a.reflect) return rc;
        return launch_border(d, a, s);                   // REFLECT: + the mirrored (MirrorPadGrad) terms of the border pixels
    }
    case SGG_ROUTE_S2N:                                  // (D.h0; a grouped call: the stacked batch, weights picked per image)
        return launch_s2n_dgrad(&ds, c.src, c.w, stacked ? c.w2 : nullptr, d->N, c.addend, c.dst, s);
    case SGG_ROUTE_N7: {
        const int rc = launch_n7(n7_args(d, dir, c), s);
        if (rc || dir == MODE_FWD) return rc;
        // the stem: then MirrorPadGrad as a fold of the 3-pixel frame onto the image (the addend joins here) -- one rounding, no separate border GEMM
        const int64_t total = (int64_t)d->N * d->H * d->W;
        int blocks = (int)((total + 255) / 256); if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(pad3_fold_kernel, dim3(blocks), dim3(256), 0, s, (const f32x4*)c.ws, (const char*)c.addend, (char*)c.dst, d->N, d->H, d->W);
        return sgg_check_launch();
    }
    case SGG_ROUTE_HALO_FWD: return launch_halo_fwd(d, a, 0, s);
    default: break;                                      // the GEMM planner's kernel
    }
    if (p.fold_bytes) {
        const int rc = launch_fold_gather(d, p, c.src, c.ws, s);
        if (rc) return rc;
        a.fold = (const char*)c.ws;
    }
    if (p.ksplit > 1) { a.ksplit = p.ksplit; a.partial = (float*)((char*)c.ws + p.fold_bytes); a.pdst = p.pdst; a.net_part = p.splitk_bytes; }
    const int rc = launch_gemm(d, dir, a, p, s);
    if (rc || p.ksplit <= 1) return rc;
    return launch_splitk_reduce(d, a, p, s);             // out = act(sum of the slabs + bias) + addend, in a fixed order
}

// every conv layer of a network in one launch, plain or scaled per item
template <bool SCALED>
static int launch_pack_batch(const sgg_pack_item* items_dev, const float* scale_dev, int n_items, int64_t max_elems, int dtype, void* stream) {
    if (!items_dev || n_items <= 0 || max_elems <= 0 || (SCALED && !scale_dev)) return SGG_EINVAL;
    int blocks = (int)((max_elems + 4095) / 4096); if (blocks > 1024) blocks = 1024;     // 64 x 64 tiles, grid-strided
    dim3 grid((unsigned)blocks, (unsigned)n_items);
    if (dtype == SGG_BF16) hipLaunchKernelGGL((pack_weights_batch_kernel<bf16, SCALED>), grid, dim3(256), 0, (hipStream_t)stream, items_dev, scale_dev);
    else if (dtype == SGG_F32) hipLaunchKernelGGL((pack_weights_batch_kernel<float, SCALED>), grid, dim3(256), 0, (hipStream_t)stream, items_dev, scale_dev);
    else return SGG_EINVAL;
    return sgg_check_launch();
}

extern "C" {

#ifdef SGG_LAB

// debug aid (not part of include/sggan.h): occupancy the runtime reports for the hot kernels
int sgg_debug_occupancy(int* out, int cap) {
    int n = 0, v = 0;
    if (cap < 3) return SGG_EINVAL;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, conv_gemm_glds_kernel<bf16, MODE_FWD, 256, 256, 2, 8, 128, 2>, 512, 131072); out[n++] = v;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, conv_gemm_glds_kernel<bf16, MODE_DGRAD, 256, 256, 2, 8, 128, 2>, 512, 131072); out[n++] = v;
    out[n++] = wgrad_debug_occupancy();                  // conv_wgrad_kernel<bf16, 128, 128, 2>, asked where the kernel is built
    return n;
}
#endif  // SGG_LAB

int sgg_pack_conv_weights(const float* w, int R, int S, int C, int K, int Cpad, int Kpad, int dtype, void* wf, void* wd, void* stream) {
    if (!w || R <= 0 || S <= 0 || C <= 0 || K <= 0 || Cpad < C || Kpad < K || Cpad % SGG_CPAD || Kpad % SGG_CPAD) return SGG_EINVAL;
    int64_t total = (int64_t)R * S * Cpad * Kpad;
    int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
    if (dtype == SGG_BF16) hipLaunchKernelGGL(pack_weights_kernel<bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, R * S, C, K, Cpad, Kpad, (bf16*)wf, (bf16*)wd);
    else if (dtype == SGG_F32) hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, R * S, C, K, Cpad, Kpad, (float*)wf, (float*)wd);
    else return SGG_EINVAL;
    return sgg_check_launch();
}

int sgg_pack_conv_weights_batch(const sgg_pack_item* items_dev, int n_items, int64_t max_elems, int dtype, void* stream) {
    return launch_pack_batch<false>(items_dev, nullptr, n_items, max_elems, dtype, stream);
}

int sgg_pack_conv_weights_batch_scaled(const sgg_pack_item* items_dev, const float* scale_dev, int n_items, int64_t max_elems, int dtype, void* stream) {
    return launch_pack_batch<true>(items_dev, scale_dev, n_items, max_elems, dtype, stream);
}

// ---- the queries: fields of the plan (0 / SGG_EINVAL for a descriptor the library rejects)
static inline bool deconv_desc_ok(const sgg_conv_desc* d) { return desc_ok(d) && d->pad_mode == SGG_PAD_ZERO; }

size_t sgg_conv2d_fwd_workspace(const sgg_conv_desc* d) { return desc_ok(d) ? plan_ws_query(plan_conv(d, MODE_FWD, false, false)) : 0; }
size_t sgg_conv2d_bwd_data_workspace(const sgg_conv_desc* d) { return desc_ok(d) ? plan_ws_query(plan_conv(d, MODE_DGRAD, false, false)) : 0; }
// a transposed conv runs the conv's data-gradient GEMM forwards and its forward GEMM backwards, without the conv entry points' head routes
size_t sgg_deconv2d_fwd_workspace(const sgg_conv_desc* d) { return desc_ok(d) ? plan_conv(d, MODE_DGRAD, false, false, true).splitk_bytes : 0; }
size_t sgg_deconv2d_bwd_data_workspace(const sgg_conv_desc* d) { return desc_ok(d) ? plan_conv(d, MODE_FWD, false, false, true).splitk_bytes : 0; }

int sgg_conv2d_route(const sgg_conv_desc* d, int op) {
    if (!desc_ok(d) || op < 0 || op > 2) return SGG_EINVAL;
    if (op == 2) return wgrad_route(d);      // C_real <= 4 assumed where it matters (S2N), see include/sggan.h
    return plan_conv(d, op == 0 ? MODE_FWD : MODE_DGRAD, false, false).route;
}
int sgg_deconv2d_route(const sgg_conv_desc* d, int op) {
    if (!deconv_desc_ok(d) || op < 0 || op > 2) return SGG_EINVAL;
    if (op == 2) return wgrad_route(d);      // C_real <= 4 assumed where it matters (S2N), see include/sggan.h
    return plan_conv(d, op == 0 ? MODE_DGRAD : MODE_FWD, false, false, true).route;
}

// Pixel chunks per image of the statistics rows the *_stats entries emit; 0 = this shape has no such epilogue
size_t sgg_conv2d_fwd_stats_chunks(const sgg_conv_desc* d) { return desc_ok(d) ? plan_conv(d, MODE_FWD, false, true).stats_chunks : 0; }
size_t sgg_conv2d_bwd_data_stats_chunks(const sgg_conv_desc* d) { return desc_ok(d) ? plan_conv(d, MODE_DGRAD, false, true).stats_chunks : 0; }
size_t sgg_deconv2d_fwd_stats_chunks(const sgg_conv_desc* d) { return deconv_desc_ok(d) ? plan_conv(d, MODE_DGRAD, false, true, true).stats_chunks : 0; }

int sgg_conv2d_bwd_data_mixed_supported(const sgg_conv_desc* d) { return desc_ok(d) && plan_conv(d, MODE_DGRAD, false, false).mixed; }
int sgg_conv2d_pair_supported(const sgg_conv_desc* d) { return desc_ok(d) && plan_conv(d, MODE_FWD, false, true).pair; }
int sgg_conv2d_fwd_normload_supported(const sgg_conv_desc* d) { return desc_ok(d) && plan_conv(d, MODE_FWD, false, true).normload; }

// ---- the launch entries: each fills a ConvCall
int sgg_conv2d_fwd(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, void* y, int act, float leak,
                   void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(0, x, w, bias, y, ws, ws_bytes, stream);
    c.act = act; c.leak = leak;
    return run_conv(d, MODE_FWD, c);
}

int sgg_conv2d_fwd_stats(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, void* y, float* partial,
                         void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_STATS, x, w, bias, y, ws, ws_bytes, stream);
    c.stats = partial;
    return run_conv(d, MODE_FWD, c);
}

// Two networks of one shape on a stacked batch (images >= nsplit use the second weight set): one launch of the LDS-resident
// 3x3 kernels instead of two -- 512 blocks, so a CU's second block loads its halo while the first one's stores drain.
int sgg_conv2d_fwd_stats_pair(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, const void* w2, const float* bias2,
                              int nsplit, void* y, float* partial, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_STATS | FORM_PAIR, x, w, bias, y, ws, ws_bytes, stream);
    c.stats = partial;
    conv_call_pair(c, w2, bias2, nsplit);
    return run_conv(d, MODE_FWD, c);
}

// "Normalise on load": conv(relu(instnorm(x_raw))) without the norm's apply pass -- x_raw is the previous conv's raw output,
// x_stats its (mean, rstd) (sgg_instnorm_finalize), and the normalised tensor comes out in x_norm as a by-product.
int sgg_conv2d_fwd_stats_normload(const sgg_conv_desc* d, const void* x_raw, const float* x_stats, const float* x_gamma, const float* x_beta,
                                  const float* x_gamma2, const float* x_beta2, void* x_norm, const void* w, const float* bias,
                                  const void* w2, const float* bias2, int nsplit, void* y, float* partial,
                                  void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_STATS | FORM_NORMLOAD | (w2 ? FORM_PAIR : 0), x_raw, w, bias, y, ws, ws_bytes, stream);
    c.stats = partial; c.nstats = x_stats; c.ngamma = x_gamma; c.nbeta = x_beta; c.nout = x_norm;
    if (w2) { conv_call_pair(c, w2, bias2, nsplit); c.ngamma2 = x_gamma2; c.nbeta2 = x_beta2; }
    return run_conv(d, MODE_FWD, c);
}

int sgg_conv2d_bwd_data(const sgg_conv_desc* d, const void* dy, const void* w, const void* addend, void* dx, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(0, dy, w, nullptr, dx, ws, ws_bytes, stream);
    c.addend = addend;
    return run_conv(d, MODE_DGRAD, c);
}

// Mixed-precision data gradient (bf16 operands, f32 result): only the LDS-resident 3x3 halo GEMM has the epilogue
int sgg_conv2d_bwd_data_mixed(const sgg_conv_desc* d, const void* dy, const void* w, const void* addend, int addend_is_f32, float* dx,
                              void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_MIXED, dy, w, nullptr, dx, ws, ws_bytes, stream);
    c.addend = addend; c.addend_f32 = addend_is_f32 ? 1 : 0;
    return run_conv(d, MODE_DGRAD, c);
}

int sgg_conv2d_bwd_data_stats(const sgg_conv_desc* d, const void* dy, const void* w, const void* addend, void* dx,
                              const void* norm_x, const float* norm_stats, const float* norm_gamma, const float* norm_beta,
                              int norm_act, float norm_leak, float* partial, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_NORM_BWD, dy, w, nullptr, dx, ws, ws_bytes, stream);
    c.addend = addend; c.stats = partial;
    c.nx = norm_x; c.nstats = norm_stats; c.ngamma = norm_gamma; c.nbeta = norm_beta; c.nact = norm_act; c.nleak = norm_leak;
    return run_conv(d, MODE_DGRAD, c);
}

int sgg_conv2d_bwd_data_pair(const sgg_conv_desc* d, const void* dy, const void* w, const void* w2, int nsplit, const void* addend, void* dx,
                             void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_PAIR, dy, w, nullptr, dx, ws, ws_bytes, stream);
    c.addend = addend;
    conv_call_pair(c, w2, nullptr, nsplit);
    return run_conv(d, MODE_DGRAD, c);
}

// ---- grouped launches: the same call site of TWO networks of one architecture (G_A->B beside G_B->A, D_A beside D_B).  `d`
// describes ONE network's call (N images); x / y (dy / dx, addend) hold 2N images, the first network's first; the result is
// exactly that of two single calls (bit for bit: each group runs the single call's tiles and split-K).  How it runs is the
// plan's `group`; ws >= 2 x the single call's workspace.
int sgg_conv2d_fwd_group2(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, const void* w2, const float* bias2,
                          void* y, int act, float leak, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_GROUP, x, w, bias, y, ws, ws_bytes, stream);
    c.act = act; c.leak = leak;
    conv_call_pair(c, w2, bias2, 0);
    return run_conv(d, MODE_FWD, c);
}
int sgg_conv2d_bwd_data_group2(const sgg_conv_desc* d, const void* dy, const void* w, const void* w2, const void* addend, void* dx,
                               void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_GROUP, dy, w, nullptr, dx, ws, ws_bytes, stream);
    c.addend = addend;
    conv_call_pair(c, w2, nullptr, 0);
    return run_conv(d, MODE_DGRAD, c);
}

// ---- Conv2DTranspose: `d` is the equivalent forward conv; x: (N,Ho,Wo,K), y: (N,H,W,C)
int sgg_deconv2d_fwd(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, void* y, int act, float leak,
                     void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_DECONV, x, w, bias, y, ws, ws_bytes, stream);
    c.act = act; c.leak = leak;
    return run_conv(d, MODE_DGRAD, c);
}
// ... that also emits the per-chunk (sum, sumsq) rows of its stored output for the instance norm behind it (module.py:254-260):
// one row per (image, 16 x 64 output-pixel tile) of the stride-2 halo kernel, from deconv_s2_stats_kernel.  w2: a stacked batch.
int sgg_deconv2d_fwd_stats(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, const void* w2, const float* bias2, int nsplit,
                           void* y, float* partial, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_DECONV | FORM_STATS | (w2 ? FORM_PAIR : 0), x, w, bias, y, ws, ws_bytes, stream);
    c.stats = partial;
    if (w2) conv_call_pair(c, w2, bias2, nsplit);
    return run_conv(d, MODE_DGRAD, c);
}
int sgg_deconv2d_fwd_group2(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, const void* w2, const float* bias2,
                            void* y, int act, float leak, void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_DECONV | FORM_GROUP, x, w, bias, y, ws, ws_bytes, stream);
    c.act = act; c.leak = leak;
    conv_call_pair(c, w2, bias2, 0);
    return run_conv(d, MODE_DGRAD, c);
}
int sgg_deconv2d_bwd_data(const sgg_conv_desc* d, const void* dy, const void* w, void* dx, void* ws, size_t ws_bytes, void* stream) {
    return run_conv(d, MODE_FWD, conv_call(FORM_DECONV, dy, w, nullptr, dx, ws, ws_bytes, stream));
}
int sgg_deconv2d_bwd_data_group2(const sgg_conv_desc* d, const void* dy, const void* w, const void* w2, void* dx,
                                 void* ws, size_t ws_bytes, void* stream) {
    ConvCall c = conv_call(FORM_DECONV | FORM_GROUP, dy, w, nullptr, dx, ws, ws_bytes, stream);
    conv_call_pair(c, w2, nullptr, 0);
    return run_conv(d, MODE_FWD, c);
}

// ---- the weight gradients (conv_wgrad.hip)
static inline size_t tensor_bytes(const sgg_conv_desc* d, bool out_side) {
    const size_t es = d->dtype == SGG_BF16 ? 2 : 4;
    return out_side ? (size_t)d->N * d->Ho * d->Wo * d->K * es : (size_t)d->N * d->H * d->W * d->C * es;
}

size_t sgg_conv2d_bwd_weight_workspace(const sgg_conv_desc* d) {
    return desc_ok(d) ? wgrad_ws_bytes(d) : 0;
}

int sgg_conv2d_bwd_weight(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    if (!desc_ok(d) || !x || !dy || !dw || Cr <= 0 || Kr <= 0 || Cr > d->C || Kr > d->K) return SGG_EINVAL;
    return run_wgrad(d, x, dy, dw, Cr, Kr, accumulate, ws, ws_bytes, (hipStream_t)stream);
}

// Grouped call (see sgg_conv2d_fwd_group2): x / dy hold 2N images, the first network's first; dw / dw2 are the two networks' gradients.
int sgg_conv2d_bwd_weight_group2(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, float* dw2, int Cr, int Kr, int accumulate,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (!desc_ok(d) || !x || !dy || !dw || !dw2 || Cr <= 0 || Kr <= 0 || Cr > d->C || Kr > d->K) return SGG_EINVAL;
    const char* xb = (const char*)x + tensor_bytes(d, false);
    const char* dyb = (const char*)dy + tensor_bytes(d, true);
    return run_wgrad(d, x, dy, dw, Cr, Kr, accumulate, ws, ws_bytes, (hipStream_t)stream, xb, dyb, dw2);
}

// Weight gradient of TWO applications of one layer (same shape) in one launch: dw (+)= wgrad(x0, dy0) + wgrad(x1, dy1).
// Only the shapes of the all-taps 3x3 kernel (SGG_EUNSUPPORTED otherwise: call sgg_conv2d_bwd_weight twice);
// workspace as for a single call.
int sgg_conv2d_bwd_weight_pair_supported(const sgg_conv_desc* d) { return desc_ok(d) && w9_ok(d) ? 1 : 0; }

int sgg_conv2d_bwd_weight_pair(const sgg_conv_desc* d, const void* x0, const void* dy0, const void* x1, const void* dy1, float* dw,
                               int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    if (!desc_ok(d) || !x0 || !dy0 || !x1 || !dy1 || !dw || Cr <= 0 || Kr <= 0 || Cr > d->C || Kr > d->K) return SGG_EINVAL;
    if (!w9_ok(d)) return SGG_EUNSUPPORTED;
    return run_w9(d, W9Net{x0, dy0, x1, dy1, dw}, nullptr, Cr, Kr, accumulate, ws, ws_bytes, (hipStream_t)stream);
}

// ... of TWO networks of one architecture (the cycle step's generators, each applied twice): four (x, dy) sets, two dW, one launch.
// Each network gets half the blocks, so half as many f32 slabs are written and reduced for the same work per CU; the sums differ
// from two sgg_conv2d_bwd_weight_pair calls only in f32 summation order (16 partial sums per network instead of 32).
int sgg_conv2d_bwd_weight_pair2(const sgg_conv_desc* d, const void* xa0, const void* dya0, const void* xa1, const void* dya1, float* dwa,
                                const void* xb0, const void* dyb0, const void* xb1, const void* dyb1, float* dwb,
                                int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    if (!desc_ok(d) || !xa0 || !dya0 || !xa1 || !dya1 || !dwa || !xb0 || !dyb0 || !xb1 || !dyb1 || !dwb || Cr <= 0 || Kr <= 0 || Cr > d->C || Kr > d->K)
        return SGG_EINVAL;
    if (!w9_pair2_ok(d)) return SGG_EUNSUPPORTED;
    const W9Net nb{xb0, dyb0, xb1, dyb1, dwb};
    return run_w9(d, W9Net{xa0, dya0, xa1, dya1, dwa}, &nb, Cr, Kr, accumulate, ws, ws_bytes, (hipStream_t)stream);
}

int sgg_deconv2d_bwd_weight(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    // deconv input x plays the conv-output role, deconv output-gradient dy the conv-input role
    return sgg_conv2d_bwd_weight(d, dy, x, dw, Cr, Kr, accumulate, ws, ws_bytes, stream);
}
int sgg_deconv2d_bwd_weight_group2(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, float* dw2, int Cr, int Kr, int accumulate,
                                   void* ws, size_t ws_bytes, void* stream) {
    return sgg_conv2d_bwd_weight_group2(d, dy, x, dw, dw2, Cr, Kr, accumulate, ws, ws_bytes, stream);
}

}  // extern "C"
