// conv_wgrad.hip -- the weight gradients of Conv2D / Conv2DTranspose (gen_tape/disc_tape.gradient, model.py:196-197).
//
//   conv_wgrad       dW[tap,c][k]  = sum_{pixel} x~[pixel,tap][c] * dy[pixel][k]        (reduction over pixels,
//                    operands transposed on the fly with ds_read_b64_tr_b16; split over pixel ranges into f32
//                    slabs that a second kernel sums in fixed order -> deterministic)
// A transposed conv's weight gradient is the equivalent conv's with the operand roles swapped (the entry layer swaps them).
// The kernels, each under its own heading: the generic register-staged and LDS-DMA GEMMs with their slab reducer, the narrow-output
// halo kernel, the 7x7 kernel of the two layers with a 3-channel side, the vector-ALU kernel of the 3 -> 64 stride-2 layer, the two
// all-taps 3x3 kernels.  The host layer at the end has ONE plan per descriptor (plan_wgrad: kernel, slab count, workspace) that the
// launcher, the workspace query and the route query read; conv_internal.h declares what conv.hip's entry points call.
#include "conv_internal.h"

struct WgradArgs {
    const char* x;       // (N,H,W,C)  gathered operand
    const char* dy;      // (N,Ho,Wo,K)
    float* ws;           // [splits][R*S*C][K] f32 slabs
    int N, H, W, C, K, R, S, stride, pad_t, pad_l, Ho, Wo, reflect;
    int P, pix_per_split;
    FastDiv dHW, dW;     // divide by Ho*Wo, Wo
    // conv_wgrad_glds_kernel only: two NETWORKS of one shape in one launch -- splits [splits_per_net, 2 * splits_per_net) read
    // xb / dyb over the same pixel ranges (each network gets half the blocks and half the slabs of a single call's grid)
    const char* xb; const char* dyb;
    int splits_per_net;
};

// -------------------------------------------------------------------------------------------------
// the generic kernels: any shape
// -------------------------------------------------------------------------------------------------

__device__ inline int wg_swz(int chunk, int row, int nchunks) {
    int f = (row & 3) | (((row >> 3) & 1) << 2);
    return chunk ^ ((f << 1) & (nchunks - 1));
}

template <typename T, int BMW, int BNW, int WGM>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
    constexpr int VEC = ET<T>::VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int BKP = 32;                               // pixels per K-step
    constexpr int WGN = 4 / WGM;
    constexpr int WMW = BMW / WGM, WNW = BNW / WGN;
    constexpr int MI = WMW / 16, NI = WNW / 16;
    constexpr int NCX = BMW / VEC, NCD = BNW / VEC;       // 16-byte chunks per tile row
    constexpr int RPX = 256 / NCX, RPD = 256 / NCD;       // pixel rows covered per pass
    constexpr int PX = (BKP + RPX - 1) / RPX, PD = (BKP + RPD - 1) / RPD;
    constexpr int XP = BMW * ES, DP = BNW * ES;           // row pitch (bytes)

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sX = smem;                       // [2][BKP][XP]
    char* sD = smem + 2 * BKP * XP;        // [2][BKP][DP]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int wm = wave / WGN, wn = wave % WGN;
    const int Mrows = a.R * a.S * a.C;
    const int m0 = blockIdx.x * BMW, n0 = blockIdx.y * BNW;
    const int pbeg = blockIdx.z * a.pix_per_split;
    const int pend = min(a.P, pbeg + a.pix_per_split);

    // fixed chunk column of this thread in each tile
    const int jx = tid % NCX, rx = tid / NCX;
    const int jd = tid % NCD, rd = tid / NCD;
    const int mrow = m0 + jx * VEC;
    const bool xcol_ok = mrow < Mrows;
    const int tap = xcol_ok ? mrow / a.C : 0, c0 = mrow - tap * a.C;
    const int tr = tap / a.S, ts = tap - tr * a.S;
    const bool dcol_ok = (n0 + jd * VEC) < a.K;

    u32x4 regX[PX], regD[PD];
    auto load_tile = [&](int p0) {
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            int prow = rx + i * RPX, p = p0 + prow;
            regX[i] = zero16();
            if (prow < BKP && xcol_ok && p < pend) {
                uint32_t n = fdiv((uint32_t)p, a.dHW), rem = (uint32_t)p - n * a.dHW.d;
                uint32_t ho = fdiv(rem, a.dW), wo = rem - ho * a.dW.d;
                int hi = (int)ho * a.stride - a.pad_t + tr, wi = (int)wo * a.stride - a.pad_l + ts;
                bool ok = true;
                if (a.reflect) {
                    hi = hi < 0 ? -hi : (hi >= a.H ? 2 * (a.H - 1) - hi : hi);
                    wi = wi < 0 ? -wi : (wi >= a.W ? 2 * (a.W - 1) - wi : wi);
                } else ok = (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
                if (ok) regX[i] = ld16(a.x + ((((size_t)n * a.H + hi) * a.W + wi) * a.C + c0) * ES);
            }
        }
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            int prow = rd + i * RPD, p = p0 + prow;
            regD[i] = zero16();
            if (prow < BKP && dcol_ok && p < pend)
                regD[i] = ld16(a.dy + ((size_t)p * a.K + n0 + jd * VEC) * ES);
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            int prow = rx + i * RPX;
            if (prow < BKP) st16(sX + (buf * BKP + prow) * XP + (wg_swz(jx, prow, NCX) << 4), regX[i]);
        }
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            int prow = rd + i * RPD;
            if (prow < BKP) st16(sD + (buf * BKP + prow) * DP + (wg_swz(jd, prow, NCD) << 4), regD[i]);
        }
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, u = lane & 15;
    const int ksteps = pend > pbeg ? (pend - pbeg + BKP - 1) / BKP : 0;
    if (ksteps > 0) { load_tile(pbeg); store_tile(0); }
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < ksteps) load_tile(pbeg + (ks + 1) * BKP);
        const char* bX = sX + buf * BKP * XP;
        const char* bD = sD + buf * BKP * DP;
        if constexpr (sizeof(T) == 2) {
            // transposing LDS read: 16-lane group g fetches pixels 8g..8g+7 (two 4-row blocks) x 16 columns;
            // lane u supplies row (u>>2), columns 4*(u&3)..+3 and receives column u of the 4 rows.
            const int q = u >> 2, pp = u & 3;
            bf16x8 fa[MI], fb[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                int col = wm * WMW + i * 16 + 4 * pp;          // element column in the X tile
                int ch = col >> 3, sub = (col & 7) * 2;
                int r0 = 8 * g + q, r1 = r0 + 4;
                bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4*)(bX + r0 * XP + (wg_swz(ch, r0, NCX) << 4) + sub));
                bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4*)(bX + r1 * XP + (wg_swz(ch, r1, NCX) << 4) + sub));
                fa[i] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                int col = wn * WNW + j * 16 + 4 * pp;
                int ch = col >> 3, sub = (col & 7) * 2;
                int r0 = 8 * g + q, r1 = r0 + 4;
                bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4*)(bD + r0 * DP + (wg_swz(ch, r0, NCD) << 4) + sub));
                bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4*)(bD + r1 * DP + (wg_swz(ch, r1, NCD) << 4) + sub));
                fb[j] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int s4 = 0; s4 < BKP / 4; ++s4) {
                int row = 4 * s4 + g;
                float fa[MI], fb[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    int col = wm * WMW + i * 16 + u;
                    fa[i] = *reinterpret_cast<const float*>(bX + row * XP + (wg_swz(col >> 2, row, NCX) << 4) + (col & 3) * 4);
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    int col = wn * WNW + j * 16 + u;
                    fb[j] = *reinterpret_cast<const float*>(bD + row * DP + (wg_swz(col >> 2, row, NCD) << 4) + (col & 3) * 4);
                }
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
            }
        }
        if (ks + 1 < ksteps) store_tile(buf ^ 1);
        __syncthreads();
    }

    // D[row = 4g+e -> (tap,c)][col = u -> k]
    float* slab = a.ws + (size_t)blockIdx.z * Mrows * a.K;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            int k = n0 + wn * WNW + j * 16 + u;
            if (k >= a.K) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int mr = m0 + wm * WMW + i * 16 + g * 4 + e;
                if (mr < Mrows) slab[(size_t)mr * a.K + k] = acc[i][j][e];
            }
        }
}

// -------------------------------------------------------------------------------------------------
// v2 weight gradient: 256 (tap,c rows) x 256 (couts) tiles, 8 waves, direct-to-LDS double-buffered staging.
// Same maths as conv_wgrad_kernel; the pixel-major tiles land in LDS by DMA (1 KiB per wave-instruction = whole
// tile rows), the XOR swizzle that makes the transposing reads conflict-free is applied on the source side.
// -------------------------------------------------------------------------------------------------
template <typename T> __device__ inline int wg2_key(int row) {
    if constexpr (sizeof(T) == 2) return ((row & 3) | (((row >> 3) & 1) << 2)) << 1;
    else return (row & 3) << 1;
}

// ROWFAST (Wo % BKP == 0): every K-stage lies inside one output row, so image / row / validity of the gathered x row are
// block-uniform (scalar) and a lane only resolves its column; the general path divides per lane and per pass, which
// cost ~20 us of 125 at the residual-block shape (all 8 waves do address arithmetic at the same time, MFMA pipe idle).
template <typename T, bool ROWFAST>
__global__ __launch_bounds__(512) void conv_wgrad_glds_kernel(WgradArgs a) {
    constexpr int VEC = ET<T>::VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int BT = 256;                               // tile rows (tap,c) and columns (couts)
    constexpr int BKP = sizeof(T) == 2 ? 64 : 32;         // pixels per stage
    constexpr int PITCH = BT * ES;                        // tile row pitch in bytes (512 / 1024)
    constexpr int NCH = PITCH / 16;                       // 16-byte chunks per tile row (32 / 64)
    constexpr int RPS = 512 / NCH;                        // tile rows staged per pass (16 / 8)
    constexpr int NP = BKP / RPS;                         // passes per tile (4)
    constexpr int TILE = BKP * PITCH;                     // bytes per operand tile (32 KB)
    constexpr int STAGE = 2 * TILE;
    constexpr int MI = 8, NI = 4;                         // wave tile 128 (rows) x 64 (couts); waves 2 x 4

    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages of { X [BKP][PITCH], DY [BKP][PITCH] }

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int wm = wave >> 2, wn = wave & 3;
    const int Mrows = a.R * a.S * a.C;
    // 1-D grid, XCD-aware: blocks b, b+8, ... share an XCD (and its L2); give each XCD a contiguous range of logical ids
    // with the (tap-row tile, cout tile) index fastest, so all tiles that stream the SAME pixel range run on ONE XCD and
    // x / dy are fetched from HBM once per split instead of once per tile (PMC: 14 % -> L2 hits; speed only).
    const int tilesM = (Mrows + BT - 1) / BT, tilesN = (a.K + BT - 1) / BT, tiles = tilesM * tilesN;
    int lid;
    {
        const int b = (int)blockIdx.x, nm = (int)gridDim.x;
        const int q = nm >> 3, rr = nm & 7, xcd = b & 7;
        lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
    }
    const int split = lid / tiles, tl = lid - split * tiles;
    const int m0 = (tl / tilesN) * BT, n0 = (tl % tilesN) * BT;
    const bool netb = split >= a.splits_per_net;          // second network's blocks (uniform per block)
    if (netb) { a.x = a.xb; a.dy = a.dyb; }
    const int pbeg = (netb ? split - a.splits_per_net : split) * a.pix_per_split;
    const int pend = min(a.P, pbeg + a.pix_per_split);

    // this thread stages LDS position `pos` of rows prow0 + RPS*i; it holds logical chunk pos ^ key(row)
    const int pos = tid % NCH, prow0 = tid / NCH;
    const int lc = pos ^ (wg2_key<T>(prow0) & (NCH - 1));            // key(row) is the same for every pass (see wg2_key)
    const int mrow = m0 + lc * VEC;
    const bool xcol_ok = mrow < Mrows;
    const int tap = xcol_ok ? mrow / a.C : 0, c0 = mrow - tap * a.C;
    const int tr = tap / a.S, ts = tap - tr * a.S;
    const bool dcol_ok = (n0 + lc * VEC) < a.K;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    auto stage_tile = [&](int stg, int p0) {
        char* sX = smem + stg * STAGE;
        char* sD = sX + TILE;
        if constexpr (ROWFAST) {
            // p0 is uniform and a multiple of BKP; P and the split size are multiples of BKP too: no tail, no row crossing
            const uint32_t n = fdiv((uint32_t)p0, a.dHW), rem = (uint32_t)p0 - n * a.dHW.d;
            const uint32_t ho = fdiv(rem, a.dW), wo0 = rem - ho * a.dW.d;
            int hi = (int)ho * a.stride - a.pad_t + tr;
            bool rowok = true;
            if (a.reflect) hi = hi < 0 ? -hi : (hi >= a.H ? 2 * (a.H - 1) - hi : hi);
            else rowok = (unsigned)hi < (unsigned)a.H;
            const char* xrow = a.x + ((size_t)n * a.H + (rowok ? hi : 0)) * a.W * a.C * ES + c0 * ES;
            const char* drow = a.dy + ((size_t)p0 * a.K + n0 + lc * VEC) * ES;
            const int wbase = (int)wo0 * a.stride - a.pad_l + ts;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int prow = prow0 + RPS * i;
                int wi = wbase + prow * a.stride;
                bool ok = rowok && xcol_ok;
                if (a.reflect) wi = wi < 0 ? -wi : (wi >= a.W ? 2 * (a.W - 1) - wi : wi);
                else ok = ok && (unsigned)wi < (unsigned)a.W;
                const char* sx = ok ? xrow + (uint32_t)(wi * a.C * ES) : zero;
                const char* sd = dcol_ok ? drow + (uint32_t)(prow * a.K * ES) : zero;
                const int wrow = (wave * 64) / NCH + RPS * i;
                dma16_to_lds(sx, (__attribute__((address_space(3))) void*)(sX + wrow * PITCH));
                dma16_to_lds(sd, (__attribute__((address_space(3))) void*)(sD + wrow * PITCH));
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int prow = prow0 + RPS * i, p = p0 + prow;
            const char* sx = zero;
            const char* sd = zero;
            if (p < pend) {
                if (xcol_ok) {
                    uint32_t n = fdiv((uint32_t)p, a.dHW), rem = (uint32_t)p - n * a.dHW.d;
                    uint32_t ho = fdiv(rem, a.dW), wo = rem - ho * a.dW.d;
                    int hi = (int)ho * a.stride - a.pad_t + tr, wi = (int)wo * a.stride - a.pad_l + ts;
                    bool ok = true;
                    if (a.reflect) {
                        hi = hi < 0 ? -hi : (hi >= a.H ? 2 * (a.H - 1) - hi : hi);
                        wi = wi < 0 ? -wi : (wi >= a.W ? 2 * (a.W - 1) - wi : wi);
                    } else ok = (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
                    if (ok) sx = a.x + ((((size_t)n * a.H + hi) * a.W + wi) * a.C + c0) * ES;
                }
                if (dcol_ok) sd = a.dy + ((size_t)p * a.K + n0 + lc * VEC) * ES;
            }
            // one wave-instruction = 64 lanes x 16 B = 1 KiB of consecutive tile bytes starting at the wave's first row
            const int wrow = (wave * 64) / NCH + RPS * i;
            dma16_to_lds(sx, (__attribute__((address_space(3))) void*)(sX + wrow * PITCH));
            dma16_to_lds(sd, (__attribute__((address_space(3))) void*)(sD + wrow * PITCH));
        }
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, u = lane & 15;
    const int ksteps = pend > pbeg ? (pend - pbeg + BKP - 1) / BKP : 0;
    if (ksteps > 0) stage_tile(0, pbeg);
    SGG_WAIT_VM0();
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
        const int cur = ks & 1;
        if (ks + 1 < ksteps) stage_tile(cur ^ 1, pbeg + (ks + 1) * BKP);
        const char* bX = smem + cur * STAGE;
        const char* bD = bX + TILE;
        if constexpr (sizeof(T) == 2) {
            // Fragment pipeline as in conv_gemm_glds_kernel: every dy fragment of the stage up front, x fragments in
            // groups of GJ fetched one group ahead of the MFMAs that consume them (the transposing reads otherwise sit
            // directly in front of their MFMAs and their latency is exposed whenever the DMA shares the LDS port).
            const int q = u >> 2, pp = u & 3;
            constexpr int KK = BKP / 32, GJ = 4, GPK = MI / GJ, NG = KK * GPK;
            auto ldT = [&](const char* base, int kk, int col) -> bf16x8 {
                const int r0 = kk * 32 + 8 * g + q, r1 = r0 + 4;
                const int k0 = wg2_key<T>(r0) & (NCH - 1), k1 = wg2_key<T>(r1) & (NCH - 1);
                const int ch = col >> 3, sub = (col & 7) * 2;
                bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4*)(base + r0 * PITCH + ((ch ^ k0) << 4) + sub));
                bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                    (__attribute__((address_space(3))) bf16x4*)(base + r1 * PITCH + ((ch ^ k1) << 4) + sub));
                return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            };
            bf16x8 fb[KK][NI];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                for (int j = 0; j < NI; ++j) fb[kk][j] = ldT(bD, kk, wn * 64 + j * 16 + 4 * pp);
            bf16x8 fa[2][GJ];
#pragma unroll
            for (int ii = 0; ii < GJ; ++ii) fa[0][ii] = ldT(bX, 0, wm * 128 + ii * 16 + 4 * pp);
#pragma unroll
            for (int gg = 0; gg < NG; ++gg) {
                const int kk = gg / GPK, ib = (gg % GPK) * GJ;
                if (gg + 1 < NG) {
                    const int kn = (gg + 1) / GPK, in = ((gg + 1) % GPK) * GJ;
#pragma unroll
                    for (int ii = 0; ii < GJ; ++ii) fa[(gg + 1) & 1][ii] = ldT(bX, kn, wm * 128 + (in + ii) * 16 + 4 * pp);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ii = 0; ii < GJ; ++ii)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[ib + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kk][j], fa[gg & 1][ii], acc[ib + ii][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int s4 = 0; s4 < BKP / 4; ++s4) {
                const int row = 4 * s4 + g;
                const int key = wg2_key<T>(row) & (NCH - 1);
                float fb[NI];
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    int col = wn * 64 + j * 16 + u;
                    fb[j] = *reinterpret_cast<const float*>(bD + row * PITCH + (((col >> 2) ^ key) << 4) + (col & 3) * 4);
                }
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    int col = wm * 128 + i * 16 + u;
                    float fa = *reinterpret_cast<const float*>(bX + row * PITCH + (((col >> 2) ^ key) << 4) + (col & 3) * 4);
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j], fa, acc[i][j], 0, 0, 0);
                }
            }
        }
        SGG_WAIT_VM0();
        __syncthreads();
    }

    // The dy fragment is the MFMA A operand, so D[row = cout][col = (tap,c)]: lane (g,u) owns couts 4g..4g+3 of row u ->
    // one 16-byte store per fragment into the [row][cout] slab (4x fewer store instructions than the transposed layout)
    float* slab = a.ws + (size_t)split * Mrows * a.K;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int mr = m0 + wm * 128 + i * 16 + u;
        if (mr >= Mrows) continue;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int k = n0 + wn * 64 + j * 16 + g * 4;
            if (k < a.K) *reinterpret_cast<f32x4*>(slab + (size_t)mr * a.K + k) = acc[i][j];
        }
    }
}

// dw[tap][c<Cr][k<Kr] (+)= sum_split ws[split][tap*C + c][k]   (fixed summation tree -> deterministic)
// One thread per 4 consecutive k (K is a multiple of 8): 16-byte slab reads, 4 independent partial sums in flight.
// dw2 != nullptr: two networks in one launch -- slabs [splits, 2 * splits) of ws sum into dw2
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, float* dw, int taps, int C, int K, int Cr, int Kr, int splits, int accumulate,
                                                           float* dw2 = nullptr) {
    const int K4 = K / 4;
    const int64_t total1 = (int64_t)taps * Cr * K4, total = dw2 ? 2 * total1 : total1;
    const size_t slab = (size_t)taps * C * K;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += (int64_t)gridDim.x * blockDim.x) {
        const bool netb = i0 >= total1;
        const int64_t i = netb ? i0 - total1 : i0;
        if (netb) dw = dw2;                              // (i0 only grows: once in the second network, always there)
        int k4 = (int)(i % K4);
        int64_t t = i / K4;
        int c = (int)(t % Cr), tap = (int)(t / Cr);
        const float* src = ws + (netb ? (size_t)splits * slab : 0) + ((size_t)tap * C + c) * K + k4 * 4;
        // eight independent 16-byte loads in flight per thread (the grid is only ~9 waves per CU: with four the pass ran at 4.8 TB/s),
        // combined in a fixed tree -> deterministic.  The slabs (their last use) are read with the streaming cache policy, which
        // leaves L2 / the Infinity Cache to the tensors the next kernels read: 283.5 -> 284.2 images/s of the step against plain
        // loads, profiles/r04_nt_loads.txt
        f32x4 acc8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc8[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        int sp = 0;
        for (; sp + 8 <= splits; sp += 8) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (size_t)(sp + u) * slab));
#pragma unroll
            for (int u = 0; u < 8; ++u) acc8[u] += v[u];
        }
        for (; sp < splits; ++sp) acc8[sp & 7] += *reinterpret_cast<const f32x4*>(src + (size_t)sp * slab);
        f32x4 s4 = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) + ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
        float* o = dw + ((size_t)tap * Cr + c) * Kr + k4 * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k4 * 4 + e < Kr) o[e] = accumulate ? o[e] + s4[e] : s4[e];
    }
}

// -------------------------------------------------------------------------------------------------
// Weight gradient of the narrow-output convolution of conv_halo_fwd_kernel (conv.hip): dW[(r,s,c)][k] = sum_pixels x~[p,(r,s),c] * dy[p][k] with
// k <= 16, c = 64.  Blocks walk 16x32-pixel tiles persistently; the input halo (DMA) and the dy tile sit in LDS;
// wave w owns taps w, w+8, ... (<= 7 of the 49) for all 64 channels, accumulating in registers across its tiles;
// both MFMA operands come from transposing LDS reads (pixels are the reduction index).  One f32 slab per block,
// summed by wgrad_reduce_kernel.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(512) void conv_halo_wgrad_kernel(WgradArgs a, int ntiles) {
    constexpr int ES = (int)sizeof(T);
    constexpr int CCH = 128 / ES;                       // channels per halo pass
    constexpr int CF = CCH / 16;                        // 16-channel fragments per pass (4 bf16 / 2 f32)
    constexpr int DPITCH = 16 * ES;                     // dy tile: 16 couts per pixel (zero padded)
    constexpr int TSLOTS = 7;                           // taps per wave (R*S <= 56)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sD = smem;                                    // [512 px][DPITCH]
    char* sH = smem + 512 * DPITCH;                     // halo

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int HWd = HALO_TW + a.S - 1, HHd = HALO_TH + a.R - 1, HP = HHd * HWd;
    const int tilesW = a.W / HALO_TW, tilesH = a.H / HALO_TH;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const int pos = tid & 7, lsw = (tid >> 4) & 7, lcc = pos ^ lsw;
    const int ntaps = a.R * a.S;
    const int g = lane >> 4, u = lane & 15, q = u >> 2, pp = u & 3;

    f32x4 acc[TSLOTS][4];
#pragma unroll
    for (int i = 0; i < TSLOTS; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int i = tid; i < 512 * DPITCH / 16; i += 512) st16(sD + i * 16, zero16());   // padded couts stay zero
    const int nchunks = a.C / CCH;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int b = tile;
        const int tw = b % tilesW; b /= tilesW;
        const int th = b % tilesH;
        const int n = b / tilesH;
        const int y0 = th * HALO_TH, x0 = tw * HALO_TW;
        for (int cc = 0; cc < nchunks; ++cc) {
            __syncthreads();
            for (int base = 0; base < HP; base += 64) {
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
                    if (ok) src = a.x + ((((size_t)n * a.H + yi) * a.W + xi) * a.C + cc * CCH) * ES + lcc * 16;
                }
                if (base + wave * 8 < HP)
                    dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sH + (base + wave * 8) * 128));
            }
            if (cc == 0) {                               // dy tile: thread = pixel; K*ES bytes of real data per pixel
                const int py = tid >> 5, px = tid & 31;
                const char* src = a.dy + (((size_t)n * a.H + y0 + py) * a.W + x0 + px) * a.K * ES;
                for (int o = 0; o < a.K * ES; o += 16) st16(sD + tid * DPITCH + o, ld16(src + o));
            }
            SGG_WAIT_VM0();
            __syncthreads();
            for (int y = 0; y < HALO_TH; ++y) {           // one k-step = the 32 pixels of tile row y
                if constexpr (sizeof(T) == 2) {
                    const int p0 = y * 32 + 8 * g + q;
                    bf16x4 blo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sD + p0 * DPITCH + pp * 8));
                    bf16x4 bhi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sD + (p0 + 4) * DPITCH + pp * 8));
                    const bf16x8 fb = (bf16x8){blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
#pragma unroll
                    for (int i = 0; i < TSLOTS; ++i) {
                        const int t = wave + 8 * i;
                        if (t >= ntaps) break;
                        const int r = t / a.S, s = t - r * a.S;
                        const int h0 = (y + r) * HWd + s + 8 * g + q, h1 = h0 + 4;
#pragma unroll
                        for (int c = 0; c < CF; ++c) {
                            const int col = c * 16 + 4 * pp, ch = col >> 3, sub = (col & 7) * 2;
                            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                (__attribute__((address_space(3))) bf16x4*)(sH + h0 * 128 + ((ch ^ ((h0 >> 1) & 7)) << 4) + sub));
                            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                                (__attribute__((address_space(3))) bf16x4*)(sH + h1 * 128 + ((ch ^ ((h1 >> 1) & 7)) << 4) + sub));
                            const bf16x8 fa = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[i][c], 0, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int s4 = 0; s4 < 8; ++s4) {          // 4 pixels per MFMA
                        const int xk = 4 * s4 + g;
                        const float fb = *reinterpret_cast<const float*>(sD + (y * 32 + xk) * DPITCH + u * 4);
#pragma unroll
                        for (int i = 0; i < TSLOTS; ++i) {
                            const int t = wave + 8 * i;
                            if (t >= ntaps) break;
                            const int r = t / a.S, s = t - r * a.S;
                            const int hp = (y + r) * HWd + s + xk;
#pragma unroll
                            for (int c = 0; c < CF; ++c) {
                                const int col = c * 16 + u;
                                const float fa = *reinterpret_cast<const float*>(sH + hp * 128 + (((col >> 2) ^ ((hp >> 1) & 7)) << 4) + (col & 3) * 4);
                                acc[i][cc * CF + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, fb, acc[i][cc * CF + c], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
    }

    // D[row = 4g+e -> channel][col = u -> cout]
    float* slab = a.ws + (size_t)blockIdx.x * ntaps * a.C * a.K;
    if (u < a.K) {
#pragma unroll
        for (int i = 0; i < TSLOTS; ++i) {
            const int t = wave + 8 * i;
            if (t >= ntaps) break;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c * 16 >= a.C) break;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    slab[((size_t)t * a.C + c * 16 + g * 4 + e) * a.K + u] = acc[i][c][e];
            }
        }
    }
}

static bool halo_wgrad_ok(const sgg_conv_desc* d) {
    const int cch = d->dtype == SGG_BF16 ? 64 : 32;
    return d->K <= 16 && d->stride == 1 && d->R <= HALO_MAXR && d->S <= HALO_MAXR && d->R * d->S <= 56 &&
           d->Ho == d->H && d->Wo == d->W && d->H % HALO_TH == 0 && d->W % HALO_TW == 0 && d->C <= 64 && d->C % cch == 0;
}
static int halo_wgrad_blocks(const sgg_conv_desc* d) {
    int ntiles = d->N * (d->H / HALO_TH) * (d->W / HALO_TW);
    return ntiles < 256 ? ntiles : 256;
}

// -------------------------------------------------------------------------------------------------
// Weight gradient of the two 7x7 layers with a 3-channel side (bf16): the head (64 -> 3, module.py:262-264) and the
// stem (3 -> 64, module.py:230-232).  Both are
//     G[r][s][c][j] = sum_{n, py, px} A~[n][py + r - pa][px + s - pa][c] * B[n][py][px][j],     c < 64, j < 3
// with A the 64-channel tensor (head: the layer input, REFLECT padded; stem: dy, zero padded by 6 -- the sum then runs
// over the PADDED grid, B = the explicitly reflect-padded input, and taps come out mirrored) and B the 3-channel one.
// conv_halo_wgrad_kernel gives every tap its own MFMAs with 13 of 16 columns empty (196 per 32 pixels, two LDS reads
// each).  Here the GEMM N dimension carries (j, tap column s) = 3 x 7 -> 32 and each wave owns ONE tap row r:
//     D_r[c][(j,s)] += sum_q A~[py + r][q][c] * Bs[py][q][(j,s)],      Bs[py][q][(j,s)] = B[py][q - s][j]
// (q = padded column inside a 58-pixel strip: 64 values = two k-steps), 8 MFMAs per 32 pixels and wave, 12 LDS reads.
// Bs -- an im2col of the 3-channel tensor along the row, 64 B per pixel -- is built in LDS by the eighth wave while
// waves 0..6 multiply.  A block walks down a strip 4 rows at a time: the 4 new A rows are DMA'd into a 14-row ring
// while the other 10 are in use.  Both operands are read with the transposing ds_read_b64_tr_b16 (pixels are the
// reduction index).  One f32 slab [7][64][32] per block; wgrad7_reduce_kernel sums them in fixed order.
// -------------------------------------------------------------------------------------------------
#ifndef W7_INTERLEAVE
#define W7_INTERLEAVE 1                                // the main loop's A-row DMAs between the MFMA batches (0: all at the head of the step)
#endif
#define W7_TW 58                                        // strip width in pixels of B's grid (58 + 6 = 64 = two k-steps)
#define W7_AROW (64 * 128)                              // bytes per A row (64 pixels x 64 channels)
#define W7_BSROW (64 * 64)                              // bytes per Bs row (64 pixels x 32 columns)
// RS rows per step; A rows are DMA'd PD steps ahead (they come from HBM: ~2 us under load, a step is < 1 us) into a
// ring of RS + 6 + PD*RS rows; raw B rows three steps ahead into a ring of 4 steps; Bs double-buffered.
template <int RS, int PD> struct W7Cfg {
    static constexpr int RING = RS + 6 + PD * RS;
    static constexpr int OFF_BS = RING * W7_AROW;
    static constexpr int OFF_BRAW = OFF_BS + 2 * RS * W7_BSROW;
    static constexpr int LDS = OFF_BRAW + 4 * RS * 512 + 1024;
    static constexpr int B_PER_STEP = RS * 2;           // raw-B DMA instructions per step (wave 7)
    static constexpr int NISS = 6;                      // waves 0..5 issue the main loop's A-row DMAs (wave 7 has the B side)
    static constexpr int A_PER_WAVE = RS * 8 / NISS;    // RS rows x 8 instructions over the issuer waves
    static_assert(RS * 8 % NISS == 0, "issuer waves must carry equal DMA counts (the vmcnt bookkeeping relies on it)");
};

struct W7Args {
    const char* A;       // (N,HA,WA,64) bf16
    const char* B;       // (N,HB,WB,8) bf16 -- the summation grid
    float* slabs;        // [blocks][7][64][32] f32
    int N, HA, WA, HB, WB, pa, reflectA, nstrips, nseg, rows_per_seg;
    int ablate;          // lab build only (SGG_ABLATE): 1 no fragment reads / MFMAs, 2 no Bs build, 3 no A-row DMA in the loop
};

template <int N> __device__ inline void w7_wait_vm() { sgg_wait_vm<N>(); }

template <int RS, int PD>
__global__ __launch_bounds__(512) void wgrad7_kernel(W7Args a) {
    using Cfg = W7Cfg<RS, PD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) char lds_char;
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    int b = blockIdx.x;
    const int seg = b % a.nseg; b /= a.nseg;
    const int strip = b % a.nstrips;
    const int n = b / a.nstrips;
    const int yb = seg * a.rows_per_seg;
    const int ye = yb + a.rows_per_seg < a.HB ? yb + a.rows_per_seg : a.HB;
    const int x0 = strip * W7_TW;
    const int nsteps = (ye - yb + RS - 1) / RS;

    // ---- A rows: ring row k (k = 0 .. rows + 5) is image row yb + k - pa; 8 DMA instructions of 8 pixels per row.
    // Rows k0 .. k0+nrows-1; instruction ids are dealt round-robin to the issuing waves.  Rows past the image read the zero page.
    const int hsub = lane >> 3, hpos = lane & 7;
    auto load_a_rows = [&](int k0, int nrows, int vw, int nw, int j0 = 0, int j1 = 1 << 20) {   // this wave acts as issuer vw of nw; its pieces [j0, j1)
        for (int id = vw + nw * j0, j = j0; id < nrows * 8 && j < j1; id += nw, ++j) {
            const int k = k0 + (id >> 3), i = id & 7;
            const int q = i * 8 + hsub;
            int yi = yb + k - a.pa, xi = x0 - a.pa + q;
            if (a.reflectA) {
                yi = yi < 0 ? -yi : (yi >= a.HA ? 2 * (a.HA - 1) - yi : yi);
                xi = xi < 0 ? -xi : (xi >= a.WA ? 2 * (a.WA - 1) - xi : xi);
            }
            const bool ok = (unsigned)yi < (unsigned)a.HA && (unsigned)xi < (unsigned)a.WA;
            const int key = ((q >> 1) & 1) | (((q >> 3) & 1) << 1);           // keyed on pixel bits 1 and 3: the transposed reads are conflict-free
            const char* src = ok ? a.A + ((((size_t)n * a.HA + yi) * a.WA + xi) * 64) * 2 + ((hpos ^ (key << 1)) << 4) : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(lds + (k % Cfg::RING) * W7_AROW + i * 1024));
        }
    };
    // ---- B rows of a step (wave 7): raw row DMA, then the im2col Bs[q][(j,s)] = B[q - s][j]
    auto load_b_raw = [&](int step) {                    // one lane = one pixel; a 4-byte wave-instruction moves 64 x 4 B:
        for (int i = 0; i < RS; ++i) {                   // dword 0 = channels (0,1), dword 1 = (2,3)
            const int py = yb + step * RS + i, px = x0 + lane;
            const bool ok = py < ye && lane < W7_TW && px < a.WB;
            const char* src = ok ? a.B + (((size_t)n * a.HB + py) * a.WB + px) * 16 : zero;
#pragma unroll
            for (int part = 0; part < 2; ++part)
                dma4_to_lds(src + part * 4, (__attribute__((address_space(3))) void*)(lds + Cfg::OFF_BRAW + ((step & 3) * RS + i) * 512 + part * 256));
        }
    };
    auto build_bs = [&](int step) {
        char* bs = smem + Cfg::OFF_BS + (step & 1) * (RS * W7_BSROW);
        const int q = lane;
        const int bsw = ((q >> 3) & 1) << 1;                                   // chunk swizzle of the Bs rows
        for (int i = 0; i < RS; ++i) {
            const char* raw = smem + Cfg::OFF_BRAW + ((step & 3) * RS + i) * 512;   // [part 0..1][pixel] dwords
            uint32_t lo[7], hi[7];                                             // pixel q - s: channels (0,1) and (2,3)
            // (unconditional loads from a clamped index + a select: a conditional load becomes a branch with a full
            // lgkmcnt(0) wait behind every read, ~2 000 cycles per row)
#pragma unroll
            for (int sc = 0; sc < 7; ++sc) {
                const int idx = q - sc, ic = idx < 0 ? 0 : idx;
                lo[sc] = *reinterpret_cast<const uint32_t*>(raw + 4 * ic);
                hi[sc] = *reinterpret_cast<const uint32_t*>(raw + 256 + 4 * ic);
            }
#pragma unroll
            for (int sc = 0; sc < 7; ++sc) {
                const bool ok = q - sc >= 0;
                lo[sc] = ok ? lo[sc] : 0u;
                hi[sc] = ok ? hi[sc] : 0u;
            }
            // columns n = j*8 + s: 16-byte chunk j holds s = 0..6 (+ a zero) for channel j; chunk 3 is zero
            u32x4 ch[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                uint32_t e[8];
#pragma unroll
                for (int sc = 0; sc < 7; ++sc) {
                    const uint32_t w = j < 2 ? lo[sc] : hi[sc];
                    e[sc] = (j == 1) ? (w >> 16) : (w & 0xffffu);
                }
                e[7] = 0u;
                ch[j] = (u32x4){e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
            }
            char* row = bs + i * W7_BSROW + q * 64;
            st16(row + ((0 ^ bsw) << 4), ch[0]);
            st16(row + ((1 ^ bsw) << 4), ch[1]);
            st16(row + ((2 ^ bsw) << 4), ch[2]);
            st16(row + ((3 ^ bsw) << 4), zero16());
        }
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) acc[it][jt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // prologue (all 8 waves issue, everything is drained): A rows of steps 0 .. PD-1, raw B of steps 0 and 1, Bs of step 0
    if (wave == 7) load_b_raw(0);
    load_a_rows(0, RS + 6 + (PD - 1) * RS, wave, 8);
    SGG_WAIT_VM0();
    if (wave == 7) {
        build_bs(0);
        load_b_raw(1);
        load_b_raw(2);
    }
    SGG_WAIT_LGKM0();
    __syncthreads();

    // Transposed fragment reads: lane 4qq+pp of 16-lane group g supplies row (pixel) 8g+qq [+4 for the upper half], columns
    // 4pp..4pp+3 of the 16-column tile.  Everything lane-dependent is folded into six LDS byte addresses computed once
    // (the swizzle keys depend only on pixel bits 1 and 3 = qq bit 1 and g bit 0); a read is then base + scalar + immediate.
    const int g = lane >> 4, u = lane & 15, qq = u >> 2, pp = u & 3;
    const uint32_t lb = (uint32_t)(uintptr_t)lds;
    const int keyA = ((qq >> 1) & 1) | ((g & 1) << 1);
    uint32_t offA[4], offB[2];
#pragma unroll
    for (int it = 0; it < 4; ++it) offA[it] = lb + (8 * g + qq) * 128 + ((((it ^ keyA) << 1) | (pp >> 1)) << 4) + (pp & 1) * 8;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) offB[jt] = lb + Cfg::OFF_BS + (8 * g + qq) * 64 + ((((jt * 2) | (pp >> 1)) ^ ((g & 1) << 1)) << 4) + (pp & 1) * 8;
    auto tr = [](uint32_t addr) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(uintptr_t)addr); };
    for (int t = 0; t < nsteps; ++t) {
        // rows of step t + PD into the slots step t - 1 released, by waves 0..5 (always issued: rows past the segment are
        // harmless and keep every issuer's count of outstanding DMAs per step constant)
        if (!W7_INTERLEAVE && wave < Cfg::NISS && SGG_ABLATE_OF(a) != 3) load_a_rows(RS + 6 + (t + PD - 1) * RS, RS, wave, Cfg::NISS);
        if (wave < 7 && SGG_ABLATE_OF(a) == 1) {
        } else if (wave < 7) {
            const int r = wave;
            // RS x 2 batches of (2 B + 4 A fragments -> 8 MFMAs); the fragments of batch b+1 are requested before the MFMAs
            // of batch b are issued (a batch's reads would otherwise sit exposed: ~200 cycles of LDS latency per 128 of MFMA)
            bf16x4 fbq[2][2][2], faq[2][4][2];            // [buffer][tile][lo/hi]
            auto request = [&](int bi, int buf) {
                const int i = bi >> 1, ks = bi & 1;
                const uint32_t abase = (uint32_t)((t * RS + i + r) % Cfg::RING) * W7_AROW + ks * 32 * 128;
                const uint32_t bbase = (uint32_t)((t & 1) * RS + i) * W7_BSROW + ks * 32 * 64;
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) { fbq[buf][jt][0] = tr(offB[jt] + bbase); fbq[buf][jt][1] = tr(offB[jt] + bbase + 4 * 64); }
#pragma unroll
                for (int it = 0; it < 4; ++it) { faq[buf][it][0] = tr(offA[it] + abase); faq[buf][it][1] = tr(offA[it] + abase + 4 * 128); }
            };
            request(0, 0);
#pragma unroll
            for (int bi = 0; bi < RS * 2; ++bi) {
                const int buf = bi & 1;
                if (bi + 1 < RS * 2) request(bi + 1, buf ^ 1);
                __builtin_amdgcn_sched_barrier(0);
                bf16x8 fb[2];
#pragma unroll
                for (int jt = 0; jt < 2; ++jt) {
                    const bf16x4 lo = fbq[buf][jt][0], hi = fbq[buf][jt][1];
                    fb[jt] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const bf16x4 lo = faq[buf][it][0], hi = faq[buf][it][1];
                    const bf16x8 fa = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                    for (int jt = 0; jt < 2; ++jt) acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[jt], acc[it][jt], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // the A-row DMAs of step t + PD, ONE piece per issuer wave after each of its first MFMA batches instead of all of
                // them at the head of the step: a piece costs its wave 60-180 cycles of issue, which now fall under the SIMD
                // partner's MFMAs (with all six issuers at the head of the step the matrix pipes idled for that long every step)
                if (W7_INTERLEAVE && bi < Cfg::A_PER_WAVE && wave < Cfg::NISS && SGG_ABLATE_OF(a) != 3) {
                    load_a_rows(RS + 6 + (t + PD - 1) * RS, RS, wave, Cfg::NISS, bi, bi + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // the rows of step t+1 (issued PD-1 steps ago) have landed; the later steps' may still be in flight
            if (wave < Cfg::NISS) w7_wait_vm<Cfg::A_PER_WAVE * (PD - 1)>();
        } else {
            // wave 7: raw B of step t+1 (issued TWO steps ago; only its own B DMAs are in its queue, step t+2's may still
            // fly) -> Bs(t+1) while the others multiply; then the raw B of step t+3 goes out.  (With the raw rows requested
            // only one step ahead this wave sat out a full HBM latency per step, and the block with it.)
            w7_wait_vm<Cfg::B_PER_STEP>();
            if (SGG_ABLATE_OF(a) != 2) build_bs(t + 1);
            load_b_raw(t + 3);
        }
        SGG_WAIT_LGKM0();
        __syncthreads();
    }
    SGG_WAIT_VM0();     // nothing may still be writing LDS when the block retires

    // D_r[row = it*16 + 4g + e -> channel c][col = jt*16 + u -> (j,s)]
    if (wave < 7) {
        float* slab = a.slabs + ((size_t)blockIdx.x * 7 + wave) * 64 * 32;
#pragma unroll
        for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int jt = 0; jt < 2; ++jt)
#pragma unroll
                for (int e = 0; e < 4; ++e) slab[(it * 16 + 4 * g + e) * 32 + jt * 16 + u] = acc[it][jt][e];
    }
}

// dw[...] (+)= sum over blocks of slab[b][r][c][j*8 + s], in fixed order.  mode 0 (head): dw is HWIO (7,7,64,Kr):
// dw[r][s][c][j].  mode 1 (stem): dw is (7,7,Cr,64) and the taps come out mirrored: dw[6-r][6-s][j][c].
__global__ __launch_bounds__(1024) void wgrad7_reduce_kernel(const float* slabs, int nblocks, float* dw, int mode, int nj, int accumulate) {
    __shared__ float red[32][32];
    const int o = threadIdx.x & 31, part = threadIdx.x >> 5;     // 32 outputs x 32 slab lanes
    const int idx = blockIdx.x * 32 + o;                 // (r, c, col) with col = j*8 + s in 0..31
    const int col = idx & 31, c = (idx >> 5) & 63, r = idx >> 11;
    float v = 0.f;
    for (int b0 = part; b0 < nblocks; b0 += 32 * 4) {    // four independent loads in flight, added in slab order
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = b0 + 32 * k;
            x[k] = b < nblocks ? slabs[(size_t)b * (7 * 64 * 32) + idx] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v += x[k];
    }
    red[part][o] = v;
    __syncthreads();
    if (part == 0) {
        float t = 0.f;
#pragma unroll
        for (int p = 0; p < 32; ++p) t += red[p][o];
        const int j = col >> 3, sc = col & 7;
        if (j < nj && sc < 7) {
            float* d = mode == 0 ? dw + ((size_t)(r * 7 + sc) * 64 + c) * nj + j
                                 : dw + ((size_t)((6 - r) * 7 + (6 - sc)) * nj + j) * 64 + c;
            *d = accumulate ? *d + t : t;
        }
    }
}

// explicit REFLECT pad 3 of an 8-channel bf16 tensor (the stem's input, as wgrad7_kernel's B operand): (N,H,W,8) -> (N,H+6,W+6,8)
__global__ __launch_bounds__(256) void reflect_pad3_kernel(const char* x, char* xp, int N, int H, int W) {
    const int Hp = H + 6, Wp = W + 6;
    const int64_t total = (int64_t)N * Hp * Wp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int wp = (int)(i % Wp);
        const int64_t t = i / Wp;
        const int hp = (int)(t % Hp), n = (int)(t / Hp);
        int h = hp - 3, w = wp - 3;
        h = h < 0 ? -h : (h >= H ? 2 * (H - 1) - h : h);
        w = w < 0 ? -w : (w >= W ? 2 * (W - 1) - w : w);
        st16(xp + (size_t)i * 16, ld16(x + (((size_t)n * H + h) * W + w) * 16));
    }
}

#ifndef W7_RSTEP
#define W7_RSTEP 3
#define W7_PDIST 2
#endif
struct W7Plan { int HB, WB, nstrips, nseg, rows_per_seg, blocks; size_t slab_bytes, xpad_bytes; };
static W7Plan w7_plan(const sgg_conv_desc* d, bool stem) {
    W7Plan p;
    p.HB = d->H + (stem ? 6 : 0); p.WB = d->W + (stem ? 6 : 0);
    p.nstrips = (p.WB + W7_TW - 1) / W7_TW;
    int nseg = 512 / (d->N * p.nstrips);                 // ~2 blocks per CU (one resident at a time: 150 KB of LDS)
    if (nseg < 1) nseg = 1;
    int rps = (p.HB + nseg - 1) / nseg;
    rps = (rps + W7_RSTEP - 1) / W7_RSTEP * W7_RSTEP;
    if (rps < 8) rps = 8;
    p.rows_per_seg = rps;
    p.nseg = (p.HB + rps - 1) / rps;
    p.blocks = d->N * p.nstrips * p.nseg;
    p.slab_bytes = (size_t)p.blocks * 7 * 64 * 32 * sizeof(float);
    p.xpad_bytes = stem ? align_up((size_t)d->N * p.HB * p.WB * 16, 256) : 0;
    return p;
}
static int run_w7(const sgg_conv_desc* d, bool stem, const void* x, const void* dy, float* dw, int Cr, int Kr, int accumulate,
                  void* ws, size_t ws_bytes, hipStream_t s) {
    const W7Plan p = w7_plan(d, stem);
    if (!ws || ws_bytes < p.slab_bytes + p.xpad_bytes) return SGG_EWORKSPACE;
    if ((stem ? Cr : Kr) > 3) return SGG_EUNSUPPORTED;
    W7Args a;
    a.slabs = (float*)ws;
    a.N = d->N; a.HB = p.HB; a.WB = p.WB; a.nstrips = p.nstrips; a.nseg = p.nseg; a.rows_per_seg = p.rows_per_seg;
    a.HA = d->H; a.WA = d->W; a.ablate = sgg_config().ablate;
    if (stem) {
        char* xpad = (char*)ws + p.slab_bytes;
        const int64_t total = (int64_t)d->N * p.HB * p.WB;
        int blocks = (int)((total + 255) / 256); if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(reflect_pad3_kernel, dim3(blocks), dim3(256), 0, s, (const char*)x, xpad, d->N, d->H, d->W);
        a.A = (const char*)dy; a.B = xpad; a.pa = 6; a.reflectA = 0;
    } else {
        a.A = (const char*)x; a.B = (const char*)dy; a.pa = 3; a.reflectA = d->pad_mode == SGG_PAD_REFLECT;
    }
    auto kern = wgrad7_kernel<W7_RSTEP, W7_PDIST>;
    constexpr int lds = W7Cfg<W7_RSTEP, W7_PDIST>::LDS;
    static_assert(lds <= 160 * 1024, "wgrad7 LDS budget");
    SGG_LDS_ATTR(kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)p.blocks), dim3(512), lds, s, a);
    int rc = sgg_check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(wgrad7_reduce_kernel, dim3(7 * 64 * 32 / 32), dim3(1024), 0, s, (const float*)ws, p.blocks, dw, stem ? 1 : 0, stem ? Cr : Kr, accumulate);
    return sgg_check_launch();
}

// -------------------------------------------------------------------------------------------------
// Weight gradient of the discriminator's first conv (module.py:284: 3x3, stride 2, SAME, 3(8) -> 64 channels; D.h0: x has 3 real
// channels, dy 64): dW[r][s][c][k] = sum_pixels x[2yo+r][2xo+s][c] dy[yo][xo][k],
// a 27 x 64 result over 262 144 pixels per 8 images.  As a GEMM the reduction runs over pixels, so both operands would have to be
// transposed through LDS for 0.45 GMAC of work; the register-staged generic kernel (v1) ran it at 20 TFLOP/s, 46.6 us incl. 21 us
// of slab reduce (now 28 + 5 us).  The work is
// small enough for the vector ALU: a lane owns one output channel k and keeps the 9 x CR sums in registers; per output pixel it
// reads its dy value (one 128-byte line per wave) and multiplies it with the pixel's 9 x CR input values, which every lane reads
// from the SAME LDS address (a broadcast read) out of three input rows staged as float32.  A block walks (image, output row, half
// row) units; its four waves split a unit's pixels, add up through LDS in fixed order at the end and write ONE slab per block.
// -------------------------------------------------------------------------------------------------
#define S2W_SEG 128                                     // output pixels per unit
#define S2W_XPIX (2 * S2W_SEG + 2)                      // input pixels per staged row (+1 used, +1 pad)
template <int CR>                                      // input channels computed (4: the first half of the padded 8)
__global__ __launch_bounds__(256) void conv3x3s2_narrow_wgrad_kernel(const char* __restrict__ x, const char* __restrict__ dy, float* __restrict__ ws,
                                                                     int N, int H, int W, int Ho, int Wo, int units, int units_per_block) {
    constexpr int CV = CR <= 4 ? 4 : 8;                 // floats per staged pixel
    // staging buffers and, after the last unit, the cross-wave reduction buffer share one allocation
    constexpr int XB = 3 * S2W_XPIX * CV * 4, DB = S2W_SEG * 64 * 2, RB = 4 * 9 * CR * 64 * 4;
    __shared__ __attribute__((aligned(16))) char sraw[(XB + DB > RB) ? (XB + DB) : RB];
    float (*sX)[S2W_XPIX][CV] = reinterpret_cast<float (*)[S2W_XPIX][CV]>(sraw);
    bf16 (*sD)[64] = reinterpret_cast<bf16 (*)[64]>(sraw + XB);
    float (*sRed)[9 * CR][64] = reinterpret_cast<float (*)[9 * CR][64]>(sraw);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int segs = (Wo + S2W_SEG - 1) / S2W_SEG;
    float acc[9][CR];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < CR; ++c) acc[t][c] = 0.f;
    const int u0 = blockIdx.x * units_per_block, u1 = min(units, u0 + units_per_block);
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    // a unit's operands travel global -> registers -> LDS; the NEXT unit's loads are issued before this unit's arithmetic
    // (with the dy values read straight from global memory per pixel the kernel was latency bound: 91 us)
    constexpr int XL = (3 * S2W_XPIX + 255) / 256, DL = S2W_SEG * 8 / 256;     // 16-byte pieces per thread
    u32x4 rx[XL], rd[DL];
    auto fetch = [&](int u) {
        int b = u;
        const int seg = b % segs; b /= segs;
        const int yo = b % Ho;
        const int n = b / Ho;
        const int xo0 = seg * S2W_SEG, X0 = 2 * xo0;
#pragma unroll
        for (int l = 0; l < XL; ++l) {
            const int i = tid + 256 * l;
            const int r = i / S2W_XPIX, px = i - r * S2W_XPIX;
            const int Y = 2 * yo + r, X = X0 + px;
            // (a select between ADDRESSES, not a conditional load: that compiles to a branch with a full vmcnt(0) wait behind it)
            const bool ok = i < 3 * S2W_XPIX && Y < H && X < W;                  // bottom / right padding: zeros
            rx[l] = ld16(ok ? x + (((size_t)n * H + Y) * W + X) * 16 : zero);
        }
#pragma unroll
        for (int l = 0; l < DL; ++l) {
            const int i = tid + 256 * l, p = i >> 3, ch = i & 7;
            rd[l] = ld16(xo0 + p < Wo ? dy + ((((size_t)n * Ho + yo) * Wo + xo0 + p) * 64 + ch * 8) * 2 : zero);
        }
    };
    if (u0 < u1) fetch(u0);
    for (int u = u0; u < u1; ++u) {
        __syncthreads();                                // the previous unit's reads of sX / sD are done
#pragma unroll
        for (int l = 0; l < XL; ++l) {
            const int i = tid + 256 * l;
            if (i >= 3 * S2W_XPIX) continue;
            const int r = i / S2W_XPIX, px = i - r * S2W_XPIX;
            float v[8];
            // (opaque to the optimiser until here: it otherwise converts each piece right behind its load in fetch() -- same
            // register count -- and waits for vmcnt(0) there, four dependent round trips per unit instead of a prefetch)
            asm volatile("" : "+v"(rx[l][0]), "+v"(rx[l][1]), "+v"(rx[l][2]), "+v"(rx[l][3]));
            ET<bf16>::unpack(rx[l], v);
#pragma unroll
            for (int e = 0; e < CV; e += 4) *reinterpret_cast<f32x4*>(&sX[r][px][e]) = (f32x4){v[e], v[e + 1], v[e + 2], v[e + 3]};
        }
#pragma unroll
        for (int l = 0; l < DL; ++l) {
            const int i = tid + 256 * l;
            st16(reinterpret_cast<char*>(&sD[0][0]) + i * 16, rd[l]);
        }
        __syncthreads();
        if (u + 1 < u1) fetch(u + 1);
        // this wave's quarter of the unit, four pixels per trip
        const int p0 = wave * (S2W_SEG / 4);
        for (int p = p0; p < p0 + S2W_SEG / 4; p += 4) {
            uint16_t draw[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) draw[q] = reinterpret_cast<const uint16_t*>(&sD[p + q][0])[lane];
            float dv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) dv[q] = __uint_as_float((uint32_t)draw[q] << 16);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int sx = 0; sx < 3; ++sx) {
                        const float* xv = &sX[r][2 * (p + q) + sx][0];     // the same address in every lane: a broadcast read
#pragma unroll
                        for (int c = 0; c < CR; ++c) acc[r * 3 + sx][c] = fmaf(dv[q], xv[c], acc[r * 3 + sx][c]);
                    }
        }
    }
    // block total in fixed wave order -> slab [9][8][64] (rows c >= Cr are never read by the reducer)
    __syncthreads();                                    // (sRed aliases the staging buffers)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < CR; ++c) sRed[wave][t * CR + c][lane] = acc[t][c];
    __syncthreads();
    float* slab = ws + (size_t)blockIdx.x * 9 * 8 * 64;
    for (int i = tid; i < 9 * CR * 64; i += 256) {
        const int row = i >> 6, k = i & 63;
        const float v = ((sRed[0][row][k] + sRed[1][row][k]) + sRed[2][row][k]) + sRed[3][row][k];
        slab[((row / CR) * 8 + (row % CR)) * 64 + k] = v;
    }
}

// Reducer for MANY small slabs (D.h0: 512 slabs of a 27 x 64 result): wgrad_reduce_kernel gives every output its own thread, which
// then walks all slabs -- 432 threads and 64 dependent rounds of loads here.  This one puts a WAVE on each 16-byte output: lane l sums
// slabs l, l + 64, ... (all loads in flight), then a fixed-order butterfly; blockIdx.y = network of a two-network launch.
__global__ __launch_bounds__(256) void wgrad_reduce_wide_kernel(const float* ws, float* dw, float* dw2, int taps, int C, int K, int Cr, int Kr, int splits, int accumulate) {
    const int K4 = K / 4, lane = threadIdx.x & 63;
    const int total = taps * Cr * K4;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= total) return;
    const int net = blockIdx.y;
    float* const out = net ? dw2 : dw;
    const size_t slab = (size_t)taps * C * K;
    const int k4 = i % K4, t = i / K4, c = t % Cr, tap = t / Cr;
    const float* src = ws + (size_t)net * splits * slab + ((size_t)tap * C + c) * K + k4 * 4;
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int sp = lane; sp < splits; sp += 64) v += *reinterpret_cast<const f32x4*>(src + (size_t)sp * slab);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], off);
    if (lane == 0) {
        float* o = out + ((size_t)tap * Cr + c) * Kr + k4 * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k4 * 4 + e < Kr) o[e] = accumulate ? o[e] + v[e] : v[e];
    }
}

#define S2W_BLOCKS 512                                  // persistent blocks = slabs (1024 / 2048 measured 7 / 22 % slower)
static bool s2n_wgrad_ok(const sgg_conv_desc* d) {
    return d->dtype == SGG_BF16 && d->pad_mode == SGG_PAD_ZERO && d->R == 3 && d->S == 3 && d->stride == 2 && d->C == 8 && d->K == 64 &&
           d->pad_t == 0 && d->pad_l == 0 && d->H == 2 * d->Ho && d->W == 2 * d->Wo;
}
struct S2WGrid { int units, per_block, blocks; };       // blocks = slabs
static S2WGrid s2n_wgrad_grid(const sgg_conv_desc* d) {
    S2WGrid g;
    g.units = d->N * d->Ho * ((d->Wo + S2W_SEG - 1) / S2W_SEG);
    g.per_block = (g.units + S2W_BLOCKS - 1) / S2W_BLOCKS;
    g.blocks = (g.units + g.per_block - 1) / g.per_block;
    return g;
}
static int launch_s2n_wgrad(const sgg_conv_desc* d, const void* x, const void* dy, float* ws, int Cr, hipStream_t s) {
    const S2WGrid g = s2n_wgrad_grid(d);
    if (Cr > 4) return SGG_EUNSUPPORTED;                  // (plan_wgrad sends wider inputs to the generic kernel)
    // four channels per pixel although D.h0 has three (the fourth is the tensor's zero padding): 36 sums = 18 register PAIRS
    // for v_pk_fma_f32 and one ds_read_b128 per tap; with 27 sums hipcc spent 90 v_mov per four pixels lining operands up
    hipLaunchKernelGGL(conv3x3s2_narrow_wgrad_kernel<4>, dim3((unsigned)g.blocks), dim3(256), 0, s, (const char*)x, (const char*)dy, ws,
                       d->N, d->H, d->W, d->Ho, d->Wo, g.units, g.per_block);
    return sgg_check_launch();
}

// -------------------------------------------------------------------------------------------------
// 3x3 stride-1 weight gradient with the x HALO resident in LDS and ALL 9 TAPS accumulated by one block (the residual
// blocks' convs, module.py:210-216 backward).
//
// conv_wgrad_glds_kernel gives every tap its own block, so a stage streams 32 KB of x and 32 KB of dy per 8.4 MFLOP
// and the kernel is bound by that L2->LDS stream, not by the MFMAs.  Here a block owns
// dW[9 taps][64 c][128 k] (36 MFMA tiles per wave: 9 taps x 4 cout tiles of its 16-channel slice) and walks pixel
// tiles of 2 rows x 64 columns: per stage the 4 x 66 halo pixels of its 64 input channels (36 KB) serve all nine taps
// as shifted rows, next to a [128 px][128 k] dy tile (32 KB) -- 68 KB per 18.9 MFLOP, 2.1x the FLOP per staged byte.
// Operands are transposed on the fly with ds_read_b64_tr_b16 as in conv_wgrad_glds_kernel; dy keeps that kernel's
// swizzle (256-byte rows), the 128-byte halo rows use w9_xkey (below), conflict-free for any tap shift.
// Pixel tiles are split over `splits` blocks per output tile; slabs are summed in fixed order by wgrad_reduce_kernel.
// -------------------------------------------------------------------------------------------------
#define W9_TW 64
#define W9_PITCH 72                                    // halo row pitch in pixels (66 used; multiple of 8 = one DMA)
#define W9_XBYTES (4 * W9_PITCH * 128)
#define W9_DBYTES (128 * 256)
#define W9_STAGE (W9_XBYTES + W9_DBYTES)

struct W9Args {
    const char* x;       // (N,H,W,C)
    const char* dy;      // (N,H,W,K)
    const char* x2;      // optional second (x, dy) pair of the same shape: pixel tiles [tiles/2, tiles) read it, so the two
    const char* dy2;     //   applications of one layer in a step share one launch, one set of slabs and one reduce
    float* ws;           // [splits][9*C][K] f32 slabs
    int N, H, W, C, K, reflect;
    int tiles, tiles_per_split;   // tiles counts both pairs
    // Two NETWORKS of one shape in one launch (the cycle step's G_A->B beside G_B->A): splits [splits_per_net, 2 * splits_per_net)
    // belong to the second network and read xb / dyb / x2b / dy2b; each network then gets half the blocks, i.e. half the slabs
    // to write and to reduce for the same work per CU.  splits_per_net >= the grid's split count: one network.
    const char* xb; const char* dyb; const char* x2b; const char* dy2b;
    int splits_per_net;
};

// 16-byte chunk XOR key of halo row `row` (128-byte rows, two per 256-byte bank line): a transposing read touches rows
// {b..b+3, b+8..b+11} per 32-lane group; bits 0, 1 and 3 of the row index tell those eight apart for every b, bit 0
// already selects the half line, bits 1 and 3 pick one of the four 32-byte column pairs.
__device__ inline int w9_xkey(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }

// (streaming (nt) LDS-DMA of the x halo / the dy tiles: the step does not move, profiles/r04_nt_loads.txt)
__global__ __launch_bounds__(512) void conv3x3_wgrad_halo_kernel(W9Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages of { X halo [4][72][128 B], DY [128][256 B] }
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index as a scalar
    const int ct = wave & 3, kh = wave >> 2;             // wave: 16-channel slice of the 64, 64-cout half of the 128
    const int ktiles = a.K >> 7, otiles = (a.C >> 6) * ktiles;
    int lid;
    {
        const int b = (int)blockIdx.x, nm = (int)gridDim.x;
        const int q = nm >> 3, rr = nm & 7, xcd = b & 7;
        lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
    }
    const int split = lid / otiles, tl = lid - split * otiles;
    const int c0 = (tl / ktiles) * 64, n0 = (tl % ktiles) * 128;
    const bool netb = split >= a.splits_per_net;         // second network's blocks (uniform per block)
    const int nsplit = netb ? split - a.splits_per_net : split;
    const int t_beg = nsplit * a.tiles_per_split;
    const int t_end = min(a.tiles, t_beg + a.tiles_per_split);
    const int tilesW = a.W / W9_TW, tilesH = a.H >> 1;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);
    const char* const X1 = netb ? a.xb : a.x;
    const char* const D1 = netb ? a.dyb : a.dy;
    const char* const X2 = netb ? a.x2b : a.x2;
    const char* const D2 = netb ? a.dy2b : a.dy2;

    const int tiles1 = X2 ? a.tiles >> 1 : a.tiles;      // tiles of the first (x, dy) pair
    auto stage_tile = [&](int stg, int tt) {
        const bool second = tt >= tiles1;
        const int t = second ? tt - tiles1 : tt;
        const char* xs = second ? X2 : X1;
        const char* dys = second ? D2 : D1;
        const int tw = t % tilesW, rest = t / tilesW;
        const int th = rest % tilesH, n = rest / tilesH;
        const int h0 = th * 2, w0 = tw * W9_TW;
        char* sX = smem + stg * W9_STAGE;
        char* sD = sX + W9_XBYTES;
        // dy: 32 wave-instructions of 4 pixels x 256 B; wave w issues 4w..4w+3
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = wave * 4 + i;
            const int px = d * 4 + (lane >> 4), pos = lane & 15;
            const int key = wg2_key<bf16>(px) & 15;
            const int trow = px >> 6, tcol = px & 63;
            const char* src = dys + ((((size_t)n * a.H + h0 + trow) * a.W + w0 + tcol) * a.K + n0) * 2 + ((pos ^ key) << 4);
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sD + d * 1024));
        }
        // x halo: 36 wave-instructions of 8 pixels x 128 B (row k = q / 9, column group q % 9); wave w issues w, w+8, ...
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int q = wave + 8 * i;
            if (q >= 36) break;
            const int k = q / 9, cg = q - 9 * k;
            const int hp = cg * 8 + (lane >> 3), pos = lane & 7;
            const int key = w9_xkey(k * W9_PITCH + hp);
            int hi = h0 - 1 + k, wi = w0 - 1 + hp;
            bool ok = hp < W9_TW + 2;
            if (a.reflect) {
                hi = hi < 0 ? -hi : (hi >= a.H ? 2 * (a.H - 1) - hi : hi);
                wi = wi < 0 ? -wi : (wi >= a.W ? 2 * (a.W - 1) - wi : wi);
            } else ok = ok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            const char* src = ok ? xs + ((((size_t)n * a.H + hi) * a.W + wi) * a.C + c0) * 2 + ((pos ^ key) << 4) : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sX + (k * W9_PITCH + cg * 8) * 128));
        }
    };

    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, u = lane & 15, q4 = u >> 2, pp = u & 3;
    // Fragment addresses = stage base + compile-time constant + lane part.  The swizzle keys depend on the low 4 bits of
    // the row index only: for dy that is the lane's row within the 32-pixel step; for the halo it is (b + lane row) mod 16
    // with b mod 16 = 8 * (halo row parity) + tap column, i.e. six classes.
    int doff[4][2], xoff[6][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int L = 8 * g + q4 + 4 * h;
        const int kd = wg2_key<bf16>(L) & 15;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int col = kh * 64 + kt * 16 + 4 * pp;
            doff[kt][h] = L * 256 + (((col >> 3) ^ kd) << 4) + (col & 7) * 2;
        }
#pragma unroll
        for (int cls = 0; cls < 6; ++cls) {
            const int bl = (cls / 3) * 8 + (cls % 3);
            const int col = ct * 16 + 4 * pp;
            xoff[cls][h] = L * 128 + (((col >> 3) ^ w9_xkey(bl + L)) << 4) + (col & 7) * 2;
        }
    }
    if (t_beg < t_end) stage_tile(0, t_beg);
    SGG_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    for (int t = t_beg; t < t_end; ++t) {
        const int cur = (t - t_beg) & 1;
        if (t + 1 < t_end) stage_tile(cur ^ 1, t + 1);
        const char* bX = smem + cur * W9_STAGE;
        const char* bD = bX + W9_XBYTES;
        // lane-varying address parts are precomputed (xoff / doff); what changes per fragment is a compile-time constant
        auto ldD = [&](int kk, int kt) -> bf16x8 {      // dy fragment: 32 pixels of k32-step kk x 16 couts
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bD + kk * (32 * 256) + doff[kt][0]));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bD + kk * (32 * 256) + doff[kt][1]));
            return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        auto ldX = [&](int kk, int tap) -> bf16x8 {     // x fragment of tap (r, s): the same 32 pixels shifted in the halo
            const int r = tap / 3, sx = tap - 3 * r;
            const int b = ((kk >> 1) + r) * W9_PITCH + (kk & 1) * 32 + sx;       // first halo row of the fragment
            const int cls = ((((kk >> 1) + r) & 1) * 3) + sx;                     // b mod 16 = 8 * parity + sx
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bX + b * 128 + xoff[cls][0]));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bX + b * 128 + xoff[cls][1]));
            return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        // 36 steps (k32-step kk, tap) of 4 MFMAs; x fragments rotate through 3 registers sets and are fetched two steps
        // (128 MFMA cycles) ahead, the dy fragments of the next k32-step during the last taps of the current one
        bf16x8 fd[2][4], fx[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) fd[0][j] = ldD(0, j);
        fx[0] = ldX(0, 0);
        fx[1] = ldX(0, 1);
#pragma unroll
        for (int i = 0; i < 36; ++i) {
            const int kk = i / 9, tap = i - 9 * kk;
            if (i + 2 < 36) fx[(i + 2) % 3] = ldX((i + 2) / 9, (i + 2) % 9);
            if (tap >= 4 && tap < 8 && kk < 3) fd[(kk + 1) & 1][tap - 4] = ldD(kk + 1, tap - 4);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[tap][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[kk & 1][j], fx[i % 3], acc[tap][j], 0, 0, 0);
        }
        SGG_WAIT_VM0();
        SGG_WAIT_LGKM0();
        __builtin_amdgcn_s_barrier();
    }

    // D[row = cout][col = c]: lane (g,u) owns couts 4g..4g+3 of channel u -> one 16-byte store per tile
    float* slab = a.ws + (size_t)split * 9 * a.C * a.K;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const size_t mr = (size_t)tap * a.C + c0 + ct * 16 + u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = n0 + kh * 64 + j * 16 + g * 4;
            *reinterpret_cast<f32x4*>(slab + mr * a.K + k) = acc[tap][j];
        }
    }
}

// -------------------------------------------------------------------------------------------------
// The same for STRIDE 2 (c2 / c3 and, with the operand roles swapped, the Conv2DTranspose layers d1 / d2,
// module.py:236-242,254-260 backward).  One tap per block made these layers stream x nine times through L2
// (1.5 GB per launch at the c2 shape, 11.6 TB/s: L2-bound at 131 us).  Here a stage is one dy row segment of 64 pixels:
// the 3 x 129 input pixels it touches are staged once, de-interleaved by column parity (LDS slot = parity * 68 + column / 2),
// so that a tap's stride-2 walk over columns is a unit-stride walk over LDS rows and the transposing reads of
// conv3x3_wgrad_halo_kernel (and its swizzle) apply unchanged: tap column s reads plane s & 1 from row s >> 1.
// -------------------------------------------------------------------------------------------------
#define W9S_PITCH 136                                  // slots per halo row: 2 parity planes x 68 (65 / 64 used)
#define W9S_XBYTES (3 * W9S_PITCH * 128)               // 52224
#define W9S_DBYTES (64 * 256)                          // 16384
#define W9S_STAGE (W9S_XBYTES + W9S_DBYTES)

struct W9SArgs {
    const char* x;       // (N,H,W,C)
    const char* dy;      // (N,Ho,Wo,K)
    float* ws;           // [splits][9*C][K] f32 slabs
    int N, H, W, C, K, Ho, Wo, pad_t, pad_l;
    int tiles, tiles_per_split;
    // two NETWORKS of one shape in one launch (as W9Args): splits [splits_per_net, 2 * splits_per_net) read xb / dyb
    const char* xb; const char* dyb;
    int splits_per_net;
};

__global__ __launch_bounds__(512) void conv3x3_wgrad_halo_s2_kernel(W9SArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 stages of { X halo [3][136][128 B], DY [64][256 B] }
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = wave & 3, kh = wave >> 2;
    const int ktiles = a.K >> 7, otiles = (a.C >> 6) * ktiles;
    int lid;
    {
        const int b = (int)blockIdx.x, nm = (int)gridDim.x;
        const int q = nm >> 3, rr = nm & 7, xcd = b & 7;
        lid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (b >> 3);
    }
    const int split = lid / otiles, tl = lid - split * otiles;
    const int c0 = (tl / ktiles) * 64, n0 = (tl % ktiles) * 128;
    const bool netb = split >= a.splits_per_net;          // second network's blocks (uniform per block)
    const int nsplit = netb ? split - a.splits_per_net : split;
    const char* const ax = netb ? a.xb : a.x;
    const char* const ady = netb ? a.dyb : a.dy;
    const int t_beg = nsplit * a.tiles_per_split;
    const int t_end = min(a.tiles, t_beg + a.tiles_per_split);
    const int tilesW = a.Wo / 64;
    const char* zero = reinterpret_cast<const char*>(g_zero_page);

    auto stage_tile = [&](int stg, int t) {
        const int tw = t % tilesW, rest = t / tilesW;
        const int ho = rest % a.Ho, n = rest / a.Ho;
        const int w0 = tw * 64;
        char* sX = smem + stg * W9S_STAGE;
        char* sD = sX + W9S_XBYTES;
        // dy: 16 wave-instructions of 4 pixels x 256 B; wave w issues 2w, 2w+1
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int d = wave * 2 + i;
            const int px = d * 4 + (lane >> 4), pos = lane & 15;
            const int key = wg2_key<bf16>(px) & 15;
            const char* src = ady + ((((size_t)n * a.Ho + ho) * a.Wo + w0 + px) * a.K + n0) * 2 + ((pos ^ key) << 4);
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sD + d * 1024));
        }
        // x halo: 3 rows x 17 wave-instructions of 8 slots; wave w issues q = w, w+8, ...
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int q = wave + 8 * i;
            if (q >= 51) break;
            const int k = q / 17, sg = q - 17 * k;
            const int slot = sg * 8 + (lane >> 3), pos = lane & 7;      // 0..135
            const int plane = slot >= 68 ? 1 : 0, j = slot - 68 * plane;
            const int col = 2 * j + plane;                              // halo column 0..128
            const int key = w9_xkey(k * W9S_PITCH + slot);
            const int hi = 2 * ho - a.pad_t + k, wi = 2 * w0 - a.pad_l + col;
            const bool ok = col <= 128 && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
            const char* src = ok ? ax + ((((size_t)n * a.H + hi) * a.W + wi) * a.C + c0) * 2 + ((pos ^ key) << 4) : zero;
            dma16_to_lds(src, (__attribute__((address_space(3))) void*)(sX + (k * W9S_PITCH + sg * 8) * 128));
        }
    };

    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, u = lane & 15, q4 = u >> 2, pp = u & 3;
    // lane parts of the fragment addresses; halo classes by (b mod 16) = 8 * (r & 1) + 4 * (s & 1) + (s >> 1)
    int doff[4][2], xoff[6][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int L = 8 * g + q4 + 4 * h;
        const int kd = wg2_key<bf16>(L) & 15;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int col = kh * 64 + kt * 16 + 4 * pp;
            doff[kt][h] = L * 256 + (((col >> 3) ^ kd) << 4) + (col & 7) * 2;
        }
#pragma unroll
        for (int cls = 0; cls < 6; ++cls) {
            const int sx = cls % 3;
            const int bl = (cls / 3) * 8 + (sx & 1) * 4 + (sx >> 1);
            const int col = ct * 16 + 4 * pp;
            xoff[cls][h] = L * 128 + (((col >> 3) ^ w9_xkey(bl + L)) << 4) + (col & 7) * 2;
        }
    }
    if (t_beg < t_end) stage_tile(0, t_beg);
    SGG_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    for (int t = t_beg; t < t_end; ++t) {
        const int cur = (t - t_beg) & 1;
        if (t + 1 < t_end) stage_tile(cur ^ 1, t + 1);
        const char* bX = smem + cur * W9S_STAGE;
        const char* bD = bX + W9S_XBYTES;
        auto ldD = [&](int kk, int kt) -> bf16x8 {
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bD + kk * (32 * 256) + doff[kt][0]));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bD + kk * (32 * 256) + doff[kt][1]));
            return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        auto ldX = [&](int kk, int tap) -> bf16x8 {     // 32 dy pixels kk*32.. of the row <-> input columns 2*px + s, row r
            const int r = tap / 3, sx = tap - 3 * r;
            const int b = r * W9S_PITCH + (sx & 1) * 68 + (sx >> 1) + kk * 32;   // first LDS row of the fragment
            const int cls = (r & 1) * 3 + sx;
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bX + b * 128 + xoff[cls][0]));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(bX + b * 128 + xoff[cls][1]));
            return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        };
        // 18 steps (k32-step kk, tap) of 4 MFMAs; x fragments rotate through 3 register sets, fetched two steps ahead
        bf16x8 fd[2][4], fx[3];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 4; ++j) fd[kk][j] = ldD(kk, j);
        fx[0] = ldX(0, 0);
        fx[1] = ldX(0, 1);
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            const int kk = i / 9, tap = i - 9 * kk;
            if (i + 2 < 18) fx[(i + 2) % 3] = ldX((i + 2) / 9, (i + 2) % 9);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[tap][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd[kk][j], fx[i % 3], acc[tap][j], 0, 0, 0);
        }
        SGG_WAIT_VM0();
        SGG_WAIT_LGKM0();
        __builtin_amdgcn_s_barrier();
    }

    float* slab = a.ws + (size_t)split * 9 * a.C * a.K;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const size_t mr = (size_t)tap * a.C + c0 + ct * 16 + u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = n0 + kh * 64 + j * 16 + g * 4;
            *reinterpret_cast<f32x4*>(slab + mr * a.K + k) = acc[tap][j];
        }
    }
}

// -------------------------------------------------------------------------------------------------
// Host layer: the shape predicates and split rules of the kernels above, ONE plan per descriptor, the launchers.
// -------------------------------------------------------------------------------------------------
static bool w9s_ok(const sgg_conv_desc* d) {
    const int en = sgg_config().w9s2;
    if (!en || d->dtype != SGG_BF16 || d->pad_mode != SGG_PAD_ZERO) return false;
    if (d->R != 3 || d->S != 3 || d->stride != 2 || d->H != 2 * d->Ho || d->W != 2 * d->Wo) return false;
    if ((unsigned)d->pad_t > 1u || (unsigned)d->pad_l > 1u) return false;
    // K >= 256 layers (c3 / d1) already run the 256x256 DMA kernel at the same speed (72 us); this kernel is for the
    // 64 <-> 128 channel layers at full resolution, which were L2-bound at 131 us (89 us here)
    if (d->K >= 256 && d->R * d->S * d->C >= 256) return false;
    return d->Wo % 64 == 0 && d->C % 64 == 0 && d->K % 128 == 0;
}
// splits of an all-taps kernel's T pixel tiles: ~256 blocks in all over the 64 x 128 output tiles, at most `cap`, none empty
static int w9_split_rule(const sgg_conv_desc* d, int T, int cap) {
    const int otiles = (d->C / 64) * (d->K / 128);
    int sp = otiles >= 256 ? 1 : 256 / otiles;
    if (sp > T) sp = T;
    if (sp > cap) sp = cap;
    const int tps = (T + sp - 1) / sp;
    return (T + tps - 1) / tps;
}
static int w9s_tiles(const sgg_conv_desc* d) { return d->N * d->Ho * (d->Wo / 64); }
static int w9s_splits(const sgg_conv_desc* d) { return w9_split_rule(d, w9s_tiles(d), 256); }

bool w9_ok(const sgg_conv_desc* d) {
    const int en = sgg_config().w9;
    if (!en || d->dtype != SGG_BF16) return false;
    if (d->R != 3 || d->S != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 || d->Ho != d->H || d->Wo != d->W) return false;
    return d->W % W9_TW == 0 && d->H % 2 == 0 && d->C % 64 == 0 && d->K % 128 == 0;
}
static int w9_tiles(const sgg_conv_desc* d) { return d->N * (d->H / 2) * (d->W / W9_TW); }
// the split count depends on the single-pair tile count only, so a paired launch needs the same workspace
static int w9_splits(const sgg_conv_desc* d) { return w9_split_rule(d, w9_tiles(d), 64); }
bool w9_pair2_ok(const sgg_conv_desc* d) { return w9_ok(d) && !(w9_splits(d) & 1); }   // each network takes half the splits

// What a descriptor's weight gradient runs as.  run_wgrad switches on it and checks its workspace against it, the workspace
// query returns its bytes, sgg_conv2d_route() / sgg_deconv2d_route() its route.
struct WgradPlan {
    int route;           // the kernel (an sgg_route)
    int slabs;           // f32 partial results a single call has room for (the generic kernels round a slab's pixel range up to 64
                         // pixels and may then fill fewer; every other kernel writes exactly these)
    size_t slab_bytes;   // one of them
    size_t ws_bytes;     // workspace of a single call: the slabs (W7 stem: and the padded copy of x); two networks: twice that
};
// Cr: the real input channel count (the vector-ALU kernel of the 8-channel stride-2 layer holds four channels per pixel); 0 where
// the caller does not know it (the workspace and route queries): C_real <= 4 is assumed there, see include/sggan.h.
static WgradPlan plan_wgrad(const sgg_conv_desc* d, int Cr) {
    const bool bf = d->dtype == SGG_BF16;
    const int64_t P = (int64_t)d->N * d->Ho * d->Wo;
    WgradPlan p;
    p.slab_bytes = (size_t)d->R * d->S * d->C * d->K * sizeof(float);
    if (conv7_head_ok(d) || conv7_stem_ok(d)) {         // the two 7x7 layers with a 3-channel side
        const W7Plan w = w7_plan(d, conv7_stem_ok(d));
        p.route = SGG_ROUTE_W7; p.slabs = w.blocks; p.slab_bytes = 7 * 64 * 32 * sizeof(float);
        p.ws_bytes = w.slab_bytes + w.xpad_bytes;
        return p;
    }
    if (halo_wgrad_ok(d)) { p.route = SGG_ROUTE_HALO_WGRAD; p.slabs = halo_wgrad_blocks(d); }   // one slab per persistent block
    else if (w9_ok(d)) { p.route = SGG_ROUTE_W9; p.slabs = w9_splits(d); }                      // 3x3 s1: x halo resident, all taps per block
    else if (w9s_ok(d)) { p.route = SGG_ROUTE_W9S; p.slabs = w9s_splits(d); }                   // 3x3 s2: the same with a parity-de-interleaved halo
    else if (s2n_wgrad_ok(d) && Cr <= 4) { p.route = SGG_ROUTE_S2N; p.slabs = s2n_wgrad_grid(d).blocks; }   // D.h0: the vector-ALU kernel, one slab per block
    else if (d->K >= 256 && d->R * d->S * d->C >= 256) {   // the LDS-DMA kernel, one 8-wave block per CU: ~256 blocks in all
        const int bkp = bf ? 64 : 32;                                   // pixels per stage (BKP in the kernel)
        p.route = sgg_config().wgrad_rowfast && d->Wo % bkp == 0 ? SGG_ROUTE_WGRAD_V2_ROWFAST : SGG_ROUTE_WGRAD_V2;
        int64_t tiles = (int64_t)((d->R * d->S * d->C + 255) / 256) * ((d->K + 255) / 256);
        int64_t sp = 256 / tiles, maxs = (P + 127) / 128;
        if (sp > maxs) sp = maxs;
        if (sp < 1) sp = 1;
        if (sp > 64) sp = 64;
        p.slabs = (int)sp;
    } else {
        p.route = d->K >= 128 ? SGG_ROUTE_WGRAD_128x128 : (d->K > 16 ? SGG_ROUTE_WGRAD_128x64 : SGG_ROUTE_WGRAD_128x16);
        int bnw = d->K >= 128 ? 128 : (d->K > 16 ? 64 : 16);
        int64_t tiles = (int64_t)((d->R * d->S * d->C + 127) / 128) * ((d->K + bnw - 1) / bnw);
        int64_t want = (1024 + tiles - 1) / tiles;                 // ~4 blocks per CU
        int64_t maxs = (P + 255) / 256;                            // >= 256 pixels per split
        int64_t sp = want < maxs ? want : maxs;
        int64_t cap = (int64_t)p.slab_bytes <= (1 << 20) ? 256 : 64;   // small slabs: the reduce pass stays cheap
        if (sp < 1) sp = 1;
        if (sp > cap) sp = cap;
        p.slabs = (int)sp;
        // An S2N shape with more than 4 real input channels lands here (K = 64: the 128x64 tile) and keeps the S2N block count as
        // its slab count instead of the rule above: the workspace query cannot know Cr, so it reports the S2N bytes, and a call
        // must run with what the query reports whichever kernel it takes.
        if (s2n_wgrad_ok(d)) p.slabs = s2n_wgrad_grid(d).blocks;
    }
    p.ws_bytes = (size_t)p.slabs * p.slab_bytes;
    return p;
}
int wgrad_route(const sgg_conv_desc* d) { return plan_wgrad(d, 0).route; }
size_t wgrad_ws_bytes(const sgg_conv_desc* d) { return plan_wgrad(d, 0).ws_bytes; }

// dw (+)= the sum of its `spn` slabs at ws; nets == 2: dwb likewise from the spn slabs behind them, in the same launch
static int launch_wgrad_reduce(const void* ws, float* dw, float* dwb, int taps, int C, int K, int Cr, int Kr, int spn, int nets, int accumulate, hipStream_t s) {
    int64_t total = (int64_t)taps * Cr * (K / 4) * nets;
    int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)ws, dw, taps, C, K, Cr, Kr, spn, accumulate, nets == 2 ? dwb : (float*)nullptr);
    return sgg_check_launch();
}

// The two all-taps 3x3 kernels with two NETWORKS of one layer shape: ONE launch of the single call's grid in which each network
// gets half the blocks, i.e. half the slabs.  The split slabs are these kernels' main cost next to the operands -- 75 MB written
// and 75 MB read again per network at the generator's four stride-2 layers, for 67 MB of x and dy, and as much at D.h3 -- so two
// launches pay them twice.  Half the slabs = another f32 summation order than the single call's: the result equals two single
// calls up to that order (1e-6 relative), not bit for bit.

// 3x3 s1.  One network (nb == nullptr), or two sharing the launch: an odd split count has no such form (SGG_EUNSUPPORTED).
// Workspace as for a single call in both forms.
int run_w9(const sgg_conv_desc* d, const W9Net& na, const W9Net* nb, int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, hipStream_t s) {
    const WgradPlan p = plan_wgrad(d, Cr);
    const int sp = p.slabs;
    if (nb && (sp & 1)) return SGG_EUNSUPPORTED;
    if (ws_bytes < p.ws_bytes || !ws) return SGG_EWORKSPACE;
    const int spn = nb ? sp / 2 : sp;                    // slabs per network
    W9Args w;
    w.x = (const char*)na.x; w.dy = (const char*)na.dy; w.x2 = (const char*)na.x2; w.dy2 = (const char*)na.dy2; w.ws = (float*)ws;
    w.xb = w.dyb = w.x2b = w.dy2b = nullptr;
    if (nb) { w.xb = (const char*)nb->x; w.dyb = (const char*)nb->dy; w.x2b = (const char*)nb->x2; w.dy2b = (const char*)nb->dy2; }
    w.splits_per_net = spn;
    w.N = d->N; w.H = d->H; w.W = d->W; w.C = d->C; w.K = d->K; w.reflect = d->pad_mode == SGG_PAD_REFLECT;
    w.tiles = w9_tiles(d) * (na.x2 ? 2 : 1);
    w.tiles_per_split = (w.tiles + spn - 1) / spn;
    SGG_LDS_ATTR(conv3x3_wgrad_halo_kernel, 2 * W9_STAGE);
    sgg_launch_timed(conv3x3_wgrad_halo_kernel, dim3((unsigned)(sp * (d->C / 64) * (d->K / 128))), dim3(512), (unsigned)(2 * W9_STAGE), s, w);
    int rc = sgg_check_launch();
    if (rc) return rc;
    return launch_wgrad_reduce(ws, na.dw, nb ? nb->dw : nullptr, 9, d->C, d->K, Cr, Kr, spn, nb ? 2 : 1, accumulate, s);
}

// 3x3 s2.  Two networks share the launch from two splits on (an odd count leaves one slab unused); with a single split each
// network gets a launch and a slab of its own.  One reduce launch in every form.
static int run_w9s(const sgg_conv_desc* d, const WgradPlan& p, const void* x, const void* dy, float* dw, const void* xb, const void* dyb, float* dwb,
                   int Cr, int Kr, int accumulate, void* ws, hipStream_t s) {
    const bool merged = xb && p.slabs >= 2;
    const int spn = merged ? p.slabs / 2 : p.slabs;      // slabs per network
    const int sp = merged ? 2 * spn : spn;               // ... per launch
    W9SArgs w;
    w.x = (const char*)x; w.dy = (const char*)dy; w.ws = (float*)ws;
    w.xb = (const char*)(merged ? xb : x); w.dyb = (const char*)(merged ? dyb : dy); w.splits_per_net = merged ? spn : (1 << 30);
    w.N = d->N; w.H = d->H; w.W = d->W; w.C = d->C; w.K = d->K; w.Ho = d->Ho; w.Wo = d->Wo; w.pad_t = d->pad_t; w.pad_l = d->pad_l;
    w.tiles = w9s_tiles(d); w.tiles_per_split = (w.tiles + spn - 1) / spn;
    SGG_LDS_ATTR(conv3x3_wgrad_halo_s2_kernel, 2 * W9S_STAGE);
    const dim3 grid((unsigned)(sp * (d->C / 64) * (d->K / 128)));
    hipLaunchKernelGGL(conv3x3_wgrad_halo_s2_kernel, grid, dim3(512), 2 * W9S_STAGE, s, w);
    if (xb && !merged) {
        w.x = (const char*)xb; w.dy = (const char*)dyb; w.ws = (float*)((char*)ws + (size_t)spn * p.slab_bytes);
        hipLaunchKernelGGL(conv3x3_wgrad_halo_s2_kernel, grid, dim3(512), 2 * W9S_STAGE, s, w);
    }
    int rc = sgg_check_launch();
    if (rc) return rc;
    return launch_wgrad_reduce(ws, dw, dwb, 9, d->C, d->K, Cr, Kr, spn, xb ? 2 : 1, accumulate, s);
}

template <typename T, int BMW, int BNW, int WGM>
static int launch_wgrad_cfg(WgradArgs& a, int splits, hipStream_t s) {
    constexpr size_t lds = 2 * 32 * (BMW + BNW) * sizeof(T);
    auto kern = conv_wgrad_kernel<T, BMW, BNW, WGM>;
    SGG_LDS_ATTR(kern, (int)lds);
    int Mrows = a.R * a.S * a.C;
    dim3 grid((unsigned)((Mrows + BMW - 1) / BMW), (unsigned)((a.K + BNW - 1) / BNW), (unsigned)splits);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
    return sgg_check_launch();
}

// The routes whose kernels take WgradArgs and exist in both dtypes: HALO_WGRAD, S2N, the LDS-DMA kernel and the three generic tiles.
// A second network's main kernel runs right after the first one's into the slabs behind them, and ONE reduce launch sums both
// sets, each in the single call's order: bit-identical results.  (The LDS-DMA kernel shares the launch instead, see below.)
template <typename T>
static int run_wgrad_slabs(const sgg_conv_desc* d, const WgradPlan& p, const void* x, const void* dy, float* dw, const void* xb, const void* dyb, float* dwb,
                           int Cr, int Kr, int accumulate, void* ws, hipStream_t s) {
    const int nets = xb ? 2 : 1, taps = d->R * d->S;
    WgradArgs a;
    a.x = (const char*)x; a.dy = (const char*)dy; a.ws = (float*)ws;
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->C; a.K = d->K; a.R = d->R; a.S = d->S; a.stride = d->stride;
    a.pad_t = d->pad_t; a.pad_l = d->pad_l; a.Ho = d->Ho; a.Wo = d->Wo; a.reflect = d->pad_mode == SGG_PAD_REFLECT;
    a.P = d->N * d->Ho * d->Wo;
    a.xb = a.x; a.dyb = a.dy; a.splits_per_net = 1 << 30;
    int splits = p.slabs;
    const bool halo = p.route == SGG_ROUTE_HALO_WGRAD, s2n = p.route == SGG_ROUTE_S2N;   // persistent blocks, one slab each: no pixel split
    const bool v2 = p.route == SGG_ROUTE_WGRAD_V2_ROWFAST || p.route == SGG_ROUTE_WGRAD_V2;
    // grouped call of the LDS-DMA kernel: one launch, half the splits (= slabs: 8 MB each at D.h31) per network -- as for the
    // all-taps 3x3 kernels above; equal to two single calls up to f32 summation order
    const bool merged = xb && v2 && splits >= 2;
    if (merged) splits /= 2;
    a.pix_per_split = halo ? 0 : (int)align_up((size_t)((a.P + splits - 1) / splits), 64);
    if (!halo && !s2n) splits = (a.P + a.pix_per_split - 1) / a.pix_per_split;   // (never more than before: the plan's workspace holds them)
    a.dHW = make_fastdiv(halo ? 1u : (uint32_t)(d->Ho * d->Wo)); a.dW = make_fastdiv(halo ? 1u : (uint32_t)d->Wo);
    const size_t need = (size_t)splits * p.slab_bytes;
    int rc = SGG_OK;
    if (merged) { a.xb = (const char*)xb; a.dyb = (const char*)dyb; a.splits_per_net = splits; }
    for (int net = 0; net < (merged ? 1 : nets) && rc == SGG_OK; ++net) {
    if (net) { a.x = (const char*)xb; a.dy = (const char*)dyb; a.ws = (float*)((char*)ws + need); }
    switch (p.route) {
    case SGG_ROUTE_HALO_WGRAD: {
        size_t lds = 512 * 16 * sizeof(T) + (size_t)(HALO_TH + d->R - 1) * (HALO_TW + d->S - 1) * 128 + 1024;
        auto kern = conv_halo_wgrad_kernel<T>;
        SGG_LDS_ATTR(kern, 160 * 1024);
        hipLaunchKernelGGL(kern, dim3(splits), dim3(512), lds, s, a, d->N * (d->H / HALO_TH) * (d->W / HALO_TW));
        rc = sgg_check_launch();
        break;
    }
    case SGG_ROUTE_S2N: rc = launch_s2n_wgrad(d, a.x, a.dy, a.ws, Cr, s); break;
    case SGG_ROUTE_WGRAD_V2_ROWFAST:
    case SGG_ROUTE_WGRAD_V2: {
        constexpr size_t lds = 2 * 2 * (size_t)(sizeof(T) == 2 ? 64 : 32) * 256 * sizeof(T);
        SGG_LDS_ATTR((conv_wgrad_glds_kernel<T, false>), lds);
        SGG_LDS_ATTR((conv_wgrad_glds_kernel<T, true>), lds);
        dim3 grid((unsigned)(((d->R * d->S * d->C + 255) / 256) * ((d->K + 255) / 256) * splits * (merged ? 2 : 1)));
        if (p.route == SGG_ROUTE_WGRAD_V2_ROWFAST) hipLaunchKernelGGL((conv_wgrad_glds_kernel<T, true>), grid, dim3(512), lds, s, a);
        else hipLaunchKernelGGL((conv_wgrad_glds_kernel<T, false>), grid, dim3(512), lds, s, a);
        rc = sgg_check_launch();
        break;
    }
    case SGG_ROUTE_WGRAD_128x128: rc = launch_wgrad_cfg<T, 128, 128, 2>(a, splits, s); break;
    case SGG_ROUTE_WGRAD_128x64: rc = launch_wgrad_cfg<T, 128, 64, 4>(a, splits, s); break;
    case SGG_ROUTE_WGRAD_128x16: rc = launch_wgrad_cfg<T, 128, 16, 4>(a, splits, s); break;
    default: rc = SGG_EUNSUPPORTED; break;               // (run_wgrad sends nothing else here)
    }
    }
    if (rc) return rc;
    if (s2n) {
        const int outs = taps * Cr * (d->K / 4);
        hipLaunchKernelGGL(wgrad_reduce_wide_kernel, dim3((unsigned)((outs + 3) / 4), (unsigned)nets), dim3(256), 0, s, (const float*)ws, dw, dwb,
                           taps, d->C, d->K, Cr, Kr, splits, accumulate);
        return sgg_check_launch();
    }
    return launch_wgrad_reduce(ws, dw, dwb, taps, d->C, d->K, Cr, Kr, splits, nets, accumulate, s);
}

int run_wgrad(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, hipStream_t s,
              const void* xb, const void* dyb, float* dwb) {
    const WgradPlan p = plan_wgrad(d, Cr);
    if (!ws || ws_bytes < p.ws_bytes * (xb ? 2 : 1)) return SGG_EWORKSPACE;
    switch (p.route) {
    case SGG_ROUTE_W7: {                                 // the second network's launches follow the first one's, in the same workspace
        const bool stem = conv7_stem_ok(d);
        int rc = run_w7(d, stem, x, dy, dw, Cr, Kr, accumulate, ws, ws_bytes, s);
        return (rc || !xb) ? rc : run_w7(d, stem, xb, dyb, dwb, Cr, Kr, accumulate, ws, ws_bytes, s);
    }
    case SGG_ROUTE_W9: {
        const W9Net first{x, dy, nullptr, nullptr, dw}, second{xb, dyb, nullptr, nullptr, dwb};
        if (!xb) return run_w9(d, first, nullptr, Cr, Kr, accumulate, ws, ws_bytes, s);
        if (w9_pair2_ok(d)) return run_w9(d, first, &second, Cr, Kr, accumulate, ws, ws_bytes, s);
        int rc = run_w9(d, first, nullptr, Cr, Kr, accumulate, ws, ws_bytes, s);          // odd split count: one after the other
        return rc ? rc : run_w9(d, second, nullptr, Cr, Kr, accumulate, ws, ws_bytes, s);
    }
    case SGG_ROUTE_W9S: return run_w9s(d, p, x, dy, dw, xb, dyb, dwb, Cr, Kr, accumulate, ws, s);
    default:
        return d->dtype == SGG_BF16 ? run_wgrad_slabs<bf16>(d, p, x, dy, dw, xb, dyb, dwb, Cr, Kr, accumulate, ws, s)
                                    : run_wgrad_slabs<float>(d, p, x, dy, dw, xb, dyb, dwb, Cr, Kr, accumulate, ws, s);
    }
}

#ifdef SGG_LAB
int wgrad_debug_occupancy() {
    int v = 0;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, conv_wgrad_kernel<bf16, 128, 128, 2>, 256, 32768);
    return v;
}
#endif
