// resample.hip -- the input pipeline's image resample (utils.py:167-233: imread -> resize -> resize -> fliplr) as ONE kernel over
// device-resident uint8 sources.  Both skimage resize stages (Gaussian anti-alias + linear interpolation) are linear and
// separable, so the host folds the whole chain into one banded matrix per axis (sggan_amd/data.py: band_table); the kernel
// applies   out[n,i,j,c] = ( sum_kr rw[i][kr] * ( sum_kc cw[j'][kc] * src[index[n], rs[i]+kr, cs[j']+kc, c] ) ) / 255,
// j' = flip[n] ? W-1-j : j, and writes the step's internal layout (channels padded to SGG_CPAD, network dtype).
//
// One block = 8 output rows x up to 256 output columns of one sample; thread t owns table column jt0 + t.  The source rows the
// band needs are staged RQ at a time into LDS as raw bytes with 16-byte loads (each source byte is read once per band; bands
// overlap by taps - step rows, which L2 absorbs); every thread reduces its column window of each staged row (the horizontally
// reduced value lives in registers) and adds it into the output rows it belongs to.  The tile's column weights sit in LDS
// transposed ([kc][t]: conflict free).  Summation order is fixed -- kc ascending inside a row, source rows ascending -- and does
// not depend on the tiling.  Every table-derived coordinate is clamped to the source / the staged window, so a malformed table
// gives wrong pixels, never an out-of-range access.
#include "common.h"
#include <algorithm>

namespace {

constexpr int RS_RB = 8;          // output rows per block
constexpr int RS_RQ = 8;          // source rows staged per chunk (at most)
constexpr int RS_CB = 256;        // output columns per block = threads
constexpr int RS_LDS = 64 * 1024; // dynamic LDS budget (the default limit: no attribute call needed)

struct ResampleArgs {
    const uint8_t* src; int64_t src_bytes; int M, H0, W0;
    const int32_t* index; const int32_t* flip;
    const float* rw; const int32_t* rs; int TR;
    const float* cw; const int32_t* cs; int TC;
    void* out; int N, H, W, C;
    int rq;            // source rows per chunk
    int seg;           // LDS bytes per staged row (multiple of 16)
    int span_cap;      // source pixels per staged row the LDS window holds
    int wstride;       // columns per row of the LDS weight tile (min(W, 256) rounded up to a wave)
};

template <typename T> __device__ inline void store_pixel(T* p, const float (&v)[4], int C);
template <> __device__ inline void store_pixel<float>(float* p, const float (&v)[4], int C) {
    float4 a = make_float4(v[0], C > 1 ? v[1] : 0.f, C > 2 ? v[2] : 0.f, C > 3 ? v[3] : 0.f);
    reinterpret_cast<float4*>(p)[0] = a;
    reinterpret_cast<float4*>(p)[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}
template <> __device__ inline void store_pixel<bf16>(bf16* p, const float (&v)[4], int C) {
    bf16x8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (bf16)0.0f;
    o[0] = (bf16)v[0];                                  // RNE
    if (C > 1) o[1] = (bf16)v[1];
    if (C > 2) o[2] = (bf16)v[2];
    if (C > 3) o[3] = (bf16)v[3];
    *reinterpret_cast<bf16x8*>(p) = o;
}

template <int CS, typename T>
__global__ __launch_bounds__(RS_CB) void resample_u8_kernel(const ResampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x;
    const int n = blockIdx.z;
    const int i0 = blockIdx.y * RS_RB;
    const int jt0 = blockIdx.x * RS_CB;
    const int ncol = min(RS_CB, a.W - jt0);
    const int nrow = min(RS_RB, a.H - i0);
    const int TR = a.TR, TC = a.TC;
    const int sidx = min(max(a.index[n], 0), a.M - 1);
    const bool flip = a.flip[n] != 0;

    const bool active = t < ncol;
    float* wl = reinterpret_cast<float*>(lds);                    // [TC][wstride] column weights of the tile
    uint8_t* stage = lds + (size_t)TC * a.wstride * sizeof(float);   // [rq][seg] raw source bytes

    // staged column window [x_lo, x_lo + span) in source pixels
    const int x_lo = min(max(a.cs[jt0], 0), a.W0 - 1);
    int x_hi = min(a.cs[jt0 + ncol - 1] + TC, a.W0);
    const int span = min(max(x_hi - x_lo, 1), a.span_cap);
    const int jt = jt0 + min(t, ncol - 1);
    const int px0 = min(max(a.cs[jt] - x_lo, 0), span - 1);       // this thread's first source pixel inside the window
    if (active)
        for (int kc = 0; kc < TC; ++kc) wl[kc * a.wstride + t] = a.cw[(size_t)jt * TC + kc];

    // source rows of the band
    const int r_lo = min(max(a.rs[i0], 0), a.H0 - 1);
    const int r_hi = min(a.rs[i0 + nrow - 1] + TR, a.H0);
    int rs_i[RS_RB];
#pragma unroll
    for (int i = 0; i < RS_RB; ++i) rs_i[i] = a.rs[min(i0 + i, a.H - 1)];

    float acc[RS_RB][4];
#pragma unroll
    for (int i = 0; i < RS_RB; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;

    const int64_t img_base = (int64_t)sidx * a.H0;
    const int chunks = (span * CS + 15 + 15) / 16;                // 16-byte pieces that cover any alignment of the window
    for (int rb = r_lo; rb < r_hi; rb += a.rq) {
        const int nq = min(a.rq, r_hi - rb);
        __syncthreads();                                          // previous chunk consumed (first pass: weights written)
        for (int e = t; e < nq * chunks; e += RS_CB) {
            const int q = e / chunks, ch = e - q * chunks;
            const int64_t off = ((img_base + rb + q) * a.W0 + x_lo) * CS;      // byte offset of the window's first pixel
            const int64_t g = ((off + (int64_t)(uintptr_t)a.src) & ~(int64_t)15) - (int64_t)(uintptr_t)a.src + (int64_t)ch * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g >= 0 && g + 16 <= a.src_bytes) {
                v = *reinterpret_cast<const uint4*>(a.src + g);
            } else {                                              // the piece straddles an end of the buffer: byte by byte, guarded
                uint8_t* b = reinterpret_cast<uint8_t*>(&v);
                for (int k = 0; k < 16; ++k)
                    if (g + k >= 0 && g + k < a.src_bytes) b[k] = a.src[g + k];
            }
            *reinterpret_cast<uint4*>(stage + (size_t)q * a.seg + ch * 16) = v;
        }
        __syncthreads();
        // horizontal pass: h[q][c] for this thread's column, weights read once per tap
        float h[RS_RQ][4];
#pragma unroll
        for (int q = 0; q < RS_RQ; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) h[q][c] = 0.f;
        int shift[RS_RQ];
#pragma unroll
        for (int q = 0; q < RS_RQ; ++q) {
            const int64_t off = ((img_base + rb + q) * a.W0 + x_lo) * CS;
            shift[q] = (int)((off + (int64_t)(uintptr_t)a.src) & 15) + q * a.seg;
        }
        for (int kc = 0; active && kc < TC; ++kc) {
            const float w = wl[kc * a.wstride + t];
            const int pb = min(px0 + kc, span - 1) * CS;
#pragma unroll
            for (int q = 0; q < RS_RQ; ++q) {
                if (q < nq) {
                    const uint8_t* p = stage + shift[q] + pb;
                    if (CS == 4) {
                        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);     // 4-byte pixels stay 4-byte aligned
                        h[q][0] = fmaf(w, (float)(u & 255u), h[q][0]);
                        h[q][1] = fmaf(w, (float)((u >> 8) & 255u), h[q][1]);
                        h[q][2] = fmaf(w, (float)((u >> 16) & 255u), h[q][2]);
                        h[q][3] = fmaf(w, (float)(u >> 24), h[q][3]);
                    } else {
                        h[q][0] = fmaf(w, (float)p[0], h[q][0]);
                        h[q][1] = fmaf(w, (float)p[1], h[q][1]);
                        h[q][2] = fmaf(w, (float)p[2], h[q][2]);
                    }
                }
            }
        }
        // vertical pass: source row rb + q is tap k = rb + q - rs[i] of output row i
#pragma unroll
        for (int q = 0; q < RS_RQ; ++q) {
            if (active && q < nq) {
#pragma unroll
                for (int i = 0; i < RS_RB; ++i) {
                    const int k = rb + q - rs_i[i];
                    if (i < nrow && k >= 0 && k < TR) {
                        const float w = a.rw[(size_t)(i0 + i) * TR + k];
#pragma unroll
                        for (int c = 0; c < CS; ++c) acc[i][c] = fmaf(w, h[q][c], acc[i][c]);
                    }
                }
            }
        }
    }
    if (active) {
        const int j = flip ? a.W - 1 - (jt0 + t) : jt0 + t;
#pragma unroll
        for (int i = 0; i < RS_RB; ++i) {
            if (i < nrow) {
                float v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = acc[i][c] / 255.0f;
                store_pixel<T>(reinterpret_cast<T*>(a.out) + (((int64_t)n * a.H + i0 + i) * a.W + j) * SGG_CPAD, v, a.C);
            }
        }
    }
}

// The same band resample over an f32 source (N, H0, W0, 4) -- the warp's intermediate (warp.hip) -- for the augmented copy:
// sample n of the source becomes sample n of the output, values are taken as they are (no / 255), and consecutive output
// samples lie out_stride elements apart so that the copies can be written between the plain samples of a doubled batch.
// Same tiling and the same summation order as resample_u8_kernel; a staged row is span float4 pixels, always aligned.
struct ResampleF32Args {
    const float4* src; int H0, W0;
    const int32_t* flip;
    const float* rw; const int32_t* rs; int TR;
    const float* cw; const int32_t* cs; int TC;
    void* out; int64_t out_stride; int N, H, W, C;
    int rq;            // source rows per chunk
    int span_cap;      // source pixels per staged row the LDS window holds
    int wstride;       // columns per row of the LDS weight tile
};

template <typename T>
__global__ __launch_bounds__(RS_CB) void resample_f32_kernel(const ResampleF32Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x;
    const int n = blockIdx.z;
    const int i0 = blockIdx.y * RS_RB;
    const int jt0 = blockIdx.x * RS_CB;
    const int ncol = min(RS_CB, a.W - jt0);
    const int nrow = min(RS_RB, a.H - i0);
    const int TR = a.TR, TC = a.TC;
    const bool flip = a.flip[n] != 0;

    const bool active = t < ncol;
    float* wl = reinterpret_cast<float*>(lds);                                                    // [TC][wstride]
    float4* stage = reinterpret_cast<float4*>(lds + (size_t)TC * a.wstride * sizeof(float));      // [rq][span_cap]

    const int x_lo = min(max(a.cs[jt0], 0), a.W0 - 1);
    const int x_hi = min(a.cs[jt0 + ncol - 1] + TC, a.W0);
    const int span = min(max(x_hi - x_lo, 1), a.span_cap);
    const int jt = jt0 + min(t, ncol - 1);
    const int px0 = min(max(a.cs[jt] - x_lo, 0), span - 1);
    if (active)
        for (int kc = 0; kc < TC; ++kc) wl[kc * a.wstride + t] = a.cw[(size_t)jt * TC + kc];

    const int r_lo = min(max(a.rs[i0], 0), a.H0 - 1);
    const int r_hi = min(a.rs[i0 + nrow - 1] + TR, a.H0);
    int rs_i[RS_RB];
#pragma unroll
    for (int i = 0; i < RS_RB; ++i) rs_i[i] = a.rs[min(i0 + i, a.H - 1)];

    float acc[RS_RB][4];
#pragma unroll
    for (int i = 0; i < RS_RB; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;

    const int64_t img_base = (int64_t)n * a.H0;
    for (int rb = r_lo; rb < r_hi; rb += a.rq) {
        const int nq = min(a.rq, r_hi - rb);
        __syncthreads();
        for (int e = t; e < nq * span; e += RS_CB) {
            const int q = e / span, px = e - q * span;
            stage[q * a.span_cap + px] = a.src[(img_base + rb + q) * a.W0 + x_lo + px];
        }
        __syncthreads();
        float h[RS_RQ][4];
#pragma unroll
        for (int q = 0; q < RS_RQ; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) h[q][c] = 0.f;
        for (int kc = 0; active && kc < TC; ++kc) {
            const float w = wl[kc * a.wstride + t];
            const int pb = min(px0 + kc, span - 1);
#pragma unroll
            for (int q = 0; q < RS_RQ; ++q) {
                if (q < nq) {
                    const float4 v = stage[q * a.span_cap + pb];
                    h[q][0] = fmaf(w, v.x, h[q][0]);
                    h[q][1] = fmaf(w, v.y, h[q][1]);
                    h[q][2] = fmaf(w, v.z, h[q][2]);
                    h[q][3] = fmaf(w, v.w, h[q][3]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < RS_RQ; ++q) {
            if (active && q < nq) {
#pragma unroll
                for (int i = 0; i < RS_RB; ++i) {
                    const int k = rb + q - rs_i[i];
                    if (i < nrow && k >= 0 && k < TR) {
                        const float w = a.rw[(size_t)(i0 + i) * TR + k];
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(w, h[q][c], acc[i][c]);
                    }
                }
            }
        }
    }
    if (active) {
        const int j = flip ? a.W - 1 - (jt0 + t) : jt0 + t;
#pragma unroll
        for (int i = 0; i < RS_RB; ++i)
            if (i < nrow)
                store_pixel<T>(reinterpret_cast<T*>(a.out) + (int64_t)n * a.out_stride + ((int64_t)(i0 + i) * a.W + j) * SGG_CPAD, acc[i], a.C);
    }
}

}  // namespace

extern "C" int sgg_resample_u8(const uint8_t* src, int M, int H0, int W0, int Cs, const int32_t* index, const int32_t* flip,
                               const float* row_w, const int32_t* row_start, int row_taps,
                               const float* col_w, const int32_t* col_start, int col_taps, int col_step,
                               void* out, int N, int H, int W, int C, int dtype, void* stream) {
    if (!src || !index || !flip || !row_w || !row_start || !col_w || !col_start || !out) return SGG_EINVAL;
    if (M <= 0 || H0 <= 0 || W0 <= 0 || N <= 0 || H <= 0 || W <= 0 || (Cs != 3 && Cs != 4) || C <= 0 || C > Cs || C > SGG_CPAD) return SGG_EINVAL;
    if (row_taps <= 0 || row_taps > H0 || col_taps <= 0 || col_taps > W0 || col_step < 0) return SGG_EINVAL;
    if (dtype != SGG_F32 && dtype != SGG_BF16) return SGG_EINVAL;
    if (((uintptr_t)out & 15) != 0 || (Cs == 4 && ((uintptr_t)src & 3) != 0)) return SGG_EINVAL;
    if (N > 65535 || (H + RS_RB - 1) / RS_RB > 65535) return SGG_EUNSUPPORTED;
    ResampleArgs a;
    a.src = src; a.src_bytes = (int64_t)M * H0 * W0 * Cs; a.M = M; a.H0 = H0; a.W0 = W0;
    a.index = index; a.flip = flip; a.rw = row_w; a.rs = row_start; a.TR = row_taps; a.cw = col_w; a.cs = col_start; a.TC = col_taps;
    a.out = out; a.N = N; a.H = H; a.W = W; a.C = C;
    const int64_t span = (int64_t)(std::min(W, RS_CB) - 1) * col_step + col_taps;      // widest column window of a tile
    a.span_cap = (int)std::min<int64_t>(span, W0);
    a.seg = (int)((((int64_t)a.span_cap * Cs + 15 + 15) / 16) * 16);
    a.wstride = (std::min(W, RS_CB) + 63) / 64 * 64;
    const int64_t wbytes = (int64_t)col_taps * a.wstride * sizeof(float);
    if (wbytes + a.seg > RS_LDS) return SGG_EUNSUPPORTED;
    a.rq = (int)std::min<int64_t>(RS_RQ, (RS_LDS - wbytes) / a.seg);
    const size_t lds = (size_t)wbytes + (size_t)a.rq * a.seg;
    dim3 grid((W + RS_CB - 1) / RS_CB, (H + RS_RB - 1) / RS_RB, N);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SGG_BF16) {
        if (Cs == 3) hipLaunchKernelGGL((resample_u8_kernel<3, bf16>), grid, dim3(RS_CB), lds, s, a);
        else hipLaunchKernelGGL((resample_u8_kernel<4, bf16>), grid, dim3(RS_CB), lds, s, a);
    } else {
        if (Cs == 3) hipLaunchKernelGGL((resample_u8_kernel<3, float>), grid, dim3(RS_CB), lds, s, a);
        else hipLaunchKernelGGL((resample_u8_kernel<4, float>), grid, dim3(RS_CB), lds, s, a);
    }
    return sgg_check_launch();
}

extern "C" int sgg_resample_f32(const float* src, int N, int H0, int W0, const int32_t* flip,
                                const float* row_w, const int32_t* row_start, int row_taps,
                                const float* col_w, const int32_t* col_start, int col_taps, int col_step,
                                void* out, int64_t out_stride, int H, int W, int C, int dtype, void* stream) {
    if (!src || !flip || !row_w || !row_start || !col_w || !col_start || !out) return SGG_EINVAL;
    if (N <= 0 || H0 <= 0 || W0 <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4) return SGG_EINVAL;
    if (row_taps <= 0 || row_taps > H0 || col_taps <= 0 || col_taps > W0 || col_step < 0) return SGG_EINVAL;
    if (dtype != SGG_F32 && dtype != SGG_BF16) return SGG_EINVAL;
    if (out_stride < (int64_t)H * W * SGG_CPAD || (out_stride % SGG_CPAD) != 0) return SGG_EINVAL;
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)src & 15) != 0) return SGG_EINVAL;
    if (N > 65535 || (H + RS_RB - 1) / RS_RB > 65535) return SGG_EUNSUPPORTED;
    ResampleF32Args a;
    a.src = reinterpret_cast<const float4*>(src); a.H0 = H0; a.W0 = W0; a.flip = flip;
    a.rw = row_w; a.rs = row_start; a.TR = row_taps; a.cw = col_w; a.cs = col_start; a.TC = col_taps;
    a.out = out; a.out_stride = out_stride; a.N = N; a.H = H; a.W = W; a.C = C;
    const int64_t span = (int64_t)(std::min(W, RS_CB) - 1) * col_step + col_taps;
    a.span_cap = (int)std::min<int64_t>(span, W0);
    const int64_t seg = (int64_t)a.span_cap * (int64_t)sizeof(float4);
    a.wstride = (std::min(W, RS_CB) + 63) / 64 * 64;
    const int64_t wbytes = (int64_t)col_taps * a.wstride * sizeof(float);
    if (wbytes + seg > RS_LDS) return SGG_EUNSUPPORTED;
    a.rq = (int)std::min<int64_t>(RS_RQ, (RS_LDS - wbytes) / seg);
    const size_t lds = (size_t)wbytes + (size_t)a.rq * seg;
    dim3 grid((W + RS_CB - 1) / RS_CB, (H + RS_RB - 1) / RS_RB, N);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SGG_BF16) hipLaunchKernelGGL((resample_f32_kernel<bf16>), grid, dim3(RS_CB), lds, s, a);
    else hipLaunchKernelGGL((resample_f32_kernel<float>), grid, dim3(RS_CB), lds, s, a);
    return sgg_check_launch();
}
