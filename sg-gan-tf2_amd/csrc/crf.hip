// crf.hip -- fully connected CRF label refinement: metric.dense_crf (metric.py:49-69), i.e. pydensecrf's DenseCRF2D with one
// Gaussian and one bilateral pairwise term, Potts compatibility, NORMALIZE_SYMMETRIC and `max_iter` mean-field steps -- with the
// message passing done EXACTLY (all N^2 pixel pairs) instead of through pydensecrf's permutohedral lattice.
//
//   U          = -log(clip(p, 1e-5, 1))                                            (C, N), N = H*W row major
//   k_g(i,j)   = exp(-|p_i - p_j|^2 / (2 sxy_g^2)),   k_b(i,j) = exp(-|p_i - p_j|^2 / (2 sxy_b^2) - |rgb_i - rgb_j|^2 / (2 srgb^2))
//   n_x[i]     = 1 / sqrt(sum_j k_x(i,j) + 1e-20)                                   (j = i included)
//   Q_0        = softmax_c(-U);   Q_{t+1} = softmax_c(-U + w_g n_g (K_g (n_g Q_t)) + w_b n_b (K_b (n_b Q_t)))
//
// K is never stored.  The pair kernel gives every thread CRF_PX target pixels i and walks the source pixels j in tiles of
// CRF_TJ whose feature rows and scaled rows (n_g Q | n_b Q)[j] are staged in LDS; every lane reads the SAME j at a time, so the
// LDS reads are broadcasts.  Per pair: the (x, y) distance once, two v_exp_f32, and per channel two FMAs into ONE accumulator
// -- the weights w_g n_g[i], w_b n_b[i] are constants of the target pixel and go onto k first.  The same kernel with NORM set
// accumulates the two "ones" columns sum_j k_g, sum_j k_b for the normalisers instead.  Plain f32 FMAs: with two or more waves
// per SIMD the f32 VALU issues at the rate of the f32-input MFMA (MI355X: 64 FLOP/clk/SIMD either way), k keeps its f32
// precision, and C = 34 pads to 40 here instead of 48 or 64 MFMA columns.
//
// Parallelism over j: grid.y splits the source range (so a 128 x 128 image fills the chip), every split writes its partial
// sums to the workspace and the softmax kernel adds them in split order.  No atomics, fixed order: two runs give the same bits.
#include "common.h"
#include <algorithm>
#include <math.h>

namespace {

constexpr int CRF_THREADS = 256;
constexpr int CRF_PX = 2;                          // target pixels per thread: halves the LDS bytes per FMA
constexpr int CRF_TI = CRF_THREADS * CRF_PX;       // target pixels per block
constexpr int CRF_TJ = 64;                         // source pixels per LDS tile
constexpr int CRF_MAX_SPLIT = 16;                  // splits of the source range (grid.y)
constexpr int CRF_MAX_CP = 40;                     // padded channels a thread can accumulate for two pixels without spilling
constexpr int CRF_FEAT = 8;                        // floats per feature row: x, y, r/srgb, g/srgb, b/srgb, 0, 0, 0
constexpr int CRF_MAX_N = 1 << 22;                 // coordinates are exact in f32, every index fits 32 bits per split

struct CrfPlan {
    int N, CP, JS, jspan;
    size_t off_feat, off_unary, off_qs, off_nrm, off_part, bytes;
};

// SGG_OK and the plan, or the reason there is none
int crf_plan(int H, int W, int C, CrfPlan& p) {
    if (H <= 0 || W <= 0 || C <= 0) return SGG_EINVAL;
    if ((int64_t)H * W > CRF_MAX_N) return SGG_EUNSUPPORTED;
    p.N = H * W;
    p.CP = (C + SGG_CPAD - 1) / SGG_CPAD * SGG_CPAD;
    if (p.CP > CRF_MAX_CP) return SGG_EUNSUPPORTED;
    const int ntiles = (p.N + CRF_TI - 1) / CRF_TI, jtiles = (p.N + CRF_TJ - 1) / CRF_TJ;
    int js = std::min(std::min(CRF_MAX_SPLIT, jtiles), std::max(1, (2 * 256 + ntiles - 1) / ntiles));     // >= 512 blocks where N allows
    p.jspan = (jtiles + js - 1) / js * CRF_TJ;
    p.JS = (p.N + p.jspan - 1) / p.jspan;                                                                 // no empty split
    size_t o = 0;
    p.off_feat = o;  o = align_up(o + (size_t)p.N * CRF_FEAT * sizeof(float), 256);
    p.off_unary = o; o = align_up(o + (size_t)p.N * p.CP * sizeof(float), 256);
    p.off_qs = o;    o = align_up(o + (size_t)p.N * 2 * p.CP * sizeof(float), 256);
    p.off_nrm = o;   o = align_up(o + (size_t)p.N * 2 * sizeof(float), 256);
    p.off_part = o;  o = align_up(o + (size_t)p.JS * p.N * p.CP * sizeof(float), 256);
    p.bytes = o;
    return SGG_OK;
}

// features and unary of every pixel.  The log is taken in double and rounded once: U is then the correctly rounded f32 of
// -log(clip(p)), which a caller can reproduce on the host bit for bit (the ready-unary path).
__global__ __launch_bounds__(CRF_THREADS) void crf_prep_kernel(const uint8_t* __restrict__ img, const float* __restrict__ probs,
                                                               const float* __restrict__ unary, float* __restrict__ feat,
                                                               float* __restrict__ U, int N, int W, int C, int CP, float inv_rgb) {
    const int i = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (i >= N) return;
    const int y = i / W, x = i - y * W;
    const uint8_t* px = img + (size_t)i * 3;
    float4* f = reinterpret_cast<float4*>(feat + (size_t)i * CRF_FEAT);
    f[0] = make_float4((float)x, (float)y, (float)px[0] * inv_rgb, (float)px[1] * inv_rgb);
    f[1] = make_float4((float)px[2] * inv_rgb, 0.f, 0.f, 0.f);
    for (int c = 0; c < CP; ++c) {
        float u = 0.f;
        if (c < C) {
            if (probs) u = (float)(-log(fmin(fmax((double)probs[(size_t)c * N + i], 1e-5), 1.0)));
            else u = unary[(size_t)c * N + i];
        }
        U[(size_t)i * CP + c] = u;
    }
}

struct CrfPairArgs {
    const float* feat; const float* qs; const float* nrm; float* part;
    int N, jspan;
    float cg, cb, ch;           // exp2 scales: -log2(e) / (2 sxy_g^2), -log2(e) / (2 sxy_b^2), -log2(e) / 2 (rgb is pre-scaled)
    float wpos, wbi;
};

template <int CP, bool NORM>
__global__ __launch_bounds__(CRF_THREADS) void crf_pair_kernel(const CrfPairArgs a) {
    constexpr int ACC = NORM ? 2 : CP;
    constexpr int ROW4 = 2 * CP / 4;                               // float4s per staged (n_g Q | n_b Q) row
    __shared__ float4 sfeat[CRF_TJ * 2];
    __shared__ float4 sq[NORM ? 1 : CRF_TJ * ROW4];
    const int t = threadIdx.x, N = a.N;
    const int jbeg = blockIdx.y * a.jspan, jend = min(N, jbeg + a.jspan);

    float fx[CRF_PX], fy[CRF_PX], fr[CRF_PX], fg[CRF_PX], fb[CRF_PX], wg[CRF_PX], wb[CRF_PX];
    float acc[CRF_PX][ACC];
#pragma unroll
    for (int p = 0; p < CRF_PX; ++p) {
        const int i = min(blockIdx.x * CRF_TI + p * CRF_THREADS + t, N - 1);       // the ragged tail computes pixel N-1 again and stores nothing
        const float4 f0 = reinterpret_cast<const float4*>(a.feat)[(size_t)i * 2], f1 = reinterpret_cast<const float4*>(a.feat)[(size_t)i * 2 + 1];
        fx[p] = f0.x; fy[p] = f0.y; fr[p] = f0.z; fg[p] = f0.w; fb[p] = f1.x;
        wg[p] = NORM ? 1.f : a.wpos * a.nrm[(size_t)i * 2];
        wb[p] = NORM ? 1.f : a.wbi * a.nrm[(size_t)i * 2 + 1];
#pragma unroll
        for (int c = 0; c < ACC; ++c) acc[p][c] = 0.f;
    }

    const float4* feat4 = reinterpret_cast<const float4*>(a.feat);
    const float4* qs4 = reinterpret_cast<const float4*>(a.qs);
    for (int j0 = jbeg; j0 < jend; j0 += CRF_TJ) {
        const int jn = min(CRF_TJ, jend - j0);
        __syncthreads();                                            // the previous tile has been consumed
        for (int e = t; e < jn * 2; e += CRF_THREADS) sfeat[e] = feat4[(size_t)j0 * 2 + e];
        if (!NORM)
            for (int e = t; e < jn * ROW4; e += CRF_THREADS) sq[e] = qs4[(size_t)j0 * ROW4 + e];
        __syncthreads();
        for (int jj = 0; jj < jn; ++jj) {
            const float4 s0 = sfeat[jj * 2], s1 = sfeat[jj * 2 + 1];
            float kg[CRF_PX], kb[CRF_PX];
#pragma unroll
            for (int p = 0; p < CRF_PX; ++p) {
                const float dx = fx[p] - s0.x, dy = fy[p] - s0.y;
                const float d2 = fmaf(dy, dy, dx * dx);                           // shared by the two kernels
                const float dr = fr[p] - s0.z, dg = fg[p] - s0.w, db = fb[p] - s1.x;
                const float c2 = fmaf(db, db, fmaf(dg, dg, dr * dr));
                kg[p] = __builtin_amdgcn_exp2f(d2 * a.cg);
                kb[p] = __builtin_amdgcn_exp2f(fmaf(d2, a.cb, c2 * a.ch));
                if (NORM) {
                    acc[p][0] += kg[p];
                    acc[p][1] += kb[p];
                } else {
                    kg[p] *= wg[p];
                    kb[p] *= wb[p];
                }
            }
            if constexpr (!NORM) {
#pragma unroll
                for (int c4 = 0; c4 < CP / 4; ++c4) {
                    const float4 qg = sq[jj * ROW4 + c4], qb = sq[jj * ROW4 + CP / 4 + c4];
#pragma unroll
                    for (int p = 0; p < CRF_PX; ++p) {
                        float* A = &acc[p][c4 * 4];
                        A[0] = fmaf(kb[p], qb.x, fmaf(kg[p], qg.x, A[0]));
                        A[1] = fmaf(kb[p], qb.y, fmaf(kg[p], qg.y, A[1]));
                        A[2] = fmaf(kb[p], qb.z, fmaf(kg[p], qg.z, A[2]));
                        A[3] = fmaf(kb[p], qb.w, fmaf(kg[p], qg.w, A[3]));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < CRF_PX; ++p) {
        const int i = blockIdx.x * CRF_TI + p * CRF_THREADS + t;
        if (i >= N) continue;
        float* o = a.part + ((size_t)blockIdx.y * N + i) * ACC;
        if (NORM) {
            *reinterpret_cast<float2*>(o) = make_float2(acc[p][0], acc[p][1]);
        } else {
#pragma unroll
            for (int c4 = 0; c4 < ACC / 4; ++c4)
                reinterpret_cast<float4*>(o)[c4] = make_float4(acc[p][c4 * 4], acc[p][c4 * 4 + 1], acc[p][c4 * 4 + 2], acc[p][c4 * 4 + 3]);
        }
    }
}

// Q = softmax_c(-U + message) with the maximum subtracted; writes the scaled rows the next pair pass stages and, after the
// last step, Q itself as (C, N).  first: part holds the normaliser sums [JS][N][2] instead of a message (Q_0 = softmax(-U)).
template <int CP>
__global__ __launch_bounds__(CRF_THREADS) void crf_softmax_kernel(const float* __restrict__ U, const float* __restrict__ part, int JS,
                                                                  float* __restrict__ nrm, float* __restrict__ qs, float* __restrict__ out,
                                                                  int N, int C, int first, int last) {
    const int i = blockIdx.x * CRF_THREADS + threadIdx.x;
    if (i >= N) return;
    float l[CP];
    float ng, nb;
    const float4* u4 = reinterpret_cast<const float4*>(U + (size_t)i * CP);
#pragma unroll
    for (int c4 = 0; c4 < CP / 4; ++c4) {
        const float4 u = u4[c4];
        l[c4 * 4] = u.x; l[c4 * 4 + 1] = u.y; l[c4 * 4 + 2] = u.z; l[c4 * 4 + 3] = u.w;
    }
    if (first) {
        float sg = 0.f, sb = 0.f;
        for (int s = 0; s < JS; ++s) {
            const float2 v = *reinterpret_cast<const float2*>(part + ((size_t)s * N + i) * 2);
            sg += v.x; sb += v.y;
        }
        ng = 1.0f / sqrtf(sg + 1e-20f);
        nb = 1.0f / sqrtf(sb + 1e-20f);
        *reinterpret_cast<float2*>(nrm + (size_t)i * 2) = make_float2(ng, nb);
#pragma unroll
        for (int c = 0; c < CP; ++c) l[c] = -l[c];
    } else {
        const float2 v = *reinterpret_cast<const float2*>(nrm + (size_t)i * 2);
        ng = v.x; nb = v.y;
        float m[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) m[c] = 0.f;
        for (int s = 0; s < JS; ++s) {
            const float4* p4 = reinterpret_cast<const float4*>(part + ((size_t)s * N + i) * CP);
#pragma unroll
            for (int c4 = 0; c4 < CP / 4; ++c4) {
                const float4 v4 = p4[c4];
                m[c4 * 4] += v4.x; m[c4 * 4 + 1] += v4.y; m[c4 * 4 + 2] += v4.z; m[c4 * 4 + 3] += v4.w;
            }
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) l[c] = m[c] - l[c];
    }
    float mx = l[0];
#pragma unroll
    for (int c = 1; c < CP; ++c)
        if (c < C) mx = fmaxf(mx, l[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        l[c] = c < C ? expf(l[c] - mx) : 0.f;
        sum += l[c];
    }
    float4* q4 = reinterpret_cast<float4*>(qs + (size_t)i * 2 * CP);
#pragma unroll
    for (int c = 0; c < CP; ++c) l[c] = l[c] / sum;
#pragma unroll
    for (int c4 = 0; c4 < CP / 4; ++c4) {
        q4[c4] = make_float4(ng * l[c4 * 4], ng * l[c4 * 4 + 1], ng * l[c4 * 4 + 2], ng * l[c4 * 4 + 3]);
        q4[CP / 4 + c4] = make_float4(nb * l[c4 * 4], nb * l[c4 * 4 + 1], nb * l[c4 * 4 + 2], nb * l[c4 * 4 + 3]);
    }
    if (last) {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) out[(size_t)c * N + i] = l[c];
    }
}

template <int CP>
int crf_run(const CrfPlan& p, const CrfPairArgs& base, const float* U, float* nrm, float* qs, float* out, int C, int max_iter,
            hipStream_t s) {
    const int N = p.N;
    const dim3 pgrid((N + CRF_TI - 1) / CRF_TI, p.JS), blk(CRF_THREADS), sgrid((N + CRF_THREADS - 1) / CRF_THREADS);
    hipLaunchKernelGGL((crf_pair_kernel<8, true>), pgrid, blk, 0, s, base);
    hipLaunchKernelGGL((crf_softmax_kernel<CP>), sgrid, blk, 0, s, U, base.part, p.JS, nrm, qs, out, N, C, 1, max_iter == 0 ? 1 : 0);
    for (int it = 1; it <= max_iter; ++it) {
        hipLaunchKernelGGL((crf_pair_kernel<CP, false>), pgrid, blk, 0, s, base);
        hipLaunchKernelGGL((crf_softmax_kernel<CP>), sgrid, blk, 0, s, U, base.part, p.JS, nrm, qs, out, N, C, 0, it == max_iter ? 1 : 0);
    }
    return sgg_check_launch();
}

}  // namespace

extern "C" size_t sgg_dense_crf_workspace_bytes(int H, int W, int C) {
    CrfPlan p;
    return crf_plan(H, W, C, p) == SGG_OK ? p.bytes : 0;
}

extern "C" int sgg_dense_crf(const uint8_t* img, const float* probs, const float* unary, int H, int W, int C, int max_iter,
                             float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, float* q_out,
                             void* ws, size_t ws_bytes, void* stream) {
    CrfPlan p;
    const int rc = crf_plan(H, W, C, p);
    if (rc != SGG_OK) return rc;
    if (!img || !q_out || (probs == nullptr) == (unary == nullptr)) return SGG_EINVAL;          // exactly one of probs / unary
    if (max_iter < 0 || !(pos_xy_std > 0.f) || !(bi_xy_std > 0.f) || !(bi_rgb_std > 0.f)) return SGG_EINVAL;
    if (!ws || ws_bytes < p.bytes) return SGG_EWORKSPACE;
    if (((uintptr_t)ws & 15) != 0) return SGG_EINVAL;
    char* w = static_cast<char*>(ws);
    float* feat = reinterpret_cast<float*>(w + p.off_feat);
    float* U = reinterpret_cast<float*>(w + p.off_unary);
    float* qs = reinterpret_cast<float*>(w + p.off_qs);
    float* nrm = reinterpret_cast<float*>(w + p.off_nrm);
    float* part = reinterpret_cast<float*>(w + p.off_part);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(crf_prep_kernel, dim3((p.N + CRF_THREADS - 1) / CRF_THREADS), dim3(CRF_THREADS), 0, s, img, probs, unary, feat, U,
                       p.N, W, C, p.CP, 1.0f / bi_rgb_std);
    const double l2e = 1.4426950408889634;
    CrfPairArgs a;
    a.feat = feat; a.qs = qs; a.nrm = nrm; a.part = part; a.N = p.N; a.jspan = p.jspan;
    a.cg = (float)(-0.5 * l2e / ((double)pos_xy_std * pos_xy_std));
    a.cb = (float)(-0.5 * l2e / ((double)bi_xy_std * bi_xy_std));
    a.ch = (float)(-0.5 * l2e);
    a.wpos = pos_w; a.wbi = bi_w;
    switch (p.CP) {
        case 8: return crf_run<8>(p, a, U, nrm, qs, q_out, C, max_iter, s);
        case 16: return crf_run<16>(p, a, U, nrm, qs, q_out, C, max_iter, s);
        case 24: return crf_run<24>(p, a, U, nrm, qs, q_out, C, max_iter, s);
        case 32: return crf_run<32>(p, a, U, nrm, qs, q_out, C, max_iter, s);
        case 40: return crf_run<40>(p, a, U, nrm, qs, q_out, C, max_iter, s);
    }
    return SGG_EUNSUPPORTED;
}
