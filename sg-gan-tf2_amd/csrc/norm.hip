// norm.hip -- instance normalisation (tfa.layers.InstanceNormalization, module.py:212..308; ops.py:13-22 by name)
// fused with the following activation (module.py:213,234,...; LeakyReLU :289-309) and the residual add (:217).
//
// HBM-bound.  NHWC: a thread owns one 16-byte channel vector and walks pixels, so every access is a coalesced
// 16-byte load and the per-(n,c) reduction never crosses channels.  Two passes per direction:
//   fwd : partial (sum, sumsq) per pixel-chunk -> finalize (mean, rstd; f64 combine, fixed order) -> apply
//   bwd : partial (sum g, sum g*xhat)          -> finalize (+ dgamma, dbeta over n)               -> apply
// Algorithmic bytes: fwd 2 reads + 1 write of the tensor, bwd 4 reads + 1 write.
#include "common.h"
#include <type_traits>

// Per-thread accumulators of the statistics passes.  On the f32 parity path they are f64: the backward sums (sum g,
// sum g*xhat) add a near-zero-mean field (the gradient that comes back through a SAME conv from another instance
// norm), so the sum cancels to ~1e-3 of its terms and an f32 running sum over 64+ pixels is off by 1e-4 of the result --
// visible against the float64 oracle (tools/diag_d_f32.py).  On the bf16 path the operands carry 8 bits: f32 is plenty.
// pixels per loop trip in the streaming passes (= 16-byte loads in flight per thread and tensor): 4 forward; 2 backward, where
// two tensors are read and 4 would cost occupancy (166 VGPRs: 3 waves/SIMD, measured 5-15 % slower than 2)
#define IN_U (BWD ? 2 : 4)
template <typename T> using InAcc = typename std::conditional<std::is_same<T, float>::value, double, float>::type;

// Two networks of the same shape run in lockstep on a batch that stacks their activations (images 0..nsplit-1 belong to
// the first, the rest to the second -- the cycle step's G_A->B / G_B->A and D_A / D_B pairs): the norm is per image, so one
// launch serves both and only the affine parameters (and their gradients) are picked by image index.  nsplit >= N: one network.
struct InSplit { const float* gamma2; const float* beta2; float* dgamma2; float* dbeta2; int nsplit; };

// The incoming gradient dy normally has the tensor's storage type T.  Mixed mode (bf16 tensors, f32 gradient chain): dy is
// f32 -- the VEC channels of a 16-byte chunk of x are then two 16-byte chunks of dy.  `elem` = element index of the chunk.
#ifndef IN_NT
#define IN_NT 15               // streaming (nt) loads in the apply passes of tensors this pass reads for the last time before they leave the
                               // caches anyway: 1 forward x, 2 backward x, 4 backward dy, 8 the forward residual (A/B: profiles/r04_nt_loads.txt)
#endif
template <typename T, typename TG, bool NT = false>
__device__ inline void in_load_grad(const char* dy, size_t elem, float* gv) {
    if constexpr (std::is_same<T, TG>::value) {
        ET<T>::unpack(NT ? ld16_nt(dy + elem * sizeof(T)) : ld16(dy + elem * sizeof(T)), gv);
    } else {
        static_assert(std::is_same<TG, float>::value && ET<T>::VEC == 8, "mixed mode: f32 gradient of a bf16 tensor");
        ET<float>::unpack(ld16(dy + elem * 4), gv);
        ET<float>::unpack(ld16(dy + elem * 4 + 16), gv + 4);
    }
}

// pixels per partial-sum chunk: >= 64, and large enough that an image has at most ~128 chunks (the finalize kernels
// walk the chunks of one channel serially: 2048 chunks cost 68 us on a 256x512x64 tensor, 128 chunks 5 us)
static inline int in_rows_per_chunk(int64_t HW) {
    int64_t r = (HW + 127) / 128;
    r = (r + 63) / 64 * 64;
    return (int)(r < 64 ? 64 : (r > 4096 ? 4096 : r));
}
// ws layout: partial[N][chunks][C][2] f32, then sums[N][C][2] and tot[N][C][2] f32 (bwd only)
static inline int in_chunks(int64_t HW) { int r = in_rows_per_chunk(HW); return (int)((HW + r - 1) / r); }

template <typename T, bool BWD, typename TG = T>
__global__ __launch_bounds__(256) void in_partial_kernel(const char* x, const char* dy, const float* gamma, const float* beta,
                                                         const float* stats, float* partial, int64_t HW, int C, int chunks,
                                                         int rpc, int act, float leak, InSplit sp) {
    constexpr int VEC = ET<T>::VEC;
    const int CV = C / VEC;                       // channel vectors per pixel
    const int n = blockIdx.y, chunk = blockIdx.x;
    if (n >= sp.nsplit) { gamma = sp.gamma2; beta = sp.beta2; }
    const int64_t p0 = (int64_t)chunk * rpc;
    const int64_t p1 = p0 + rpc < HW ? p0 + rpc : HW;
    using AccT = InAcc<T>;
    __shared__ AccT red[256][2 * VEC + 1];
    // threads cover (pixel row, channel vector) pairs: cv = item % CV walks fastest
    for (int cvb = 0; cvb < CV; cvb += 256) {
        const int lanes = CV - cvb < 256 ? CV - cvb : 256;       // channel vectors handled in this sweep
        const int rows = 256 / lanes;                            // pixel rows in flight
        const int cv = cvb + (int)(threadIdx.x % lanes), prow = threadIdx.x / lanes;
        AccT s1[VEC], s2[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) s1[e] = s2[e] = (AccT)0;
        float mu[VEC], rs[VEC], gm[VEC], bt[VEC];
        if (BWD && prow < rows) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                int c = cv * VEC + e;
                mu[e] = stats[((size_t)n * C + c) * 2]; rs[e] = stats[((size_t)n * C + c) * 2 + 1];
                gm[e] = gamma[c]; bt[e] = beta[c];
            }
        }
        // IN_U pixels per trip: all their loads are issued before the first use (one 16-byte load in flight per thread left the
        // pass latency bound), and the activation code is resolved once -- the element loop is then branch-free selects.
        // The per-thread accumulation order (pixel order) is unchanged.
        if (prow < rows)
            act_dispatch(BWD ? act : SGG_ACT_NONE, [&](auto act_c) {
                constexpr int ACT = decltype(act_c)::value;
                auto accumulate = [&](const u32x4& xr, const float* gv) {
                    float xv[VEC];
                    ET<T>::unpack(xr, xv);
                    if (!BWD) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) { s1[e] += (AccT)xv[e]; s2[e] += (AccT)xv[e] * (AccT)xv[e]; }
                    } else {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            float xh = (xv[e] - mu[e]) * rs[e];
                            float g = gv[e] * act_grad_c<ACT>(gm[e] * xh + bt[e], leak);
                            s1[e] += (AccT)g; s2[e] += (AccT)g * (AccT)xh;
                        }
                    }
                };
                const size_t base = ((size_t)n * HW * C + (size_t)cv * VEC) * sizeof(T), pstep = (size_t)C * sizeof(T);
                int64_t p = p0 + prow;
                for (; p + (IN_U - 1) * rows < p1; p += IN_U * rows) {
                    u32x4 xr[IN_U];
                    float gv[IN_U][BWD ? VEC : 1];
#pragma unroll
                    for (int u = 0; u < IN_U; ++u) xr[u] = ld16(x + base + (size_t)(p + u * rows) * pstep);
                    if (BWD) {
#pragma unroll
                        for (int u = 0; u < IN_U; ++u) in_load_grad<T, TG, (IN_NT & 4) != 0>(dy, (base + (size_t)(p + u * rows) * pstep) / sizeof(T), gv[u]);
                    }
#pragma unroll
                    for (int u = 0; u < IN_U; ++u) accumulate(xr[u], gv[u]);
                }
                for (; p < p1; p += rows) {
                    const size_t off = base + (size_t)p * pstep;
                    float gv[BWD ? VEC : 1];
                    const u32x4 xr = ld16(x + off);
                    if (BWD) in_load_grad<T, TG>(dy, off / sizeof(T), gv);
                    accumulate(xr, gv);
                }
            });
#pragma unroll
        for (int e = 0; e < VEC; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][VEC + e] = s2[e]; }
        __syncthreads();
        // fixed-order combine over the pixel rows of each channel vector
        for (int item = threadIdx.x; item < lanes * VEC; item += 256) {
            int l = item / VEC, e = item % VEC;
            AccT a = (AccT)0, b = (AccT)0;
            for (int r = 0; r < rows; ++r) { a += red[r * lanes + l][e]; b += red[r * lanes + l][VEC + e]; }
            int c = (cvb + l) * VEC + e;
            size_t o = (((size_t)n * chunks + chunk) * C + c) * 2;
            partial[o] = (float)a; partial[o + 1] = (float)b;
        }
        __syncthreads();
    }
}

// Finalize: one 1024-thread block per (32 channels, image); 32 chunk-lanes per channel, each with up to four independent
// loads in flight, combined in fixed order (deterministic).  (8 lanes walking 16 chunks one dependent L2 load after the
// other took 5-6 us per launch -- 250 launches per cycle step, 3.7 % of it.)
#define FIN_CH 32
#define FIN_LANES 32
__device__ inline void fin_reduce(const float* partial, int n, int c, int chunks, int C, int lane, double& s1, double& s2) {
    s1 = 0.0; s2 = 0.0;
    for (int k0 = lane; k0 < chunks; k0 += FIN_LANES * 4) {
        float2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * FIN_LANES;
            v[u] = k < chunks ? *reinterpret_cast<const float2*>(partial + (((size_t)n * chunks + k) * C + c) * 2) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s1 += (double)v[u].x; s2 += (double)v[u].y; }
    }
}

__global__ __launch_bounds__(1024) void in_finalize_fwd_kernel(const float* partial, float* stats, int64_t HW, int C, int chunks, float eps) {
    __shared__ double red[FIN_LANES][FIN_CH][2];
    const int tx = threadIdx.x % FIN_CH, ty = threadIdx.x / FIN_CH;
    const int c = blockIdx.x * FIN_CH + tx, n = blockIdx.y;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) fin_reduce(partial, n, c, chunks, C, ty, s1, s2);
    red[ty][tx][0] = s1; red[ty][tx][1] = s2;
    __syncthreads();
    if (ty == 0 && c < C) {
        for (int l = 1; l < FIN_LANES; ++l) { s1 += red[l][tx][0]; s2 += red[l][tx][1]; }
        double mean = s1 / (double)HW, var = s2 / (double)HW - mean * mean;
        if (var < 0.0) var = 0.0;
        size_t i = (size_t)n * C + c;
        stats[i * 2] = (float)mean;
        stats[i * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// sums[n][c] = (sum g, sum g*xhat) / HW ; tot[n][c] = the raw sums (for dgamma/dbeta)
__global__ __launch_bounds__(1024) void in_finalize_bwd_kernel(const float* partial, float* sums, float* tot, int64_t HW, int C, int chunks) {
    __shared__ double red[FIN_LANES][FIN_CH][2];
    const int tx = threadIdx.x % FIN_CH, ty = threadIdx.x / FIN_CH;
    const int c = blockIdx.x * FIN_CH + tx, n = blockIdx.y;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) fin_reduce(partial, n, c, chunks, C, ty, s1, s2);
    red[ty][tx][0] = s1; red[ty][tx][1] = s2;
    __syncthreads();
    if (ty == 0 && c < C) {
        for (int l = 1; l < FIN_LANES; ++l) { s1 += red[l][tx][0]; s2 += red[l][tx][1]; }
        size_t i = ((size_t)n * C + c) * 2;
        sums[i] = (float)(s1 / (double)HW); sums[i + 1] = (float)(s2 / (double)HW);
        tot[i] = (float)s1; tot[i + 1] = (float)s2;
    }
}

// dgamma[c] (+)= sum_n sum g*xhat ; dbeta[c] (+)= sum_n sum g   (fixed order over n -> deterministic).  Run by the
// first block of the backward apply kernel (a separate launch cost ~5 us per instance norm for a few hundred FLOPs).
struct InParamGrad { const float* tot; float* dgamma; float* dbeta; int N, Cr, accumulate; };
__device__ inline void in_param_grad(const InParamGrad& g, int C, const InSplit& sp) {
    const int n1 = g.N < sp.nsplit ? g.N : sp.nsplit;
    for (int c = threadIdx.x; c < g.Cr; c += blockDim.x) {
        double tg = 0.0, tb = 0.0;
        for (int n = 0; n < n1; ++n) { tb += (double)g.tot[((size_t)n * C + c) * 2]; tg += (double)g.tot[((size_t)n * C + c) * 2 + 1]; }
        g.dgamma[c] = g.accumulate ? g.dgamma[c] + (float)tg : (float)tg;
        g.dbeta[c] = g.accumulate ? g.dbeta[c] + (float)tb : (float)tb;
        if (n1 < g.N) {                                  // the second network's images
            tg = 0.0; tb = 0.0;
            for (int n = n1; n < g.N; ++n) { tb += (double)g.tot[((size_t)n * C + c) * 2]; tg += (double)g.tot[((size_t)n * C + c) * 2 + 1]; }
            sp.dgamma2[c] = g.accumulate ? sp.dgamma2[c] + (float)tg : (float)tg;
            sp.dbeta2[c] = g.accumulate ? sp.dbeta2[c] + (float)tb : (float)tb;
        }
    }
}

template <typename T, bool BWD, typename TG = T>
__global__ __launch_bounds__(256) void in_apply_kernel(const char* x, const char* dy, const char* residual, const float* gamma,
                                                       const float* beta, const float* stats, const float* sums, char* out,
                                                       int64_t HW, int C, int rows_per_block, int act, float leak, InParamGrad pg, InSplit sp) {
    constexpr int VEC = ET<T>::VEC;
    const int CV = C / VEC;
    const int n = blockIdx.y;
    if (BWD && blockIdx.x == 0 && blockIdx.y == 0) in_param_grad(pg, C, sp);
    if (n >= sp.nsplit) { gamma = sp.gamma2; beta = sp.beta2; }
    const int64_t p0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t p1 = p0 + rows_per_block < HW ? p0 + rows_per_block : HW;
    for (int cvb = 0; cvb < CV; cvb += 256) {
        const int lanes = CV - cvb < 256 ? CV - cvb : 256;
        const int rows = 256 / lanes;
        const int cv = cvb + (int)(threadIdx.x % lanes), prow = threadIdx.x / lanes;
        if (prow >= rows) continue;
        float A[VEC], B[VEC], mu[VEC], rs[VEC], gm[VEC], bt[VEC], m1[VEC], m2[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            int c = cv * VEC + e;
            mu[e] = stats[((size_t)n * C + c) * 2]; rs[e] = stats[((size_t)n * C + c) * 2 + 1];
            gm[e] = gamma[c]; bt[e] = beta[c];
            A[e] = gm[e] * rs[e]; B[e] = bt[e] - mu[e] * A[e];
            if (BWD) { m1[e] = sums[((size_t)n * C + c) * 2]; m2[e] = sums[((size_t)n * C + c) * 2 + 1]; }
        }
        act_dispatch(act, [&](auto act_c) {
            constexpr int ACT = decltype(act_c)::value;
            auto sweep = [&](auto res_c) {
                constexpr bool RES = decltype(res_c)::value;
                auto one = [&](const u32x4& xr, const u32x4& rr, const float* gv, size_t off) {
                    float xv[VEC], o[VEC];
                    ET<T>::unpack(xr, xv);
                    if (!BWD) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) o[e] = act_apply_c<ACT>(xv[e] * A[e] + B[e], leak);
                        if (RES) {
                            float rv[VEC];
                            ET<T>::unpack(rr, rv);
#pragma unroll
                            for (int e = 0; e < VEC; ++e) o[e] += rv[e];
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            float xh = (xv[e] - mu[e]) * rs[e];
                            float g = gv[e] * act_grad_c<ACT>(gm[e] * xh + bt[e], leak);
                            o[e] = A[e] * (g - m1[e] - xh * m2[e]);
                        }
                    }
                    st16(out + off, ET<T>::pack(o));
                };
                const size_t base = ((size_t)n * HW * C + (size_t)cv * VEC) * sizeof(T), pstep = (size_t)C * sizeof(T);
                int64_t p = p0 + prow;
                for (; p + (IN_U - 1) * rows < p1; p += IN_U * rows) {      // IN_U pixels per trip, all loads first (see in_partial_kernel)
                    u32x4 xr[IN_U], rr[IN_U];
                    float gv[IN_U][BWD ? VEC : 1];
#pragma unroll
                    for (int u = 0; u < IN_U; ++u) {
                        const size_t off = base + (size_t)(p + u * rows) * pstep;
                        xr[u] = (IN_NT & (BWD ? 2 : 1)) ? ld16_nt(x + off) : ld16(x + off);
                        if (RES) rr[u] = (IN_NT & 8) ? ld16_nt(residual + off) : ld16(residual + off);
                    }
                    if (BWD) {
#pragma unroll
                        for (int u = 0; u < IN_U; ++u) in_load_grad<T, TG>(dy, (base + (size_t)(p + u * rows) * pstep) / sizeof(T), gv[u]);
                    }
#pragma unroll
                    for (int u = 0; u < IN_U; ++u) one(xr[u], rr[u], gv[u], base + (size_t)(p + u * rows) * pstep);
                }
                for (; p < p1; p += rows) {
                    const size_t off = base + (size_t)p * pstep;
                    float gv[BWD ? VEC : 1];
                    const u32x4 xr = (IN_NT & (BWD ? 2 : 1)) ? ld16_nt(x + off) : ld16(x + off);
                    u32x4 rr = xr;
                    if (RES) rr = (IN_NT & 8) ? ld16_nt(residual + off) : ld16(residual + off);
                    if (BWD) in_load_grad<T, TG, (IN_NT & 4) != 0>(dy, off / sizeof(T), gv);
                    one(xr, rr, gv, off);
                }
            };
            if (!BWD && residual) sweep(std::true_type{}); else sweep(std::false_type{});
        });
    }
}


// -------------------------------------------------------------------------------------------------
// Small maps (HW <= IN_FUSED_MAXHW = 512 pixels: the discriminator tail, module.py:296-309; at 2048 pixels the serial
// walk of a block over its slab is already slower than the split kernels): one block owns a slab of IN_CVB channel
// vectors of one image and does both passes itself -- statistics, then the apply pass over the same (L2-resident)
// pixels -- in ONE launch instead of three or four; the split kernels above are launch-latency bound on these
// (20 us for a 0.5 MB tensor).  Same arithmetic order inside a block every run -> deterministic.
// -------------------------------------------------------------------------------------------------
#define IN_CVB 4
#define IN_FUSED_MAXHW 512

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void in_fused_small_kernel(const char* x, const char* dy, const char* residual, const float* gamma,
                                                             const float* beta, float* stats, float* tot, char* out,
                                                             int64_t HW, int C, float eps, int act, float leak, InSplit sp) {
    constexpr int VEC = ET<T>::VEC;
    constexpr int ROWS = 256 / IN_CVB;
    const int CV = C / VEC;
    const int n = blockIdx.y;
    if (n >= sp.nsplit) { gamma = sp.gamma2; beta = sp.beta2; }
    const int cvl = threadIdx.x % IN_CVB, prow = threadIdx.x / IN_CVB;
    const int cv = blockIdx.x * IN_CVB + cvl;
    const bool live = cv < CV;
    using AccT = InAcc<T>;
    __shared__ AccT red[256][2 * VEC + 1];
    __shared__ float sh_a[IN_CVB * VEC], sh_b[IN_CVB * VEC];

    float mu[VEC], rs[VEC], gm[VEC], bt[VEC];
    if (live) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int c = cv * VEC + e;
            gm[e] = gamma[c]; bt[e] = beta[c];
            if (BWD) { mu[e] = stats[((size_t)n * C + c) * 2]; rs[e] = stats[((size_t)n * C + c) * 2 + 1]; }
        }
    }
    AccT s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s1[e] = s2[e] = (AccT)0;
    if (live)
        for (int64_t p = prow; p < HW; p += ROWS) {
            const size_t off = (((size_t)n * HW + p) * C + (size_t)cv * VEC) * sizeof(T);
            float xv[VEC];
            ET<T>::unpack(ld16(x + off), xv);
            if (!BWD) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) { s1[e] += (AccT)xv[e]; s2[e] += (AccT)xv[e] * (AccT)xv[e]; }
            } else {
                float gv[VEC];
                ET<T>::unpack(ld16(dy + off), gv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float xh = (xv[e] - mu[e]) * rs[e];
                    const float g = gv[e] * (act == SGG_ACT_RELU ? (gm[e] * xh + bt[e] > 0.f ? 1.f : 0.f) : act == SGG_ACT_LRELU ? (gm[e] * xh + bt[e] > 0.f ? 1.f : leak) : 1.f);
                    s1[e] += (AccT)g; s2[e] += (AccT)g * (AccT)xh;
                }
            }
        }
#pragma unroll
    for (int e = 0; e < VEC; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][VEC + e] = s2[e]; }
    __syncthreads();
    if (threadIdx.x < IN_CVB * VEC) {                    // fixed-order combine over the pixel rows, in f64
        const int l = threadIdx.x / VEC, e = threadIdx.x % VEC;
        double a = 0.0, b = 0.0;
        for (int r = 0; r < ROWS; ++r) { a += (double)red[r * IN_CVB + l][e]; b += (double)red[r * IN_CVB + l][VEC + e]; }
        const int c = (blockIdx.x * IN_CVB + l) * VEC + e;
        if (c < C) {
            const size_t i = ((size_t)n * C + c) * 2;
            if (!BWD) {
                const double mean = a / (double)HW;
                double var = b / (double)HW - mean * mean;
                if (var < 0.0) var = 0.0;
                const float mf = (float)mean, rf = (float)(1.0 / sqrt(var + (double)eps));
                stats[i] = mf; stats[i + 1] = rf;
                sh_a[threadIdx.x] = mf; sh_b[threadIdx.x] = rf;
            } else {
                tot[i] = (float)a; tot[i + 1] = (float)b;
                sh_a[threadIdx.x] = (float)(a / (double)HW); sh_b[threadIdx.x] = (float)(b / (double)HW);
            }
        }
    }
    __syncthreads();
    if (!live) return;
    float A[VEC], B[VEC], m1[VEC], m2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if (!BWD) { mu[e] = sh_a[cvl * VEC + e]; rs[e] = sh_b[cvl * VEC + e]; }
        else { m1[e] = sh_a[cvl * VEC + e]; m2[e] = sh_b[cvl * VEC + e]; }
        A[e] = gm[e] * rs[e]; B[e] = bt[e] - mu[e] * A[e];
    }
    act_dispatch(act, [&](auto act_c) {
        constexpr int ACT = decltype(act_c)::value;
        for (int64_t p = prow; p < HW; p += ROWS) {
            const size_t off = (((size_t)n * HW + p) * C + (size_t)cv * VEC) * sizeof(T);
            float xv[VEC], o[VEC];
            ET<T>::unpack(ld16(x + off), xv);
            if (!BWD) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = act_apply_c<ACT>(xv[e] * A[e] + B[e], leak);
                if (residual) {
                    float rv[VEC];
                    ET<T>::unpack(ld16(residual + off), rv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) o[e] += rv[e];
                }
            } else {
                float gv[VEC];
                ET<T>::unpack(ld16(dy + off), gv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float xh = (xv[e] - mu[e]) * rs[e];
                    const float g = gv[e] * act_grad_c<ACT>(gm[e] * xh + bt[e], leak);
                    o[e] = A[e] * (g - m1[e] - xh * m2[e]);
                }
            }
            st16(out + off, ET<T>::pack(o));
        }
    });
}

__global__ void in_param_grad_kernel(InParamGrad g, int C, InSplit sp) { in_param_grad(g, C, sp); }


// -------------------------------------------------------------------------------------------------
// Skip added BEFORE the activation: y = act(gamma*xhat + beta + skip) -- generator_unet's d3 / d7 (module.py:181-184,
// 199-202: IN, add([., e5]), Activation('relu')).  The forward is the statistics pass / finalize above plus its own apply
// kernel; the backward takes the stored OUTPUT y: dz = dy * act'(y) (relu / lrelu keep the sign, so act'(y) == act'(z)) is
// computed once, in the statistics pass, and stored -- it is the skip path's gradient and the input of the unchanged
// act-NONE apply pass (in_apply_kernel<T, true>), which then reads dz and x only.
// -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void in_apply_skip_kernel(const char* x, const char* skip, const float* gamma, const float* beta,
                                                            const float* stats, char* out, int64_t HW, int C, int rows_per_block,
                                                            int act, float leak, InSplit sp) {
    constexpr int VEC = ET<T>::VEC;
    const int CV = C / VEC;
    const int n = blockIdx.y;
    if (n >= sp.nsplit) { gamma = sp.gamma2; beta = sp.beta2; }      // the second network's images (block-uniform)
    const int64_t p0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t p1 = p0 + rows_per_block < HW ? p0 + rows_per_block : HW;
    for (int cvb = 0; cvb < CV; cvb += 256) {
        const int lanes = CV - cvb < 256 ? CV - cvb : 256;
        const int rows = 256 / lanes;
        const int cv = cvb + (int)(threadIdx.x % lanes), prow = threadIdx.x / lanes;
        if (prow >= rows) continue;
        float A[VEC], B[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int c = cv * VEC + e;
            const float mu = stats[((size_t)n * C + c) * 2], rs = stats[((size_t)n * C + c) * 2 + 1];
            A[e] = gamma[c] * rs; B[e] = beta[c] - mu * A[e];
        }
        act_dispatch(act, [&](auto act_c) {
            constexpr int ACT = decltype(act_c)::value;
            auto one = [&](const u32x4& xr, const u32x4& sr, size_t off) {
                float xv[VEC], sv[VEC], o[VEC];
                ET<T>::unpack(xr, xv);
                ET<T>::unpack(sr, sv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = act_apply_c<ACT>(xv[e] * A[e] + B[e] + sv[e], leak);
                st16(out + off, ET<T>::pack(o));
            };
            const size_t base = ((size_t)n * HW * C + (size_t)cv * VEC) * sizeof(T), pstep = (size_t)C * sizeof(T);
            int64_t p = p0 + prow;
            for (; p + 3 * rows < p1; p += 4 * rows) {               // 4 pixels per trip, all loads first (see in_partial_kernel)
                u32x4 xr[4], sr[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const size_t off = base + (size_t)(p + u * rows) * pstep;
                    xr[u] = ld16_nt(x + off);
                    sr[u] = ld16_nt(skip + off);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) one(xr[u], sr[u], base + (size_t)(p + u * rows) * pstep);
            }
            for (; p < p1; p += rows) {
                const size_t off = base + (size_t)p * pstep;
                one(ld16_nt(x + off), ld16_nt(skip + off), off);
            }
        });
    }
}

// Backward statistics pass of the skip form: dz = dy * act'(y) is stored to dz_out, and the per-chunk (sum dz, sum dz*xhat)
// rows are written in the layout of in_partial_kernel (fixed per-thread pixel order, fixed combine order -> deterministic).
template <typename T>
__global__ __launch_bounds__(256) void in_skip_bwd_partial_kernel(const char* x, const char* dy, const char* y, const float* stats,
                                                                  char* dz_out, float* partial, int64_t HW, int C, int chunks, int rpc,
                                                                  int act, float leak) {
    constexpr int VEC = ET<T>::VEC;
    const int CV = C / VEC;
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int64_t p0 = (int64_t)chunk * rpc;
    const int64_t p1 = p0 + rpc < HW ? p0 + rpc : HW;
    using AccT = InAcc<T>;
    __shared__ AccT red[256][2 * VEC + 1];
    for (int cvb = 0; cvb < CV; cvb += 256) {
        const int lanes = CV - cvb < 256 ? CV - cvb : 256;
        const int rows = 256 / lanes;
        const int cv = cvb + (int)(threadIdx.x % lanes), prow = threadIdx.x / lanes;
        AccT s1[VEC], s2[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) s1[e] = s2[e] = (AccT)0;
        if (prow < rows) {
            float mu[VEC], rs[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int c = cv * VEC + e;
                mu[e] = stats[((size_t)n * C + c) * 2]; rs[e] = stats[((size_t)n * C + c) * 2 + 1];
            }
            act_dispatch(act, [&](auto act_c) {
                constexpr int ACT = decltype(act_c)::value;
                auto one = [&](const u32x4& xr, const u32x4& gr, const u32x4& yr, size_t off) {
                    float xv[VEC], gv[VEC], yv[VEC], dz[VEC];
                    ET<T>::unpack(xr, xv);
                    ET<T>::unpack(gr, gv);
                    ET<T>::unpack(yr, yv);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) dz[e] = gv[e] * act_grad_c<ACT>(yv[e], leak);
                    const u32x4 dzr = ET<T>::pack(dz);
                    st16(dz_out + off, dzr);
                    // the sums are taken over the STORED dz (what the apply pass reads back), so both passes see the same values
                    ET<T>::unpack(dzr, dz);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float xh = (xv[e] - mu[e]) * rs[e];
                        s1[e] += (AccT)dz[e]; s2[e] += (AccT)dz[e] * (AccT)xh;
                    }
                };
                const size_t base = ((size_t)n * HW * C + (size_t)cv * VEC) * sizeof(T), pstep = (size_t)C * sizeof(T);
                int64_t p = p0 + prow;
                for (; p + rows < p1; p += 2 * rows) {                 // 2 pixels per trip (three tensors read), loads first
                    u32x4 xr[2], gr[2], yr[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const size_t off = base + (size_t)(p + u * rows) * pstep;
                        xr[u] = ld16(x + off); gr[u] = ld16_nt(dy + off); yr[u] = ld16_nt(y + off);
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) one(xr[u], gr[u], yr[u], base + (size_t)(p + u * rows) * pstep);
                }
                for (; p < p1; p += rows) {
                    const size_t off = base + (size_t)p * pstep;
                    one(ld16(x + off), ld16_nt(dy + off), ld16_nt(y + off), off);
                }
            });
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][VEC + e] = s2[e]; }
        __syncthreads();
        for (int item = threadIdx.x; item < lanes * VEC; item += 256) {
            const int l = item / VEC, e = item % VEC;
            AccT a = (AccT)0, b = (AccT)0;
            for (int r = 0; r < rows; ++r) { a += red[r * lanes + l][e]; b += red[r * lanes + l][VEC + e]; }
            const int c = (cvb + l) * VEC + e;
            const size_t o = (((size_t)n * chunks + chunk) * C + c) * 2;
            partial[o] = (float)a; partial[o + 1] = (float)b;
        }
        __syncthreads();
    }
}

// -------------------------------------------------------------------------------------------------
// Host side.  Every entry point fills one InCall and runs in_forward or in_backward, which validate, carve the workspace
// (partial[N][chunks][C][2], absent when the caller brings the rows; then sums[N][C][2] and tot[N][C][2], backward only) and
// derive the grids once, then launch the passes the call's fields select.  DESIGN.md section 3 has the table of forms.
// -------------------------------------------------------------------------------------------------
struct InCall {
    const void* x = nullptr; const float* gamma = nullptr; const float* beta = nullptr;
    float* stats = nullptr;                        // (mean, rstd)[N][C]: written forward, read backward
    void* out = nullptr;                           // y forward, dx backward
    int N = 0; int64_t HW = 0; int C = 0; float eps = 0.f; int act = SGG_ACT_NONE; float leak = 0.f; int dtype = SGG_F32;
    void* ws = nullptr; size_t ws_bytes = 0; void* stream = nullptr;
    bool pair = false; InSplit sp = {nullptr, nullptr, nullptr, nullptr, 0x7fffffff};      // one network unless in_pair() fills it
    bool with_skip = false;                        // y = act(gamma*xhat + beta + skip): addend is the skip; backward takes y_in, writes dskip
    const void* addend = nullptr;                  // forward: the residual (added after the activation; optional) or the skip
    const void* y_in = nullptr; void* dskip = nullptr;
    bool with_partial = false; const float* partial = nullptr; int chunks = 0;             // statistics rows of the producing conv
    const void* dy = nullptr; bool dy_f32 = false; // backward; dy_f32: mixed mode (bf16 tensors, f32 gradient)
    float* dgamma = nullptr; float* dbeta = nullptr; int C_real = 0, accumulate = 0;
};
static InCall in_fwd_call(const void* x, const float* gamma, const float* beta, const void* addend, bool with_skip, void* y, float* stats,
                          int N, int64_t HW, int C, float eps, int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream) {
    InCall c;
    c.x = x; c.gamma = gamma; c.beta = beta; c.addend = addend; c.with_skip = with_skip; c.out = y; c.stats = stats; c.N = N; c.HW = HW; c.C = C;
    c.eps = eps; c.act = act; c.leak = leak; c.dtype = dtype; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
    return c;
}
static InCall in_bwd_call(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats, void* dx, float* dgamma,
                          float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak, int dtype,
                          void* ws, size_t ws_bytes, void* stream) {
    InCall c;
    c.dy = dy; c.x = x; c.gamma = gamma; c.beta = beta; c.stats = (float*)stats; c.out = dx; c.dgamma = dgamma; c.dbeta = dbeta; c.N = N; c.HW = HW;
    c.C = C; c.C_real = C_real; c.accumulate = accumulate; c.act = act; c.leak = leak; c.dtype = dtype; c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
    return c;
}
static void in_rows(InCall& c, const float* partial, int chunks) { c.with_partial = true; c.partial = partial; c.chunks = chunks; }
// two networks on one stacked batch, for forward and backward alike (forward: no dgamma2 / dbeta2)
static void in_pair(InCall& c, const float* gamma2, const float* beta2, float* dgamma2, float* dbeta2, int nsplit) {
    c.pair = true; c.sp.gamma2 = gamma2; c.sp.beta2 = beta2; c.sp.dgamma2 = dgamma2; c.sp.dbeta2 = dbeta2; c.sp.nsplit = nsplit;
}
static inline bool in_pair_ok(const InCall& c) { return !c.pair || (c.sp.gamma2 && c.sp.beta2 && c.sp.nsplit > 0 && c.sp.nsplit < c.N); }

static bool in_use_fused(int64_t HW) {
    const int mx = sgg_config().in_fused_maxhw;
    return HW <= (mx >= 0 ? mx : IN_FUSED_MAXHW);
}

static int in_rows_per_block(int N, int64_t HW) {
    // aim for >= 2048 blocks of >= 64 pixels
    int64_t r = HW * N / 2048;
    if (r < 64) r = 64;
    if (r > 4096) r = 4096;
    return (int)r;
}
static inline dim3 in_apply_grid(const InCall& c, int rpb) { return dim3((unsigned)((c.HW + rpb - 1) / rpb), c.N); }

// ---- the instantiation a call's dtype selects, one helper per kernel family (the specialisations of a family share one type)
static auto in_partial_fn(const InCall& c, bool bwd) {
    if (c.dtype == SGG_F32) return bwd ? in_partial_kernel<float, true> : in_partial_kernel<float, false>;
    if (c.dy_f32) return in_partial_kernel<bf16, true, float>;
    return bwd ? in_partial_kernel<bf16, true> : in_partial_kernel<bf16, false>;
}
static auto in_apply_fn(const InCall& c, bool bwd) {
    if (c.dtype == SGG_F32) return bwd ? in_apply_kernel<float, true> : in_apply_kernel<float, false>;
    if (c.dy_f32) return in_apply_kernel<bf16, true, float>;
    return bwd ? in_apply_kernel<bf16, true> : in_apply_kernel<bf16, false>;
}
static auto in_fused_fn(const InCall& c, bool bwd) {
    if (c.dtype == SGG_F32) return bwd ? in_fused_small_kernel<float, true> : in_fused_small_kernel<float, false>;
    return bwd ? in_fused_small_kernel<bf16, true> : in_fused_small_kernel<bf16, false>;
}
static auto in_apply_skip_fn(const InCall& c) { return c.dtype == SGG_F32 ? in_apply_skip_kernel<float> : in_apply_skip_kernel<bf16>; }
static auto in_skip_bwd_partial_fn(const InCall& c) { return c.dtype == SGG_F32 ? in_skip_bwd_partial_kernel<float> : in_skip_bwd_partial_kernel<bf16>; }

// ---- the passes, each launched from here only
// statistics: per-chunk (sum, sumsq) forward, (sum g, sum g*xhat) backward; the skip backward also stores dz to dskip
static void in_launch_stats(const InCall& c, bool bwd, float* partial, int chunks) {
    const dim3 gp(chunks, c.N);
    const int rpc = in_rows_per_chunk(c.HW);
    hipStream_t s = (hipStream_t)c.stream;
    if (bwd && c.with_skip)
        hipLaunchKernelGGL(in_skip_bwd_partial_fn(c), gp, dim3(256), 0, s, (const char*)c.x, (const char*)c.dy, (const char*)c.y_in,
                           (const float*)c.stats, (char*)c.dskip, partial, c.HW, c.C, chunks, rpc, c.act, c.leak);
    else
        hipLaunchKernelGGL(in_partial_fn(c, bwd), gp, dim3(256), 0, s, (const char*)c.x, (const char*)(bwd ? c.dy : nullptr), c.gamma, c.beta,
                           (const float*)(bwd ? c.stats : nullptr), partial, c.HW, c.C, chunks, rpc, c.act, c.leak, c.sp);
}
// forward: stats = (mean, rstd); backward: sums = the two sums / HW, tot = the raw sums
static void in_launch_finalize(const InCall& c, bool bwd, const float* partial, int chunks, float* sums, float* tot) {
    const dim3 gf((c.C + FIN_CH - 1) / FIN_CH, c.N);
    hipStream_t s = (hipStream_t)c.stream;
    if (bwd) hipLaunchKernelGGL(in_finalize_bwd_kernel, gf, dim3(1024), 0, s, partial, sums, tot, c.HW, c.C, chunks);
    else hipLaunchKernelGGL(in_finalize_fwd_kernel, gf, dim3(1024), 0, s, partial, c.stats, c.HW, c.C, chunks, c.eps);
}
// backward: g is the gradient the pass reads (dy, or the skip form's dskip) with the activation still to be undone by (act, leak).
// The bf16 forward launch is the timed one of this family (sgg_time_next_launch): a span then times the apply pass only.
static void in_launch_apply(const InCall& c, bool bwd, const void* g, int act, float leak, const float* sums, const InParamGrad& pg) {
    const int rpb = in_rows_per_block(c.N, c.HW);
    const dim3 ga = in_apply_grid(c, rpb);
    hipStream_t s = (hipStream_t)c.stream;
    const auto kern = in_apply_fn(c, bwd);
    auto launch = [&](auto... a) {
        if (!bwd && c.dtype == SGG_BF16) sgg_launch_timed(kern, ga, dim3(256), 0u, s, a...);
        else hipLaunchKernelGGL(kern, ga, dim3(256), 0, s, a...);
    };
    launch((const char*)c.x, (const char*)(bwd ? g : nullptr), (const char*)(bwd ? nullptr : c.addend), c.gamma, c.beta, (const float*)c.stats,
           sums, (char*)c.out, c.HW, c.C, rpb, act, leak, pg, c.sp);
}
static void in_launch_apply_skip(const InCall& c) {
    const int rpb = in_rows_per_block(c.N, c.HW);
    hipLaunchKernelGGL(in_apply_skip_fn(c), in_apply_grid(c, rpb), dim3(256), 0, (hipStream_t)c.stream, (const char*)c.x, (const char*)c.addend,
                       c.gamma, c.beta, (const float*)c.stats, (char*)c.out, c.HW, c.C, rpb, c.act, c.leak, c.sp);
}
static void in_launch_fused(const InCall& c, bool bwd, float* tot) {
    const int vec = c.dtype == SGG_BF16 ? 8 : 4;
    const dim3 gf((unsigned)((c.C / vec + IN_CVB - 1) / IN_CVB), c.N);
    hipLaunchKernelGGL(in_fused_fn(c, bwd), gf, dim3(256), 0, (hipStream_t)c.stream, (const char*)c.x, (const char*)(bwd ? c.dy : nullptr),
                       (const char*)(bwd ? nullptr : c.addend), c.gamma, c.beta, c.stats, tot, (char*)c.out, c.HW, c.C, bwd ? 0.f : c.eps,
                       c.act, c.leak, c.sp);
}

// One precedence for every form: arguments (SGG_EINVAL), then what no kernel does (SGG_EUNSUPPORTED), then the dtype
// (SGG_EINVAL), then the workspace (SGG_EWORKSPACE).  A refused call launches nothing.
static int in_forward(const InCall& c) {
    if (!c.x || !c.gamma || !c.beta || !c.out || !c.stats || c.N <= 0 || c.HW <= 0 || c.C <= 0 || c.C % SGG_CPAD || !in_pair_ok(c)) return SGG_EINVAL;
    if ((c.with_skip && !c.addend) || (c.with_partial && (!c.partial || c.chunks <= 0))) return SGG_EINVAL;
    if (c.act == SGG_ACT_TANH || c.dy_f32) return SGG_EUNSUPPORTED;
    if (c.dtype != SGG_BF16 && c.dtype != SGG_F32) return SGG_EINVAL;
    if (!c.with_partial && (!c.ws || c.ws_bytes < sgg_instnorm_workspace(c.N, c.HW, c.C))) return SGG_EWORKSPACE;
    if (!c.with_skip && !c.with_partial && in_use_fused(c.HW)) {
        in_launch_fused(c, false, nullptr);
        return sgg_check_launch();
    }
    const int chunks = c.with_partial ? c.chunks : in_chunks(c.HW);
    if (!c.with_partial) in_launch_stats(c, false, (float*)c.ws, chunks);
    in_launch_finalize(c, false, c.with_partial ? c.partial : (const float*)c.ws, chunks, nullptr, nullptr);
    if (c.with_skip) in_launch_apply_skip(c);
    else in_launch_apply(c, false, nullptr, c.act, c.leak, nullptr, InParamGrad{});
    return sgg_check_launch();
}

// Mixed mode (dy_f32): dy is f32, x / dx are bf16 (the gradient chain between the instance norms of the residual blocks stays f32:
// the norm backward subtracts the mean and the xhat-correlated part of dy, so a bf16 rounding of dy -- relative to dy, not
// to what is left of it -- is amplified there layer after layer).  Same passes as the plain backward.
static int in_backward(const InCall& c) {
    if (!c.dy || !c.x || !c.gamma || !c.beta || !c.stats || !c.out || !c.dgamma || !c.dbeta || c.N <= 0 || c.HW <= 0 || c.C <= 0 ||
        c.C % SGG_CPAD || c.C_real <= 0 || c.C_real > c.C || !in_pair_ok(c) || (c.pair && (!c.sp.dgamma2 || !c.sp.dbeta2))) return SGG_EINVAL;
    if (c.with_partial && (!c.partial || c.chunks <= 0)) return SGG_EINVAL;
    if (c.with_skip && (!c.y_in || !c.dskip || c.out == c.dskip || c.out == c.dy || c.out == c.x)) return SGG_EINVAL;
    if (c.act == SGG_ACT_TANH || (int)c.dy_f32 + (int)c.with_partial + (int)c.with_skip > 1) return SGG_EUNSUPPORTED;
    if (c.dtype != SGG_BF16 && (c.dtype != SGG_F32 || c.dy_f32)) return SGG_EINVAL;
    const int chunks = c.with_partial ? c.chunks : in_chunks(c.HW);
    const size_t own = c.with_partial ? 0 : (size_t)c.N * chunks * c.C * 2;          // floats of the partial rows this call writes
    if (!c.ws || c.ws_bytes < (own + (size_t)c.N * c.C * 4) * sizeof(float)) return SGG_EWORKSPACE;
    float* sums = (float*)c.ws + own;
    float* tot = sums + (size_t)c.N * c.C * 2;
    const InParamGrad pg{tot, c.dgamma, c.dbeta, c.N, c.C_real, c.accumulate};
    if (!c.dy_f32 && !c.with_partial && !c.with_skip && in_use_fused(c.HW)) {
        in_launch_fused(c, true, tot);
        hipLaunchKernelGGL(in_param_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)c.stream, pg, c.C, c.sp);
        return sgg_check_launch();
    }
    if (!c.with_partial) in_launch_stats(c, true, (float*)c.ws, chunks);
    in_launch_finalize(c, true, c.with_partial ? c.partial : (const float*)c.ws, chunks, sums, tot);
    // the skip form's statistics pass has undone the activation: dskip = dy * act'(y) is what the apply pass reads
    if (c.with_skip) in_launch_apply(c, true, c.dskip, SGG_ACT_NONE, 0.f, sums, pg);
    else in_launch_apply(c, true, c.dy, c.act, c.leak, sums, pg);
    return sgg_check_launch();
}

extern "C" {

size_t sgg_instnorm_workspace(int N, int64_t HW, int C) {
    if (N <= 0 || HW <= 0 || C <= 0) return 0;
    return ((size_t)N * in_chunks(HW) * C * 2 + (size_t)N * C * 4) * sizeof(float);
}

// ---- public entry points: one network, or two networks of the same shape stacked on the batch dimension ("pair": images
// 0..nsplit-1 use gamma/beta and add to dgamma/dbeta, the rest use gamma2/beta2 and dgamma2/dbeta2)
int sgg_instnorm_fwd(const void* x, const float* gamma, const float* beta, const void* residual, void* y, float* stats,
                     int N, int64_t HW, int C, float eps, int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream) {
    return in_forward(in_fwd_call(x, gamma, beta, residual, false, y, stats, N, HW, C, eps, act, leak, dtype, ws, ws_bytes, stream));
}
int sgg_instnorm_fwd_partial(const void* x, const float* gamma, const float* beta, const void* residual, void* y, float* stats,
                             const float* partial, int chunks, int N, int64_t HW, int C, float eps, int act, float leak, int dtype,
                             void* stream) {
    InCall c = in_fwd_call(x, gamma, beta, residual, false, y, stats, N, HW, C, eps, act, leak, dtype, nullptr, 0, stream);
    in_rows(c, partial, chunks);
    return in_forward(c);
}
int sgg_instnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats, void* dx,
                     float* dgamma, float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak,
                     int dtype, void* ws, size_t ws_bytes, void* stream) {
    return in_backward(in_bwd_call(dy, x, gamma, beta, stats, dx, dgamma, dbeta, N, HW, C, C_real, accumulate, act, leak, dtype, ws, ws_bytes, stream));
}
int sgg_instnorm_bwd_mixed(const float* dy, const void* x, const float* gamma, const float* beta, const float* stats, void* dx,
                           float* dgamma, float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak,
                           void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_bwd_call(dy, x, gamma, beta, stats, dx, dgamma, dbeta, N, HW, C, C_real, accumulate, act, leak, SGG_BF16, ws, ws_bytes, stream);
    c.dy_f32 = true;
    return in_backward(c);
}
int sgg_instnorm_bwd_partial(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats, void* dx,
                             float* dgamma, float* dbeta, const float* partial, int chunks, int N, int64_t HW, int C, int C_real,
                             int accumulate, int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_bwd_call(dy, x, gamma, beta, stats, dx, dgamma, dbeta, N, HW, C, C_real, accumulate, act, leak, dtype, ws, ws_bytes, stream);
    in_rows(c, partial, chunks);
    return in_backward(c);
}
// (mean, rstd)[N][C] from per-chunk (sum, sumsq) rows -- the finalize step of sgg_instnorm_fwd_partial on its own, for a
// consumer that applies the norm itself (sgg_conv2d_fwd_stats_normload)
int sgg_instnorm_finalize(const float* partial, int chunks, float* stats, int N, int64_t HW, int C, float eps, void* stream) {
    if (!partial || !stats || chunks <= 0 || N <= 0 || HW <= 0 || C <= 0 || C % SGG_CPAD) return SGG_EINVAL;
    InCall c;
    c.stats = stats; c.N = N; c.HW = HW; c.C = C; c.eps = eps; c.stream = stream;
    in_launch_finalize(c, false, partial, chunks, nullptr, nullptr);
    return sgg_check_launch();
}
int sgg_instnorm_fwd_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                          const void* residual, void* y, float* stats, int N, int64_t HW, int C, float eps, int act, float leak,
                          int dtype, void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_fwd_call(x, gamma, beta, residual, false, y, stats, N, HW, C, eps, act, leak, dtype, ws, ws_bytes, stream);
    in_pair(c, gamma2, beta2, nullptr, nullptr, nsplit);
    return in_forward(c);
}
int sgg_instnorm_fwd_partial_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                                  const void* residual, void* y, float* stats, const float* partial, int chunks, int N, int64_t HW, int C,
                                  float eps, int act, float leak, int dtype, void* stream) {
    InCall c = in_fwd_call(x, gamma, beta, residual, false, y, stats, N, HW, C, eps, act, leak, dtype, nullptr, 0, stream);
    in_rows(c, partial, chunks);
    in_pair(c, gamma2, beta2, nullptr, nullptr, nsplit);
    return in_forward(c);
}
int sgg_instnorm_bwd_pair(const void* dy, const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                          int nsplit, const float* stats, void* dx, float* dgamma, float* dbeta, float* dgamma2, float* dbeta2,
                          int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak, int dtype,
                          void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_bwd_call(dy, x, gamma, beta, stats, dx, dgamma, dbeta, N, HW, C, C_real, accumulate, act, leak, dtype, ws, ws_bytes, stream);
    in_pair(c, gamma2, beta2, dgamma2, dbeta2, nsplit);
    return in_backward(c);
}

// ---- skip added before the activation (generator_unet d3 / d7): y = act(gamma*xhat + beta + skip).  One network or two in
// lockstep on a stacked batch (the _pair entry points): the statistics passes and the backward's dz pass never read the
// affine parameters, so only the two apply kernels and the parameter-gradient sums pick a set by image index.
int sgg_instnorm_fwd_skip(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* stats,
                          int N, int64_t HW, int C, float eps, int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream) {
    return in_forward(in_fwd_call(x, gamma, beta, skip, true, y, stats, N, HW, C, eps, act, leak, dtype, ws, ws_bytes, stream));
}
int sgg_instnorm_fwd_skip_partial(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* stats,
                                  const float* partial, int chunks, int N, int64_t HW, int C, float eps, int act, float leak, int dtype,
                                  void* stream) {
    InCall c = in_fwd_call(x, gamma, beta, skip, true, y, stats, N, HW, C, eps, act, leak, dtype, nullptr, 0, stream);
    in_rows(c, partial, chunks);
    return in_forward(c);
}
int sgg_instnorm_bwd_skip(const void* dy, const void* y, const void* x, const float* gamma, const float* beta, const float* stats,
                          void* dx, void* dskip, float* dgamma, float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate,
                          int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_bwd_call(dy, x, gamma, beta, stats, dx, dgamma, dbeta, N, HW, C, C_real, accumulate, act, leak, dtype, ws, ws_bytes, stream);
    c.with_skip = true; c.y_in = y; c.dskip = dskip;
    return in_backward(c);
}
int sgg_instnorm_fwd_skip_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                               const void* skip, void* y, float* stats, int N, int64_t HW, int C, float eps, int act, float leak,
                               int dtype, void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_fwd_call(x, gamma, beta, skip, true, y, stats, N, HW, C, eps, act, leak, dtype, ws, ws_bytes, stream);
    in_pair(c, gamma2, beta2, nullptr, nullptr, nsplit);
    return in_forward(c);
}
int sgg_instnorm_fwd_skip_partial_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                                       const void* skip, void* y, float* stats, const float* partial, int chunks, int N, int64_t HW, int C,
                                       float eps, int act, float leak, int dtype, void* stream) {
    InCall c = in_fwd_call(x, gamma, beta, skip, true, y, stats, N, HW, C, eps, act, leak, dtype, nullptr, 0, stream);
    in_rows(c, partial, chunks);
    in_pair(c, gamma2, beta2, nullptr, nullptr, nsplit);
    return in_forward(c);
}
int sgg_instnorm_bwd_skip_pair(const void* dy, const void* y, const void* x, const float* gamma, const float* beta, const float* gamma2,
                               const float* beta2, int nsplit, const float* stats, void* dx, void* dskip, float* dgamma, float* dbeta,
                               float* dgamma2, float* dbeta2, int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak,
                               int dtype, void* ws, size_t ws_bytes, void* stream) {
    InCall c = in_bwd_call(dy, x, gamma, beta, stats, dx, dgamma, dbeta, N, HW, C, C_real, accumulate, act, leak, dtype, ws, ws_bytes, stream);
    c.with_skip = true; c.y_in = y; c.dskip = dskip;
    in_pair(c, gamma2, beta2, dgamma2, dbeta2, nsplit);
    return in_backward(c);
}

}  // extern "C"
