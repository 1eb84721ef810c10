// swd.hip -- sliced Wasserstein distance of Laplacian-pyramid patches (Karras et al. 2018, section 5): the unpaired
// realism score of the test pass.  Four entry points, the sort between the last two is the caller's (torch.sort):
//
//   sgg_swd_pyramid      8-bit colours -> the Laplacian pyramid of every image, float32, levels concatenated, each planar
//   sgg_swd_descriptors  7x7x3 patches of one level at Philox-drawn centres -> rows of 147 floats
//   sgg_swd_project      per-channel mean / deviation over a whole descriptor set, then the normalised rows times the directions
//   sgg_swd_distance     per direction the sum of |a - b| over two sorted rows
//
// Pyramid: t = [1,4,6,4,1]/16, mirror border without edge repeat (-1 -> 1, n -> n-2).  G_k = down(G_{k-1}) filters with t (x) t
// and keeps every second row / column from 0; up zero-stuffs to twice the size and filters with 4 (t (x) t) under the same
// mirror rule on the stuffed grid, Lap_{k-1} = G_{k-1} - up(G_k), Lap_{L-1} = G_{L-1}.  The Gaussian chain is kept in DOUBLE:
// the input has 8 bits, every down adds 8 fraction bits and up 6, at most 47 bits at five levels -- every intermediate is an
// exact dyadic rational, so no sum depends on its order, and the float32 store is the one rounding.
//
// Statistics and projections are double with a FIXED order: per thread in element order, a fixed shuffle tree per wave, the
// four waves in order, the chunks' partials in index order by a one-block fold.  No floating-point atomics, no allocation, no
// host sync: every call can be captured.
#include "common.h"
#include <math.h>

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_WAVES = SW_THREADS / SGG_WAVE;
constexpr int SW_MAX_LEVELS = 5;
constexpr int SW_MAX_HW = 1 << 22;
constexpr int SW_PATCH = 7, SW_R = 3;
constexpr int SW_PLANE = SW_PATCH * SW_PATCH;       // 49 values of a channel
constexpr int SW_K = 3 * SW_PLANE;                  // 147 values of a descriptor, (channel, y, x)
constexpr int SW_CHUNK = 256;                       // descriptor rows per partial sum
constexpr int SW_TM = 32, SW_TD = 128;              // rows x directions of a projection block
constexpr int SW_DPT = 16;                          // directions per thread
constexpr int SW_GRID_Y = 65535;

struct SwdOperand {
    const void* p;
    int kind, cs, vec;
};

__device__ inline double sw_wave_sum(double v) {    // a fixed tree: the same lanes meet in the same order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int sw_mirror(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p); }

// G_0: the quantised colours as doubles, planar.  blockIdx.y: the image.
__global__ __launch_bounds__(SW_THREADS) void swd_quant_kernel(const SwdOperand I, int HW, int64_t E, double* __restrict__ ws) {
    const int p = blockIdx.x * SW_THREADS + threadIdx.x;
    if (p >= HW) return;
    const int n = blockIdx.y;
    const int64_t i = (int64_t)n * HW + p;
    int r, g, b;
    if (I.kind == SGG_BF16) load_colour<SGG_BF16>(I.p, i, I.cs, I.vec != 0, r, g, b);           // I.kind is uniform
    else if (I.kind == SGG_F32) load_colour<SGG_F32>(I.p, i, I.cs, I.vec != 0, r, g, b);
    else load_colour<SGG_U8>(I.p, i, I.cs, false, r, g, b);
    double* g0 = ws + (int64_t)n * E;
    g0[p] = (double)r; g0[HW + p] = (double)g; g0[2 * HW + p] = (double)b;
}

// G_{k+1} from G_k (h x w -> h/2 x w/2).  blockIdx.y: the plane 3 n + c.  Rows first, then the column of row sums; the taps
// are small integers and the operands dyadic, so every product and sum is exact and the order is free.
__global__ __launch_bounds__(SW_THREADS) void swd_down_kernel(double* __restrict__ ws, int64_t E, int64_t off_f, int64_t off_c, int h, int w) {
    const int hc = h >> 1, wc = w >> 1;
    const int p = blockIdx.x * SW_THREADS + threadIdx.x;
    if (p >= hc * wc) return;
    const int n = blockIdx.y / 3, c = blockIdx.y - 3 * n;
    const int y = p / wc, x = p - y * wc;
    const double* src = ws + (int64_t)n * E + off_f + (int64_t)c * h * w;
    const int x0 = sw_mirror(2 * x - 2, w), x1 = sw_mirror(2 * x - 1, w), x2 = 2 * x, x3 = sw_mirror(2 * x + 1, w), x4 = sw_mirror(2 * x + 2, w);
    const double T[5] = {1.0, 4.0, 6.0, 4.0, 1.0};
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const double* row = src + (int64_t)sw_mirror(2 * y + a - 2, h) * w;
        acc += T[a] * ((row[x0] + row[x4]) + 4.0 * (row[x1] + row[x3]) + 6.0 * row[x2]);
    }
    ws[(int64_t)n * E + off_c + (int64_t)c * hc * wc + p] = acc * (1.0 / 256.0);
}

// one axis of up(): the coarse samples that the five taps around stuffed position y meet, and their weights (of 16).  The mirror
// keeps the parity of a position (the stuffed size is even), so an even y meets its three even neighbours with 1, 6, 1 and an
// odd y the two beside it with 4, 4.
__device__ inline void sw_up_taps(int y, int n, int* idx, double* wt) {
    if (y & 1) {
        idx[0] = (y - 1) >> 1; idx[1] = sw_mirror(y + 1, n) >> 1; idx[2] = idx[1];
        wt[0] = 4.0; wt[1] = 4.0; wt[2] = 0.0;
    } else {
        idx[0] = sw_mirror(y - 2, n) >> 1; idx[1] = y >> 1; idx[2] = sw_mirror(y + 2, n) >> 1;
        wt[0] = 1.0; wt[1] = 6.0; wt[2] = 1.0;
    }
}

// Lap_k = G_k - up(G_{k+1}) (LAST: Lap_k = G_k), rounded to float32 at the store.  blockIdx.y: the plane.
template <bool LAST>
__global__ __launch_bounds__(SW_THREADS) void swd_lap_kernel(const double* __restrict__ ws, int64_t E, int64_t off_f, int64_t off_c, int h, int w,
                                                            float* __restrict__ pyr) {
    const int p = blockIdx.x * SW_THREADS + threadIdx.x;
    if (p >= h * w) return;
    const int n = blockIdx.y / 3, c = blockIdx.y - 3 * n;
    const int64_t at = (int64_t)n * E + off_f + (int64_t)c * h * w + p;
    double v = ws[at];
    if (!LAST) {
        const int y = p / w, x = p - y * w;
        const int hc = h >> 1, wc = w >> 1;
        const double* src = ws + (int64_t)n * E + off_c + (int64_t)c * hc * wc;
        int yi[3], xi[3];
        double yw[3], xw[3];
        sw_up_taps(y, h, yi, yw);
        sw_up_taps(x, w, xi, xw);
        double up = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double* row = src + (int64_t)yi[a] * wc;
            up += yw[a] * (xw[0] * row[xi[0]] + xw[1] * row[xi[1]] + xw[2] * row[xi[2]]);
        }
        v -= up * (1.0 / 64.0);                       // 4 / 256
    }
    pyr[at] = (float)v;
}

struct SwU4 { uint32_t v[4]; };
__device__ inline SwU4 sw_philox4x32_10(SwU4 c, uint32_t k0, uint32_t k1) {     // Random123's constants, as diffaug.hip
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.v[0]), lo0 = 0xD2511F53u * c.v[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.v[2]), lo1 = 0xCD9E8D57u * c.v[2];
        SwU4 n;
        n.v[0] = hi1 ^ c.v[1] ^ k0; n.v[1] = lo1; n.v[2] = hi0 ^ c.v[3] ^ k1; n.v[3] = lo0;
        c = n;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}

// one thread per descriptor value.  blockIdx.y: the image of the call; every thread of a patch draws the patch's words again
// (ten rounds of integer work against 147 stores).
__global__ __launch_bounds__(SW_THREADS) void swd_descriptor_kernel(const float* __restrict__ pyr, int64_t E, int64_t off, int h, int w, int patches,
                                                                   uint32_t level, uint32_t seed, uint32_t g0, float* __restrict__ desc) {
    const uint32_t e = blockIdx.x * SW_THREADS + threadIdx.x;
    if (e >= (uint32_t)patches * SW_K) return;
    const uint32_t p = e / SW_K, k = e - p * SW_K;
    const int i = blockIdx.y;
    SwU4 ctr;
    ctr.v[0] = g0 + (uint32_t)i; ctr.v[1] = level; ctr.v[2] = p >> 1; ctr.v[3] = 0u;
    const SwU4 r = sw_philox4x32_10(ctr, seed, 1u);
    const uint32_t wy = (p & 1u) ? r.v[2] : r.v[0], wx = (p & 1u) ? r.v[3] : r.v[1];
    const int cy = SW_R + (int)__umulhi(wy, (uint32_t)(h - 2 * SW_R)), cx = SW_R + (int)__umulhi(wx, (uint32_t)(w - 2 * SW_R));
    const int c = k / SW_PLANE, q = k - c * SW_PLANE, dy = q / SW_PATCH, dx = q - dy * SW_PATCH;
    const float* plane = pyr + (int64_t)i * E + off + (int64_t)c * h * w;
    desc[((int64_t)i * patches + p) * SW_K + k] = plane[(int64_t)(cy - SW_R + dy) * w + (cx - SW_R + dx)];
}

__device__ inline int sw_channel(int k) { return k >= 2 * SW_PLANE ? 2 : (k >= SW_PLANE ? 1 : 0); }

// part[chunk][3]: per channel the sum of x (DEV: of (x - mean)^2) over the chunk's SW_CHUNK rows
template <bool DEV>
__global__ __launch_bounds__(SW_THREADS) void swd_sum_kernel(const float* __restrict__ desc, int64_t M, const double* __restrict__ moments,
                                                            double* __restrict__ part) {
    __shared__ double red[3][SW_WAVES];
    const int64_t row0 = (int64_t)blockIdx.x * SW_CHUNK;
    const int cnt = (int)min((int64_t)SW_CHUNK, M - row0) * SW_K;
    const float* src = desc + row0 * SW_K;
    double mean[3] = {0.0, 0.0, 0.0};
    if (DEV) { mean[0] = moments[0]; mean[1] = moments[2]; mean[2] = moments[4]; }
    double acc[3] = {0.0, 0.0, 0.0};
    for (int e = threadIdx.x; e < cnt; e += SW_THREADS) {
        const int c = sw_channel(e % SW_K);
        double x = (double)src[e];
        if (DEV) {
            x -= c == 0 ? mean[0] : (c == 1 ? mean[1] : mean[2]);
            x *= x;
        }
        acc[0] += c == 0 ? x : 0.0; acc[1] += c == 1 ? x : 0.0; acc[2] += c == 2 ? x : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double s = sw_wave_sum(acc[c]);
        if ((threadIdx.x & (SGG_WAVE - 1)) == 0) red[c][threadIdx.x / SGG_WAVE] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = red[threadIdx.x][0];
#pragma unroll
        for (int wv = 1; wv < SW_WAVES; ++wv) s += red[threadIdx.x][wv];
        part[(int64_t)blockIdx.x * 3 + threadIdx.x] = s;
    }
}

// one block: the partials in index order.  stage 0 writes the mean, stage 1 the population standard deviation.
__global__ void swd_fold_kernel(const double* __restrict__ part, int chunks, double count, int stage, double* __restrict__ moments) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    double s = 0.0;
    for (int i = 0; i < chunks; ++i) s += part[(int64_t)i * 3 + c];
    moments[2 * c + stage] = stage ? sqrt(s / count) : s / count;
}

// proj[d][m] = sum_k z[m][k] * dirs[k][d], k ascending, one product and one add per term in double.  A block owns SW_TM rows and
// SW_TD directions: the rows are normalised once into LDS ([k][row], so the 32 lanes of a half wave read consecutive doubles),
// a thread keeps SW_DPT directions of one row.  FULL: the block's directions all exist and dirs' rows are 16-byte aligned.
template <bool FULL>
__global__ __launch_bounds__(SW_THREADS) void swd_project_kernel(const float* __restrict__ desc, int64_t M, const float* __restrict__ dirs, int D,
                                                                const double* __restrict__ moments, double* __restrict__ proj) {
    __shared__ double zs[SW_K][SW_TM];
    const int64_t m0 = (int64_t)blockIdx.x * SW_TM;
    const int rows = (int)min((int64_t)SW_TM, M - m0);
    const double mean[3] = {moments[0], moments[2], moments[4]}, sd[3] = {moments[1], moments[3], moments[5]};
    const float* src = desc + m0 * SW_K;
    for (int e = threadIdx.x; e < SW_TM * SW_K; e += SW_THREADS) {
        const int ml = e / SW_K, k = e - ml * SW_K;
        const int c = sw_channel(k);
        double z = 0.0;
        if (ml < rows) {
            const double mu = c == 0 ? mean[0] : (c == 1 ? mean[1] : mean[2]), s = c == 0 ? sd[0] : (c == 1 ? sd[1] : sd[2]);
            if (s != 0.0) z = ((double)src[e] - mu) / s;                              // a constant channel: zeros
        }
        zs[k][ml] = z;
    }
    __syncthreads();
    const int ml = threadIdx.x & (SW_TM - 1);
    const int dbase = blockIdx.y * SW_TD + (threadIdx.x / SW_TM) * SW_DPT;
    double acc[SW_DPT];
#pragma unroll
    for (int j = 0; j < SW_DPT; ++j) acc[j] = 0.0;
    for (int k = 0; k < SW_K; ++k) {
        const double z = zs[k][ml];
        const float* dr = dirs + (int64_t)k * D + dbase;
        float dv[SW_DPT];
        if (FULL) {
#pragma unroll
            for (int j = 0; j < SW_DPT; j += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(dr + j);
                dv[j] = v[0]; dv[j + 1] = v[1]; dv[j + 2] = v[2]; dv[j + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < SW_DPT; ++j) dv[j] = dbase + j < D ? dr[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < SW_DPT; ++j) acc[j] += z * (double)dv[j];
    }
    if (ml < rows) {
#pragma unroll
        for (int j = 0; j < SW_DPT; ++j)
            if (FULL || dbase + j < D) proj[(int64_t)(dbase + j) * M + m0 + ml] = acc[j];
    }
}

// out[d] = sum_m |a[d][m] - b[d][m]|: one block per direction, thread t takes m = t, t + 256, ... in that order
__global__ __launch_bounds__(SW_THREADS) void swd_distance_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t M,
                                                                 double* __restrict__ out) {
    __shared__ double red[SW_WAVES];
    const double* ra = a + (int64_t)blockIdx.x * M;
    const double* rb = b + (int64_t)blockIdx.x * M;
    double acc = 0.0;
    for (int64_t m = threadIdx.x; m < M; m += SW_THREADS) acc += fabs(ra[m] - rb[m]);
    acc = sw_wave_sum(acc);
    if ((threadIdx.x & (SGG_WAVE - 1)) == 0) red[threadIdx.x / SGG_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
#pragma unroll
        for (int wv = 1; wv < SW_WAVES; ++wv) s += red[wv];
        out[blockIdx.x] = s;
    }
}

bool sw_shape_ok(int H, int W, int levels) {
    if (levels < 1 || levels > SW_MAX_LEVELS || H <= 0 || W <= 0) return false;
    const int mask = (1 << (levels - 1)) - 1;
    if ((H & mask) || (W & mask)) return false;
    if ((H >> (levels - 1)) < SW_PATCH || (W >> (levels - 1)) < SW_PATCH) return false;
    return (int64_t)H * W <= SW_MAX_HW;
}
int64_t sw_level_off(int H, int W, int level) {     // elements of an image's levels in front of `level`
    int64_t off = 0;
    for (int l = 0; l < level; ++l) off += 3 * (int64_t)(H >> l) * (W >> l);
    return off;
}
int sw_blocks(int64_t n) { return (int)((n + SW_THREADS - 1) / SW_THREADS); }
int64_t sw_chunks(int64_t M) { return (M + SW_CHUNK - 1) / SW_CHUNK; }

}  // namespace

extern "C" size_t sgg_swd_pyramid_elems(int H, int W, int levels) {
    return sw_shape_ok(H, W, levels) ? (size_t)sw_level_off(H, W, levels) : 0;
}

extern "C" size_t sgg_swd_pyramid_workspace(int N, int H, int W, int levels) {
    if (N <= 0) return 0;
    return (size_t)N * sgg_swd_pyramid_elems(H, W, levels) * sizeof(double);
}

extern "C" size_t sgg_swd_project_workspace(int64_t M) { return M > 0 ? (size_t)sw_chunks(M) * 3 * sizeof(double) : 0; }

extern "C" int sgg_swd_pyramid(const void* img, int kind, int cstride, int N, int H, int W, int levels, float* pyr, void* ws, size_t ws_bytes,
                               void* stream) {
    if (!img || !pyr || !ws || N <= 0 || ((uintptr_t)pyr & 3) || ((uintptr_t)ws & 7)) return SGG_EINVAL;
    SwdOperand I;
    if (kind == SGG_U8) {
        if (cstride != 3 && cstride != 4) return SGG_EINVAL;
        I.vec = 0;
    } else if (kind == SGG_F32 || kind == SGG_BF16) {
        if (cstride < 3) return SGG_EINVAL;
        if ((uintptr_t)img & (kind == SGG_F32 ? 3 : 1)) return SGG_EINVAL;
        I.vec = cstride == SGG_CPAD && ((uintptr_t)img & 15) == 0;
    } else {
        return SGG_EINVAL;
    }
    I.p = img; I.kind = kind; I.cs = cstride;
    if (!sw_shape_ok(H, W, levels)) return SGG_EUNSUPPORTED;
    if ((int64_t)N * 3 > SW_GRID_Y) return SGG_EUNSUPPORTED;                            // the grid: one plane per blockIdx.y
    if (ws_bytes < sgg_swd_pyramid_workspace(N, H, W, levels)) return SGG_EWORKSPACE;
    const int64_t E = sw_level_off(H, W, levels);
    double* g = (double*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(swd_quant_kernel, dim3(sw_blocks((int64_t)H * W), N), dim3(SW_THREADS), 0, s, I, H * W, E, g);
    for (int l = 0; l + 1 < levels; ++l) {
        const int h = H >> l, w = W >> l;
        hipLaunchKernelGGL(swd_down_kernel, dim3(sw_blocks((int64_t)(h >> 1) * (w >> 1)), 3 * N), dim3(SW_THREADS), 0, s, g, E,
                           sw_level_off(H, W, l), sw_level_off(H, W, l + 1), h, w);
    }
    for (int l = 0; l < levels; ++l) {
        const int h = H >> l, w = W >> l;
        const dim3 grid(sw_blocks((int64_t)h * w), 3 * N);
        if (l + 1 < levels)
            hipLaunchKernelGGL(swd_lap_kernel<false>, grid, dim3(SW_THREADS), 0, s, (const double*)g, E, sw_level_off(H, W, l),
                               sw_level_off(H, W, l + 1), h, w, pyr);
        else
            hipLaunchKernelGGL(swd_lap_kernel<true>, grid, dim3(SW_THREADS), 0, s, (const double*)g, E, sw_level_off(H, W, l), (int64_t)0, h, w, pyr);
    }
    return sgg_check_launch();
}

extern "C" int sgg_swd_descriptors(const float* pyr, int N, int H, int W, int levels, int level, int patches, uint32_t seed, int64_t image_offset,
                                   float* desc, void* stream) {
    if (!pyr || !desc || N <= 0 || patches <= 0 || level < 0 || image_offset < 0 || ((uintptr_t)pyr & 3) || ((uintptr_t)desc & 3)) return SGG_EINVAL;
    if (!sw_shape_ok(H, W, levels)) return SGG_EUNSUPPORTED;
    if (level >= levels) return SGG_EINVAL;
    if (N > SW_GRID_Y || (int64_t)patches * SW_K > 0x7fffffff) return SGG_EUNSUPPORTED;  // the grid: one image per blockIdx.y
    hipLaunchKernelGGL(swd_descriptor_kernel, dim3(sw_blocks((int64_t)patches * SW_K), N), dim3(SW_THREADS), 0, (hipStream_t)stream, pyr,
                       sw_level_off(H, W, levels), sw_level_off(H, W, level), H >> level, W >> level, patches, (uint32_t)level, seed,
                       (uint32_t)image_offset, desc);
    return sgg_check_launch();
}

extern "C" int sgg_swd_project(const float* desc, int64_t M, const float* dirs, int D, double* proj, double* moments, void* ws, size_t ws_bytes,
                               void* stream) {
    if (!desc || !dirs || !proj || !moments || !ws || M <= 0 || D <= 0) return SGG_EINVAL;
    if (((uintptr_t)desc & 3) || ((uintptr_t)dirs & 3) || ((uintptr_t)proj & 7) || ((uintptr_t)moments & 7) || ((uintptr_t)ws & 7)) return SGG_EINVAL;
    const int64_t tiles_m = (M + SW_TM - 1) / SW_TM, chunks = sw_chunks(M);
    const int tiles_d = (D + SW_TD - 1) / SW_TD;
    if (tiles_m > 0x7fffffff || tiles_d > SW_GRID_Y) return SGG_EUNSUPPORTED;            // the grid
    if (ws_bytes < sgg_swd_project_workspace(M)) return SGG_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    const double count = (double)M * (double)SW_PLANE;
    hipLaunchKernelGGL(swd_sum_kernel<false>, dim3((int)chunks), dim3(SW_THREADS), 0, s, desc, M, (const double*)moments, part);
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(SGG_WAVE), 0, s, (const double*)part, (int)chunks, count, 0, moments);
    hipLaunchKernelGGL(swd_sum_kernel<true>, dim3((int)chunks), dim3(SW_THREADS), 0, s, desc, M, (const double*)moments, part);
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(SGG_WAVE), 0, s, (const double*)part, (int)chunks, count, 1, moments);
    const dim3 grid((int)tiles_m, tiles_d);
    if (D % SW_TD == 0 && ((uintptr_t)dirs & 15) == 0)
        hipLaunchKernelGGL(swd_project_kernel<true>, grid, dim3(SW_THREADS), 0, s, desc, M, dirs, D, (const double*)moments, proj);
    else
        hipLaunchKernelGGL(swd_project_kernel<false>, grid, dim3(SW_THREADS), 0, s, desc, M, dirs, D, (const double*)moments, proj);
    return sgg_check_launch();
}

extern "C" int sgg_swd_distance(const double* sa, const double* sb, int D, int64_t M, double* out, void* stream) {
    if (!sa || !sb || !out || D <= 0 || M <= 0 || ((uintptr_t)sa & 7) || ((uintptr_t)sb & 7) || ((uintptr_t)out & 7)) return SGG_EINVAL;
    hipLaunchKernelGGL(swd_distance_kernel, dim3(D), dim3(SW_THREADS), 0, (hipStream_t)stream, sa, sb, M, out);
    return sgg_check_launch();
}
