// spectral.hip -- spectral normalisation of a network's conv kernels (include/sggan.h, "spectral norm"): one power iteration per
// layer and the gradient transform that goes with it, each for every layer of a network in one call (a device item table, as
// sgg_pack_conv_weights_batch has one).
//
// A layer's kernel is the row-major f32 matrix M (rows = R*S*C, K columns) as it lies in the parameter buffer.  The cost is bytes
// (35 MB for a full-width discriminator), so M is read ONCE per call: a block takes a band of SGG_SPECTRAL_BAND rows, one wave
// per row, a lane owning the columns {V * (lane + 64 q) + k}.  The wave forms t_i = row_i . u (double, butterfly over the lanes) and
// adds t_i * row_i to its per-lane column sums, which is Mt t restricted to the band; s = Mt v is that over |t|, so v is never
// needed while M is in flight.  The bands' shares are folded by a block per item and 64 columns, and one block per item finishes u and
// sigma.  Every sum is double and runs in an order fixed by the shapes alone: the same bits on every run.
#include "common.h"

namespace {

constexpr int SN_BAND = SGG_SPECTRAL_BAND;      // rows of M per block
constexpr int SN_WAVES = 4;                     // waves per block: wave w takes rows r0 + w, r0 + w + 4, ... of the band, two at a time
constexpr int SN_THREADS = SN_WAVES * 64;
constexpr int SN_MAXK = SGG_SPECTRAL_MAX_K;
constexpr double SN_EPS = 1e-12;

__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int sn_bands(int rows) { return (rows + SN_BAND - 1) / SN_BAND; }

// The sum of n doubles `stride` apart by the whole block, in an order n alone fixes: thread i adds elements i, i + 256, ..., then a
// tree over the threads.  (One thread walking the bands is a chain of dependent cache misses: 144 of them for a 4608-row layer.)
__device__ inline double block_sum_strided(const double* __restrict__ p, int n, size_t stride, double* red) {
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int b = tid; b < n; b += SN_THREADS) a += p[(size_t)b * stride];
    red[tid] = a;
    __syncthreads();
    for (int o = SN_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// item sanity against the launch's bounds (the table lives on the device: the host sized grid and workspace from max_rows / max_K)
__device__ inline bool sn_item_ok(const sgg_spectral_item& it, int max_rows, int max_K) {
    return it.w && it.u && it.v && it.sigma && it.inv_sigma && it.rows > 0 && it.K > 0 && it.rows <= max_rows && it.K <= max_K && it.K <= SN_MAXK;
}

// one row's elements of this lane: e = q * V + k  <->  column V * (lane + 64 q) + k; columns past K read 0
template <int V, int NQ>
__device__ __forceinline__ void row_load(const float* __restrict__ row, int K, int lane, float* a) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int col = V * (lane + 64 * q);
        if constexpr (V == 4) {
            u32x4 c = zero16();
            if (col < K) c = ld16(row + col);
            ET<float>::unpack(c, a + 4 * q);
        } else {
            a[q] = col < K ? row[col] : 0.f;
        }
    }
}
template <int V, int NQ>
__device__ __forceinline__ void row_store(float* __restrict__ row, int K, int lane, const float* a) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int col = V * (lane + 64 * q);
        if (col < K) {
            if constexpr (V == 4) st16(row + col, ET<float>::pack(a + 4 * q));
            else row[col] = a[q];
        }
    }
}

// V = 4 (16-byte loads) needs 16-byte aligned rows; NQ covers ceil(K / (64 V)) chunks per lane
#define SN_DISPATCH(K_, vec_, CALL)                                   \
    do {                                                              \
        if (vec_) {                                                   \
            const int nq_ = ((K_) + 255) / 256;                       \
            if (nq_ <= 1) CALL(4, 1); else if (nq_ <= 2) CALL(4, 2); else CALL(4, 4); \
        } else {                                                      \
            const int nq_ = ((K_) + 63) / 64;                         \
            if (nq_ <= 1) CALL(1, 1); else if (nq_ <= 2) CALL(1, 2); else if (nq_ <= 4) CALL(1, 4); \
            else if (nq_ <= 8) CALL(1, 8); else CALL(1, 16);          \
        }                                                             \
    } while (0)

__device__ inline bool sn_vec_ok(const void* p, int K) { return (K & 3) == 0 && ((uintptr_t)p & 15) == 0; }

// ---- sigma, launch 1: t = M u of the band's rows, and the band's share of Mt t and of |t|^2
template <int V, int NQ>
__device__ __forceinline__ void sigma_band(const float* __restrict__ M, const float* __restrict__ u, int K, int r0, int r1,
                                           double* __restrict__ t_out, double* __restrict__ part, double* lds_acc, double* lds_tt) {
    constexpr int E = V * NQ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float uf[E];
    double acc[E];
    row_load<V, NQ>(u, K, lane, uf);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;
    double tt = 0.0;
    for (int i = r0 + wave; i < r1; i += 2 * SN_WAVES) {
        const int i2 = i + SN_WAVES;
        const bool two = i2 < r1;                              // (wave-uniform)
        float a[E], b[E];
        row_load<V, NQ>(M + (size_t)i * K, K, lane, a);
        if (two) row_load<V, NQ>(M + (size_t)i2 * K, K, lane, b);
        else {
#pragma unroll
            for (int e = 0; e < E; ++e) b[e] = 0.f;
        }
        double pa = 0.0, pb = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) { pa += (double)a[e] * (double)uf[e]; pb += (double)b[e] * (double)uf[e]; }
        pa = wave_sum_d(pa);
        pb = wave_sum_d(pb);
        if (lane == 0) {
            t_out[i] = pa;
            if (two) t_out[i2] = pb;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) { acc[e] += pa * (double)a[e]; acc[e] += pb * (double)b[e]; }
        tt += pa * pa;
        tt += pb * pb;
    }
    // the four waves' sums, added in wave order
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int col = V * (lane + 64 * q) + k;
            if (col < K) lds_acc[wave * SN_MAXK + col] = acc[q * V + k];
        }
    if (lane == 0) lds_tt[wave] = tt;
    __syncthreads();
    for (int col = threadIdx.x; col < K; col += SN_THREADS) {
        double s = lds_acc[col];
#pragma unroll
        for (int w = 1; w < SN_WAVES; ++w) s += lds_acc[w * SN_MAXK + col];
        part[col] = s;
    }
    if (threadIdx.x == 0) {
        double s = lds_tt[0];
#pragma unroll
        for (int w = 1; w < SN_WAVES; ++w) s += lds_tt[w];
        part[K] = s;
    }
}

constexpr int SN_FOLD_COLS = 64;                // columns per fold block: its four waves split the bands of a column between them
constexpr int SN_MAX_CHUNKS = SN_MAXK / SN_FOLD_COLS;

// workspace of one item: [t: max_rows doubles][bands x (max_K + 1) doubles: the band's column sums, then its sum of t^2]
// [s: max_K doubles][the fold blocks' sums of s^2: SN_MAX_CHUNKS doubles]
__device__ __host__ inline size_t sigma_item_doubles(int max_rows, int max_K) {
    return (size_t)max_rows + (size_t)((max_rows + SN_BAND - 1) / SN_BAND) * (size_t)(max_K + 1) + (size_t)max_K + SN_MAX_CHUNKS;
}
__device__ inline size_t sigma_s_offset(int max_rows, int max_K) {
    return (size_t)max_rows + (size_t)((max_rows + SN_BAND - 1) / SN_BAND) * (size_t)(max_K + 1);
}

__global__ __launch_bounds__(SN_THREADS) void spectral_sigma_partial_kernel(const sgg_spectral_item* items, int max_rows, int max_K, double* ws) {
    __shared__ double lds_acc[SN_WAVES * SN_MAXK];
    __shared__ double lds_tt[SN_WAVES];
    const sgg_spectral_item it = items[blockIdx.y];
    if (!sn_item_ok(it, max_rows, max_K) || (int)blockIdx.x >= sn_bands(it.rows)) return;
    double* t = ws + (size_t)blockIdx.y * sigma_item_doubles(max_rows, max_K);
    double* part = t + max_rows + (size_t)blockIdx.x * (size_t)(max_K + 1);
    const int r0 = blockIdx.x * SN_BAND, r1 = min(r0 + SN_BAND, it.rows);
    const bool vec = sn_vec_ok(it.w, it.K) && sn_vec_ok(it.u, it.K);
#define CALL(V, NQ) sigma_band<V, NQ>(it.w, it.u, it.K, r0, r1, t, part, lds_acc, lds_tt)
    SN_DISPATCH(it.K, vec, CALL);
#undef CALL
}

// ---- sigma, launch 2 (a block per item and 64 columns): |t|, this block's share of v = t / |t|, and its columns of s = Mt t / |t| --
// the bands of a column split between the four waves, their sums added in wave order -- with the columns' sum of squares
__global__ __launch_bounds__(SN_THREADS) void spectral_sigma_fold_kernel(const sgg_spectral_item* items, int max_rows, int max_K, double* ws, int advance) {
    __shared__ double red[SN_THREADS];
    const sgg_spectral_item it = items[blockIdx.y];
    const int c0 = blockIdx.x * SN_FOLD_COLS;
    if (!sn_item_ok(it, max_rows, max_K) || c0 >= it.K) return;
    const int rows = it.rows, K = it.K, nb = sn_bands(rows), tid = threadIdx.x, nchunks = (K + SN_FOLD_COLS - 1) / SN_FOLD_COLS;
    double* t = ws + (size_t)blockIdx.y * sigma_item_doubles(max_rows, max_K);
    const double* part = t + max_rows;
    double* s_out = t + sigma_s_offset(max_rows, max_K);
    const size_t stride = (size_t)(max_K + 1);
    const double tt = block_sum_strided(part + K, nb, stride, red);
    const double nt = sqrt(fmax(tt, SN_EPS));
    for (int i = blockIdx.x * SN_THREADS + tid; i < rows; i += nchunks * SN_THREADS) it.v[i] = (float)(t[i] / nt);
    if (!advance) {                                                     // u stays: sigma = vt M u = |t|^2 / |t|
        if (blockIdx.x == 0 && tid == 0) {
            const double sig = fmax(tt / nt, SN_EPS);
            it.sigma[0] = (float)sig;
            it.inv_sigma[0] = (float)(1.0 / sig);
        }
        return;
    }
    const int lane = tid & 63, wave = tid >> 6, col = c0 + lane;
    double a = 0.0;
    if (col < K) {
#pragma unroll 4
        for (int b = wave; b < nb; b += SN_WAVES) a += part[(size_t)b * stride + col];
    }
    red[tid] = a;
    __syncthreads();
    double sq = 0.0;
    if (tid < 64) {
        double sj = red[tid];
#pragma unroll
        for (int w = 1; w < SN_WAVES; ++w) sj += red[w * 64 + tid];
        sj = sj / nt;
        if (col < K) s_out[col] = sj;                                   // (columns past K hold 0)
        sq = sj * sj;
    }
    __syncthreads();
    red[tid] = sq;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) s_out[max_K + blockIdx.x] = red[0];
}

// ---- sigma, launch 3 (one block per item, advance only): |s| from the fold blocks' sums in block order, u = s / |s|, sigma
__global__ __launch_bounds__(SN_THREADS) void spectral_sigma_finish_kernel(const sgg_spectral_item* items, int max_rows, int max_K, const double* ws) {
    const sgg_spectral_item it = items[blockIdx.x];
    if (!sn_item_ok(it, max_rows, max_K)) return;
    const int K = it.K, nchunks = (K + SN_FOLD_COLS - 1) / SN_FOLD_COLS;
    const double* s = ws + (size_t)blockIdx.x * sigma_item_doubles(max_rows, max_K) + sigma_s_offset(max_rows, max_K);
    double ss = 0.0;
    for (int c = 0; c < nchunks; ++c) ss += s[max_K + c];               // (at most 16; every thread: the same loads, the same sum)
    const double ns = sqrt(fmax(ss, SN_EPS));
    for (int j = threadIdx.x; j < K; j += SN_THREADS) it.u[j] = (float)(s[j] / ns);
    if (threadIdx.x == 0) {                                             // vt M u with the new u: |s|^2 / |s|
        const double sig = fmax(ss / ns, SN_EPS);
        it.sigma[0] = (float)sig;
        it.inv_sigma[0] = (float)(1.0 / sig);
    }
}

// ---- gradient, launch 1: the band's share of sum(dWbar o W)
template <int V, int NQ>
__device__ __forceinline__ void dot_band(const float* __restrict__ W, const float* __restrict__ G, int K, int r0, int r1, double* __restrict__ out,
                                         double* lds) {
    constexpr int E = V * NQ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int i = r0 + wave; i < r1; i += SN_WAVES) {
        float a[E], b[E];
        row_load<V, NQ>(W + (size_t)i * K, K, lane, a);
        row_load<V, NQ>(G + (size_t)i * K, K, lane, b);
#pragma unroll
        for (int e = 0; e < E; ++e) acc += (double)a[e] * (double)b[e];
    }
    acc = wave_sum_d(acc);
    if (lane == 0) lds[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = lds[0];
#pragma unroll
        for (int w = 1; w < SN_WAVES; ++w) s += lds[w];
        *out = s;
    }
}

__global__ __launch_bounds__(SN_THREADS) void spectral_grad_dot_kernel(const sgg_spectral_item* items, int max_rows, int max_K, double* ws) {
    __shared__ double lds[SN_WAVES];
    const sgg_spectral_item it = items[blockIdx.y];
    if (!sn_item_ok(it, max_rows, max_K) || !it.g || (int)blockIdx.x >= sn_bands(it.rows)) return;
    const int r0 = blockIdx.x * SN_BAND, r1 = min(r0 + SN_BAND, it.rows);
    double* out = ws + (size_t)blockIdx.y * (size_t)sn_bands(max_rows) + blockIdx.x;
    const bool vec = sn_vec_ok(it.w, it.K) && sn_vec_ok(it.g, it.K);
#define CALL(V, NQ) dot_band<V, NQ>(it.w, it.g, it.K, r0, r1, out, lds)
    SN_DISPATCH(it.K, vec, CALL);
#undef CALL
}

// ---- gradient, launch 2: lambda = (the bands' sums, in band order) / sigma, then dW = (dWbar - lambda v ut) / sigma in place
template <int V, int NQ>
__device__ __forceinline__ void grad_band(float* __restrict__ G, const float* __restrict__ u, const float* __restrict__ v, int K, int r0, int r1,
                                          double lam, double inv) {
    constexpr int E = V * NQ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float uf[E];
    row_load<V, NQ>(u, K, lane, uf);
    for (int i = r0 + wave; i < r1; i += SN_WAVES) {
        float a[E];
        row_load<V, NQ>(G + (size_t)i * K, K, lane, a);
        const double vi = (double)v[i];
#pragma unroll
        for (int e = 0; e < E; ++e) a[e] = (float)(((double)a[e] - lam * (vi * (double)uf[e])) * inv);
        row_store<V, NQ>(G + (size_t)i * K, K, lane, a);
    }
}

__global__ __launch_bounds__(SN_THREADS) void spectral_grad_apply_kernel(const sgg_spectral_item* items, int max_rows, int max_K, const double* ws) {
    __shared__ double red[SN_THREADS];
    const sgg_spectral_item it = items[blockIdx.y];
    const int nb = sn_bands(it.rows);
    if (!sn_item_ok(it, max_rows, max_K) || !it.g || (int)blockIdx.x >= nb) return;
    const double* part = ws + (size_t)blockIdx.y * (size_t)sn_bands(max_rows);
    const double dot = block_sum_strided(part, nb, 1, red);
    const double inv = (double)it.inv_sigma[0];
    const double lam = dot * inv;
    const int r0 = blockIdx.x * SN_BAND, r1 = min(r0 + SN_BAND, it.rows);
    const bool vec = sn_vec_ok(it.g, it.K) && sn_vec_ok(it.u, it.K);
#define CALL(V, NQ) grad_band<V, NQ>(it.g, it.u, it.v, it.K, r0, r1, lam, inv)
    SN_DISPATCH(it.K, vec, CALL);
#undef CALL
}

bool sn_args_ok(const void* items, int n_items, int max_rows, int max_K) {
    return items && n_items > 0 && n_items <= 65535 && max_rows > 0 && max_K > 0 && max_K <= SN_MAXK && (max_rows + SN_BAND - 1) / SN_BAND <= 65535 * 1024;
}

}  // namespace

extern "C" {

size_t sgg_spectral_sigma_workspace(int n_items, int max_rows, int max_K) {
    if (n_items <= 0 || max_rows <= 0 || max_K <= 0 || max_K > SN_MAXK) return 0;
    return (size_t)n_items * sigma_item_doubles(max_rows, max_K) * sizeof(double);
}

int sgg_spectral_sigma(const sgg_spectral_item* items_dev, int n_items, int max_rows, int max_K, int advance, void* ws, size_t ws_bytes, void* stream) {
    if (!sn_args_ok(items_dev, n_items, max_rows, max_K)) return SGG_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < sgg_spectral_sigma_workspace(n_items, max_rows, max_K)) return SGG_EWORKSPACE;
    const unsigned nb = (unsigned)((max_rows + SN_BAND - 1) / SN_BAND);
    hipLaunchKernelGGL(spectral_sigma_partial_kernel, dim3(nb, (unsigned)n_items), dim3(SN_THREADS), 0, (hipStream_t)stream, items_dev, max_rows, max_K, (double*)ws);
    hipLaunchKernelGGL(spectral_sigma_fold_kernel, dim3((unsigned)((max_K + SN_FOLD_COLS - 1) / SN_FOLD_COLS), (unsigned)n_items), dim3(SN_THREADS), 0,
                       (hipStream_t)stream, items_dev, max_rows, max_K, (double*)ws, advance ? 1 : 0);
    if (advance)
        hipLaunchKernelGGL(spectral_sigma_finish_kernel, dim3((unsigned)n_items), dim3(SN_THREADS), 0, (hipStream_t)stream, items_dev, max_rows, max_K,
                           (const double*)ws);
    return sgg_check_launch();
}

size_t sgg_spectral_grad_workspace(int n_items, int max_rows) {
    if (n_items <= 0 || max_rows <= 0) return 0;
    return (size_t)n_items * (size_t)((max_rows + SN_BAND - 1) / SN_BAND) * sizeof(double);
}

int sgg_spectral_grad(const sgg_spectral_item* items_dev, int n_items, int max_rows, int max_K, void* ws, size_t ws_bytes, void* stream) {
    if (!sn_args_ok(items_dev, n_items, max_rows, max_K)) return SGG_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < sgg_spectral_grad_workspace(n_items, max_rows)) return SGG_EWORKSPACE;
    const dim3 grid((unsigned)((max_rows + SN_BAND - 1) / SN_BAND), (unsigned)n_items);
    hipLaunchKernelGGL(spectral_grad_dot_kernel, grid, dim3(SN_THREADS), 0, (hipStream_t)stream, items_dev, max_rows, max_K, (double*)ws);
    hipLaunchKernelGGL(spectral_grad_apply_kernel, grid, dim3(SN_THREADS), 0, (hipStream_t)stream, items_dev, max_rows, max_K, (const double*)ws);
    return sgg_check_launch();
}

}  // extern "C"
