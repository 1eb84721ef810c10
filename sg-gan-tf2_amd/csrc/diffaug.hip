// diffaug.hip -- differentiable augmentation of the discriminators' input: per image row of a stacked batch one
// parameter row of 8 floats [b, s, c, y0, x0, ch, cw, 0]; with C real channels of Cpad = 8 per pixel, for pixel p = (y, x):
//
//   x1 = x + b                                         brightness
//   m  = (x1[p,0] + ... + x1[p,C-1]) / C               f32, channel order
//   x2 = x1 + (s - 1) * (x1 - m)                       saturation
//   M  = b + S / (C*H*W),  S = sum of x over the image's real channels
//   x3 = x2 + (c - 1) * (x2 - M)                       contrast (mean(x2) == mean(x1): one reduction over the INPUT)
//   y  = 0 if y0 <= y < y0+ch and x0 <= x < x0+cw, else x3          cutout: a select
//
// and the adjoint, g the gradient w.r.t. y:  g3 = 0 inside the rectangle, else g;  Gs = sum of g3;  g2 = c * g3;
//   dx = g2 + (s - 1) * (g2 - mean_k g2[p,:]) + (1 - c) * Gs / (C*H*W)   (+ addend[p,k])
// Padded channels of y and dx are written as 0.  Written as x + (k-1)(x - mean), the neutral row [0,1,1,0,0,0,0,0] gives back
// the input's values in both dtypes.
//
// Pure bandwidth kernels: one pixel is one 16-byte (bf16) or 32-byte (f32) vector, loaded and stored whole.  The image sum is
// DA_CHUNK-pixel partials in double (per thread in pixel order, a fixed shuffle tree per wave, the four waves in order); every
// apply block then folds its image's partials again, in double, in the same order (lane i takes partials i, i + 64, ..., then
// the same tree).  No atomics, no allocation, no host sync: two launches forward, two backward, the same bits every run.
//
// The parameter rows are drawn on the device (diffaug_draw_kernel) from Philox4x32-10 [Random123's constants]: key (seed, 0),
// counter (t_lo, t_hi, g, 4 * stream_id + j) with t the 64-bit step counter READ FROM DEVICE MEMORY when the launch runs, g the
// global sample index and j the draw block -- nothing varies on the host, so the launch can be captured and replayed.
#include "common.h"
#include <math.h>

namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_CHUNK = 2048;                      // pixels per block (8 per thread), of the sum and of the apply pass
constexpr int DA_WAVES = DA_THREADS / SGG_WAVE;
constexpr int64_t DA_MAX_HW = 1 << 26;

__device__ inline double da_wave_sum(double v) {    // a fixed tree: the same lanes meet in the same order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T> __device__ inline void da_load(const T* p, float* f) {       // one pixel: SGG_CPAD channels
    if constexpr (std::is_same<T, float>::value) {
        ET<float>::unpack(ld16(p), f);
        ET<float>::unpack(ld16(p + 4), f + 4);
    } else {
        ET<bf16>::unpack(ld16(p), f);
    }
}
template <typename T> __device__ inline void da_store(T* p, const float* f) {
    if constexpr (std::is_same<T, float>::value) {
        st16(p, ET<float>::pack(f));
        st16(p + 4, ET<float>::pack(f + 4));
    } else {
        st16(p, ET<bf16>::pack(f));
    }
}

struct DaRect { int y0, x0, y1, x1; };              // the cutout, [y0, y1) x [x0, x1); empty when ch or cw is 0
__device__ inline DaRect da_rect(const float* row) {
    DaRect r;
    r.y0 = (int)row[3]; r.x0 = (int)row[4];
    r.y1 = r.y0 + (int)row[5]; r.x1 = r.x0 + (int)row[6];
    return r;
}
__device__ inline bool da_inside(const DaRect& r, uint32_t p, const FastDiv& wdiv) {
    const int y = (int)fdiv(p, wdiv), x = (int)p - y * (int)wdiv.d;
    return y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1;
}

// ws[row * chunks + chunk] = sum over the chunk's pixels and real channels (MASK: outside the row's rectangle), in double
template <typename T, bool MASK>
__global__ __launch_bounds__(DA_THREADS) void diffaug_sum_kernel(const T* __restrict__ x, const float* __restrict__ params, int HW,
                                                                const FastDiv wdiv, int C, int chunks, double* __restrict__ ws) {
    __shared__ double red[DA_WAVES];
    const int row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
    const T* img = x + (size_t)row * HW * SGG_CPAD;
    DaRect rc = {0, 0, 0, 0};
    if (MASK) rc = da_rect(params + (size_t)row * 8);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < DA_CHUNK / DA_THREADS; ++i) {
        const int p = chunk * DA_CHUNK + i * DA_THREADS + (int)threadIdx.x;
        if (p < HW) {
            float f[SGG_CPAD];
            da_load(img + (size_t)p * SGG_CPAD, f);
            if (!(MASK && da_inside(rc, (uint32_t)p, wdiv))) {
#pragma unroll
                for (int k = 0; k < SGG_CPAD; ++k)
                    if (k < C) acc += (double)f[k];
            }
        }
    }
    acc = da_wave_sum(acc);
    if ((threadIdx.x & (SGG_WAVE - 1)) == 0) red[threadIdx.x / SGG_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
#pragma unroll
        for (int w = 1; w < DA_WAVES; ++w) s += red[w];
        ws[blockIdx.x] = s;
    }
}

// the image's sum from its partials: every wave of every apply block, the same order
__device__ inline double da_fold(const double* __restrict__ part, int chunks) {
    double s = 0.0;
    for (int i = (int)(threadIdx.x & (SGG_WAVE - 1)); i < chunks; i += SGG_WAVE) s += part[i];
    return da_wave_sum(s);
}

template <typename T>
__global__ __launch_bounds__(DA_THREADS) void diffaug_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ params,
                                                                const double* __restrict__ ws, int HW, const FastDiv wdiv, int C, int chunks) {
    const int row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
    const float* pr = params + (size_t)row * 8;
    const float b = pr[0], sm1 = pr[1] - 1.f, cm1 = pr[2] - 1.f;
    const DaRect rc = da_rect(pr);
    const double S = da_fold(ws + (size_t)row * chunks, chunks);
    const float M = (float)((double)b + S / ((double)C * (double)HW));
    const float fC = (float)C;
    const T* img = x + (size_t)row * HW * SGG_CPAD;
    T* out = y + (size_t)row * HW * SGG_CPAD;
#pragma unroll
    for (int i = 0; i < DA_CHUNK / DA_THREADS; ++i) {
        const int p = chunk * DA_CHUNK + i * DA_THREADS + (int)threadIdx.x;
        if (p >= HW) continue;
        float f[SGG_CPAD];
        da_load(img + (size_t)p * SGG_CPAD, f);
        const bool cut = da_inside(rc, (uint32_t)p, wdiv);
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < SGG_CPAD; ++k)
            if (k < C) {
                f[k] = f[k] + b;
                m = k == 0 ? f[0] : m + f[k];
            }
        m = m / fC;
#pragma unroll
        for (int k = 0; k < SGG_CPAD; ++k) {
            float v = 0.f;
            if (k < C && !cut) {
                const float x2 = f[k] + sm1 * (f[k] - m);
                v = x2 + cm1 * (x2 - M);
            }
            f[k] = v;
        }
        da_store(out + (size_t)p * SGG_CPAD, f);
    }
}

template <typename T>
__global__ __launch_bounds__(DA_THREADS) void diffaug_bwd_kernel(const T* __restrict__ dy, const float* __restrict__ params,
                                                                const T* __restrict__ addend, T* __restrict__ dx,
                                                                const double* __restrict__ ws, int HW, const FastDiv wdiv, int C, int chunks) {
    const int row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
    const float* pr = params + (size_t)row * 8;
    const float sm1 = pr[1] - 1.f, c = pr[2];
    const DaRect rc = da_rect(pr);
    const double Gs = da_fold(ws + (size_t)row * chunks, chunks);
    const float G = (float)((1.0 - (double)c) * Gs / ((double)C * (double)HW));
    const float fC = (float)C;
    const size_t base = (size_t)row * HW * SGG_CPAD;
#pragma unroll
    for (int i = 0; i < DA_CHUNK / DA_THREADS; ++i) {
        const int p = chunk * DA_CHUNK + i * DA_THREADS + (int)threadIdx.x;
        if (p >= HW) continue;
        const size_t off = base + (size_t)p * SGG_CPAD;
        float g[SGG_CPAD], a[SGG_CPAD];
        da_load(dy + off, g);
        if (addend) da_load(addend + off, a);
        const bool cut = da_inside(rc, (uint32_t)p, wdiv);
        float mk = 0.f;
#pragma unroll
        for (int k = 0; k < SGG_CPAD; ++k)
            if (k < C) {
                g[k] = c * (cut ? 0.f : g[k]);
                mk = k == 0 ? g[0] : mk + g[k];
            }
        mk = mk / fC;
#pragma unroll
        for (int k = 0; k < SGG_CPAD; ++k) {
            float v = 0.f;
            if (k < C) {
                v = g[k] + sm1 * (g[k] - mk);
                v = v + G;
                if (addend) v = v + a[k];
            }
            g[k] = v;
        }
        da_store(dx + off, g);
    }
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants)
struct DaU4 { uint32_t v[4]; };
__device__ inline DaU4 philox4x32_10(DaU4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.v[0]), lo0 = 0xD2511F53u * c.v[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.v[2]), lo1 = 0xCD9E8D57u * c.v[2];
        DaU4 n;
        n.v[0] = hi1 ^ c.v[1] ^ k0; n.v[1] = lo1; n.v[2] = hi0 ^ c.v[3] ^ k1; n.v[3] = lo0;
        c = n;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ inline float da_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }     // 24 bits: exact

__global__ void diffaug_draw_kernel(float* __restrict__ params, int rows, const int64_t* __restrict__ iterations, uint32_t seed,
                                    uint32_t g0, uint32_t w3, int H, int W, int bits, float B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint64_t t = (uint64_t)iterations[0];
    DaU4 ctr;
    ctr.v[0] = (uint32_t)t; ctr.v[1] = (uint32_t)(t >> 32); ctr.v[2] = g0 + (uint32_t)i;
    float b = 0.f, s = 1.f, c = 1.f, y0 = 0.f, x0 = 0.f, ch = 0.f, cw = 0.f;
    if (bits & SGG_DIFFAUG_COLOR) {
        ctr.v[3] = w3;
        const DaU4 r = philox4x32_10(ctr, seed, 0u);
        b = (da_uniform(r.v[0]) - 0.5f) * B;
        s = 2.f * da_uniform(r.v[1]);
        c = da_uniform(r.v[2]) + 0.5f;
    }
    if (bits & SGG_DIFFAUG_CUTOUT) {
        ctr.v[3] = w3 + 1u;
        const DaU4 r = philox4x32_10(ctr, seed, 0u);
        const int h = H / 2, w = W / 2;
        y0 = floorf(da_uniform(r.v[0]) * (float)(H + 1 - h % 2)) - (float)(h / 2);
        x0 = floorf(da_uniform(r.v[1]) * (float)(W + 1 - w % 2)) - (float)(w / 2);
        ch = (float)h; cw = (float)w;
    }
    float* o = params + (size_t)i * 8;
    const f32x4 lo = {b, s, c, y0}, hi = {x0, ch, cw, 0.f};
    *reinterpret_cast<f32x4*>(o) = lo;
    *reinterpret_cast<f32x4*>(o + 4) = hi;
}

int da_chunks(int H, int W) { return (int)(((int64_t)H * W + DA_CHUNK - 1) / DA_CHUNK); }

// the checks forward and backward share; 0 chunks: not launchable
int da_check(const void* a, const void* b, const void* params, int rows, int H, int W, int C_real, int Cpad, int dtype, const void* ws,
             size_t ws_bytes, int& chunks) {
    if (!a || !b || !params || !ws || rows <= 0 || H <= 0 || W <= 0 || C_real <= 0 || C_real > Cpad) return SGG_EINVAL;
    if (dtype != SGG_F32 && dtype != SGG_BF16) return SGG_EINVAL;
    if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)params & 15) || ((uintptr_t)ws & 7)) return SGG_EINVAL;
    if (Cpad != SGG_CPAD || (int64_t)H * W > DA_MAX_HW) return SGG_EUNSUPPORTED;
    chunks = da_chunks(H, W);
    if ((int64_t)chunks * rows * DA_THREADS > 0xffffffffll) return SGG_EUNSUPPORTED;     // HIP launches at most 2^32 - 1 threads
    if (ws_bytes < sgg_diffaug_workspace(rows, H, W)) return SGG_EWORKSPACE;
    return SGG_OK;
}

}  // namespace

extern "C" size_t sgg_diffaug_workspace(int rows, int H, int W) {
    if (rows <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > DA_MAX_HW) return 0;
    return (size_t)rows * (size_t)da_chunks(H, W) * sizeof(double);
}

extern "C" int sgg_diffaug_draw(float* params, int rows, const int64_t* iterations, uint32_t seed, int64_t sample_offset, int stream_id,
                                int H, int W, int policy_bits, float brightness, void* stream) {
    if (!params || !iterations || rows <= 0 || H <= 0 || W <= 0 || stream_id < 0 || stream_id >= (1 << 28) || sample_offset < 0)
        return SGG_EINVAL;
    if (((uintptr_t)params & 15) || (policy_bits & ~(SGG_DIFFAUG_COLOR | SGG_DIFFAUG_CUTOUT))) return SGG_EINVAL;
    const int threads = 64;
    hipLaunchKernelGGL(diffaug_draw_kernel, dim3((rows + threads - 1) / threads), dim3(threads), 0, (hipStream_t)stream, params, rows,
                       iterations, seed, (uint32_t)sample_offset, 4u * (uint32_t)stream_id, H, W, policy_bits, brightness);
    return sgg_check_launch();
}

extern "C" int sgg_diffaug_fwd(const void* x, void* y, const float* params, int rows, int H, int W, int C_real, int Cpad, int dtype,
                               void* ws, size_t ws_bytes, void* stream) {
    int chunks = 0;
    const int rc = da_check(x, y, params, rows, H, W, C_real, Cpad, dtype, ws, ws_bytes, chunks);
    if (rc) return rc;
    if (x == y) return SGG_EINVAL;                                                       // out of place: x stays as it is
    const int HW = H * W;
    const FastDiv wdiv = make_fastdiv((uint32_t)W);
    const dim3 grid(chunks * rows), block(DA_THREADS);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    if (dtype == SGG_F32) {
        hipLaunchKernelGGL((diffaug_sum_kernel<float, false>), grid, block, 0, s, (const float*)x, params, HW, wdiv, C_real, chunks, part);
        hipLaunchKernelGGL(diffaug_fwd_kernel<float>, grid, block, 0, s, (const float*)x, (float*)y, params, (const double*)part, HW, wdiv,
                           C_real, chunks);
    } else {
        hipLaunchKernelGGL((diffaug_sum_kernel<bf16, false>), grid, block, 0, s, (const bf16*)x, params, HW, wdiv, C_real, chunks, part);
        hipLaunchKernelGGL(diffaug_fwd_kernel<bf16>, grid, block, 0, s, (const bf16*)x, (bf16*)y, params, (const double*)part, HW, wdiv,
                           C_real, chunks);
    }
    return sgg_check_launch();
}

extern "C" int sgg_diffaug_bwd(const void* dy, const float* params, const void* addend, void* dx, int rows, int H, int W, int C_real,
                               int Cpad, int dtype, void* ws, size_t ws_bytes, void* stream) {
    int chunks = 0;
    const int rc = da_check(dy, dx, params, rows, H, W, C_real, Cpad, dtype, ws, ws_bytes, chunks);
    if (rc) return rc;
    if (addend && ((uintptr_t)addend & 15)) return SGG_EINVAL;
    const int HW = H * W;
    const FastDiv wdiv = make_fastdiv((uint32_t)W);
    const dim3 grid(chunks * rows), block(DA_THREADS);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    if (dtype == SGG_F32) {
        hipLaunchKernelGGL((diffaug_sum_kernel<float, true>), grid, block, 0, s, (const float*)dy, params, HW, wdiv, C_real, chunks, part);
        hipLaunchKernelGGL(diffaug_bwd_kernel<float>, grid, block, 0, s, (const float*)dy, params, (const float*)addend, (float*)dx,
                           (const double*)part, HW, wdiv, C_real, chunks);
    } else {
        hipLaunchKernelGGL((diffaug_sum_kernel<bf16, true>), grid, block, 0, s, (const bf16*)dy, params, HW, wdiv, C_real, chunks, part);
        hipLaunchKernelGGL(diffaug_bwd_kernel<bf16>, grid, block, 0, s, (const bf16*)dy, params, (const bf16*)addend, (bf16*)dx,
                           (const double*)part, HW, wdiv, C_real, chunks);
    }
    return sgg_check_launch();
}
