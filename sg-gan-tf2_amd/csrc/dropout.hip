// dropout.hip -- training-mode dropout of the U-Net decoder: y = m * x * scale IN PLACE, the mask m regenerated from
// counters wherever it is needed -- the backward of y = m * scale * x is dx = m * scale * dy, the SAME launch on the gradient.
//
// x is (n_samples, elems_per_sample); element i of sample n belongs to vector e = i / 8, lane j = i % 8:
//
//   r = Philox4x32-10(counter (t_lo, t_hi, g, e), key (seed, 1 + stream_id))      t = *iterations, READ ON THE DEVICE when the
//   d = (r[j >> 1] >> (16 * (j & 1))) & 0xFFFF                                    launch runs; g = (uint32)(sample_offset + n)
//   y = d >= threshold ? (storage type)(x * scale) : +0                           scale = 65536.f / (65536 - threshold), f32
//
// The draw depends on the element index alone, never on the dtype or the launch shape: f32 and bf16 drop the same elements.  Key
// word 1 is never 0, the key of sgg_diffaug_draw's streams.  threshold 0 keeps everything at scale 1: no launch at all.
//
// Shape: a pure streaming kernel, one Philox call per 8 elements = one 16-byte bf16 vector or two 16-byte f32 vectors, each loaded
// and stored whole, once.  No LDS, no atomics, no workspace; nothing launch-shaped depends on data.  Blocks of DO_THREADS = 256;
// a block takes chunks of DO_CHUNK = DO_THREADS * DO_VPT = 1024 vectors of ONE sample (blockIdx.y), thread t the vectors
// t, t + 256, ... of the chunk, so a wave's 64 loads are one contiguous 1 KB (bf16), and all DO_VPT loads of a thread are issued
// before the first is used (4 x 16 bytes in flight per thread, 8 resident blocks per CU: 128 KB per CU).  The grid is capped at
// about DO_GRID_BLOCKS = 2048 blocks (256 CUs x 8 resident blocks: one wave of blocks fills the chip) -- min(chunks per sample,
// 2048 / n_samples) in x, the samples in y -- and a block strides over its sample's remaining chunks by gridDim.x.
// Arithmetic per vector: ten rounds of two 32 x 32 -> 64-bit products.  Loads and stores keep the default cache policy: the tensor
// was just written by the transposed conv and is read next by the instance norm.
#include "common.h"

namespace {

constexpr int DO_THREADS = 256;
constexpr int DO_VPT = 4;                            // vectors of 8 elements per thread and chunk
constexpr int DO_CHUNK = DO_THREADS * DO_VPT;        // vectors per block and grid stride
constexpr int DO_GRID_BLOCKS = 2048;                 // the grid's target size
constexpr int64_t DO_MAX_ELEMS = 1ll << 35;          // per sample: the vector index is Philox counter word 3

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants)
__device__ inline u32x4 do_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (u32x4){c0, c1, c2, c3};
}

// the 8 elements of one vector: kept ones times scale (one f32 product, one rounding to T), dropped ones +0
template <typename T> __device__ inline void do_apply(T* p, const u32x4* v, const u32x4& r, uint32_t threshold, float scale) {
    float f[8];
    if constexpr (std::is_same<T, float>::value) {
        ET<float>::unpack(v[0], f);
        ET<float>::unpack(v[1], f + 4);
    } else {
        ET<bf16>::unpack(v[0], f);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t d = (r[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        f[j] = d >= threshold ? f[j] * scale : 0.f;
    }
    if constexpr (std::is_same<T, float>::value) {
        st16(p, ET<float>::pack(f));
        st16(p + 4, ET<float>::pack(f + 4));
    } else {
        st16(p, ET<bf16>::pack(f));
    }
}

template <typename T>
__global__ __launch_bounds__(DO_THREADS) void dropout_kernel(T* __restrict__ x, int64_t vecs, int64_t chunks, uint32_t threshold,
                                                            float scale, const int64_t* __restrict__ iterations, uint32_t seed,
                                                            uint32_t g0, uint32_t key1) {
    constexpr int L = std::is_same<T, float>::value ? 2 : 1;        // 16-byte loads per vector
    const uint64_t t = (uint64_t)iterations[0];
    const uint32_t t_lo = (uint32_t)t, t_hi = (uint32_t)(t >> 32), g = g0 + blockIdx.y;
    T* row = x + (size_t)blockIdx.y * (size_t)vecs * 8;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t e0 = c * DO_CHUNK + threadIdx.x;
        u32x4 v[DO_VPT][L];
#pragma unroll
        for (int i = 0; i < DO_VPT; ++i) {
            const int64_t e = e0 + i * DO_THREADS;
            if (e < vecs) {
#pragma unroll
                for (int l = 0; l < L; ++l) v[i][l] = ld16(row + e * 8 + l * 4);
            }
        }
#pragma unroll
        for (int i = 0; i < DO_VPT; ++i) {
            const int64_t e = e0 + i * DO_THREADS;
            if (e < vecs) do_apply<T>(row + e * 8, v[i], do_philox(t_lo, t_hi, g, (uint32_t)e, seed, key1), threshold, scale);
        }
    }
}

}  // namespace

extern "C" int sgg_dropout(void* x, int64_t n_samples, int64_t elems_per_sample, int threshold, const int64_t* iterations,
                           uint32_t seed, int64_t sample_offset, int stream_id, int dtype, void* stream) {
    if (!x || !iterations || n_samples < 0 || elems_per_sample < 0 || (elems_per_sample & 7) || ((uintptr_t)x & 15)) return SGG_EINVAL;
    if (threshold < 0 || threshold > 65535 || stream_id < 0 || stream_id >= (1 << 28) || sample_offset < 0) return SGG_EINVAL;
    if (dtype != SGG_F32 && dtype != SGG_BF16) return SGG_EINVAL;
    if (elems_per_sample > DO_MAX_ELEMS || n_samples > 65535) return SGG_EUNSUPPORTED;      // (gridDim.y holds the samples)
    if (n_samples == 0 || elems_per_sample == 0 || threshold == 0) return SGG_OK;
    const int64_t vecs = elems_per_sample / 8, chunks = (vecs + DO_CHUNK - 1) / DO_CHUNK;
    const int64_t cap = DO_GRID_BLOCKS / n_samples > 0 ? DO_GRID_BLOCKS / n_samples : 1;
    const dim3 grid((unsigned)(chunks < cap ? chunks : cap), (unsigned)n_samples), block(DO_THREADS);
    const float scale = 65536.f / (float)(65536 - threshold);
    const uint32_t g0 = (uint32_t)sample_offset, key1 = 1u + (uint32_t)stream_id;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SGG_F32)
        hipLaunchKernelGGL(dropout_kernel<float>, grid, block, 0, s, (float*)x, vecs, chunks, (uint32_t)threshold, scale, iterations, seed, g0, key1);
    else
        hipLaunchKernelGGL(dropout_kernel<bf16>, grid, block, 0, s, (bf16*)x, vecs, chunks, (uint32_t)threshold, scale, iterations, seed, g0, key1);
    return sgg_check_launch();
}
