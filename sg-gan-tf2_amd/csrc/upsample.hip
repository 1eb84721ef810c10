// upsample.hip -- the fixed 2x resampling U in front of the resize-convolution layers of generator_resnet, and its
// adjoint.  NHWC with padded channels: U takes x (N,H,W,Cp) to y (N,2H,2W,Cp), U^T takes dy (N,2H,2W,Cp) to dx (N,H,W,Cp).
//
//   nearest:   y[n,p,q,c] = x[n, p>>1, q>>1, c]                                              -- a copy: output bits are input bits
//   bilinear:  half-pixel centres (tf.image.resize, Keras UpSampling2D(interpolation="bilinear"), torch align_corners=False):
//              per axis of length n   y[2i] = 0.25 x[max(i-1,0)] + 0.75 x[i],   y[2i+1] = 0.75 x[i] + 0.25 x[min(i+1,n-1)];
//              in 2-D the tensor product: weights 9/16, 3/16, 3/16, 1/16, clamped taps adding up at the borders
//   adjoint:   nearest: the sum of the 2x2 block.  bilinear: per axis dx[i] = sum_{k=-1..2} w_k dy[clamp(2i+k, 0, 2n-1)] with
//              w = (0.25, 0.75, 0.75, 0.25) -- the clamp IS the border term (dx[0] += 0.25 dy[0], dx[n-1] += 0.25 dy[2n-1]); 16 taps in 2-D
//
// Arithmetic: f32.  A result is the sum of its taps in ROW-MAJOR ORDER OVER THE SOURCE OFFSETS (a clamped tap keeps its place and
// its weight): acc = w_0 * v_0, then acc = acc + w_t * v_t for t = 1.., every product and every sum rounded to f32 (never
// contracted), the weight w_t = (row weight) * (column weight) an exact multiple of 1/16; then ONE rounding to the storage type
// (bf16: to nearest even).  The nearest adjoint has no products: ((d00 + d01) + d10) + d11.  Both directions are gathers -- a
// thread computes whole results -- so there are no atomics and no workspace, nothing launch-shaped depends on data, and runs agree
// bit for bit; f32 and bf16 differ by the last rounding only.
//
// Shape: pure streaming kernels (as dropout.hip).  The work item of BOTH directions is one 8-channel vector of the LOW-resolution
// tensor -- 16 bytes of bf16 (one load / store) or 32 bytes of f32 (two) -- index e = ((n * H + i) * W + j) * (Cp / 8) + cv: the
// forward loads the 3x3 neighbourhood of (i, j) (nearest: the one vector) and stores the four outputs (2i + a, 2j + b); the
// adjoint loads the 4x4 (nearest: 2x2) window of dy and stores dx[e].  Every load and store is whole, all loads of an item are
// issued before the first is used, addresses are 64-bit.  Blocks of UP_THREADS = 256 take chunks of UP_CHUNK = 256 consecutive
// items, one per thread, so a wave's 64 items are the channel vectors of adjacent pixels of one row: its loads are contiguous
// runs, and the neighbour re-reads of bilinear (3x in the forward's rows, 2x in the adjoint's) hit the lines the same or the
// neighbouring wave just fetched -- from HBM each byte of x moves once and each byte of y once.  The grid is capped at
// UP_GRID_BLOCKS = 1024 blocks (256 CUs x 4 resident blocks = 16 waves per CU; an item has 1 to 32 sixteen-byte loads in flight, so
// even the nearest forward keeps 16 KB of loads per CU outstanding beside its 64 KB of stores -- reads are a fifth of its traffic)
// with a stride loop over the remaining chunks.  20-38 VGPRs (nearest), 64-86 (bilinear), no spills, no scratch, no LDS.  Default
// cache policy: the forward's output is read next by the conv, the adjoint's by the norm backward in front of it.
#include "common.h"

namespace {

constexpr int UP_THREADS = 256;
constexpr int UP_CHUNK = UP_THREADS;                 // low-resolution vectors per block and grid stride: one per thread
constexpr int UP_GRID_BLOCKS = 1024;                 // the grid's cap
constexpr int64_t UP_MAX_VECS = 0x7fffffffll;        // the item index and its decomposition are 32-bit (FastDiv: n < 2^31)

template <typename T> struct Vec8 {                  // 8 channels of one pixel
    static constexpr int L = std::is_same<T, float>::value ? 2 : 1;       // 16-byte loads
    u32x4 c[L];
    __device__ inline void load(const T* p) {
#pragma unroll
        for (int l = 0; l < L; ++l) c[l] = ld16(p + l * ET<T>::VEC);
    }
    __device__ inline void store(T* p) const {
#pragma unroll
        for (int l = 0; l < L; ++l) st16(p + l * ET<T>::VEC, c[l]);
    }
    __device__ inline void unpack(float* f) const {
#pragma unroll
        for (int l = 0; l < L; ++l) ET<T>::unpack(c[l], f + l * ET<T>::VEC);
    }
    __device__ inline void pack(const float* f) {
#pragma unroll
        for (int l = 0; l < L; ++l) c[l] = ET<T>::pack(f + l * ET<T>::VEC);
    }
};

// acc (+)= w * v over the 8 channels: product and sum each rounded to f32
template <bool FIRST> __device__ inline void up_tap(float* acc, const float* v, float w) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float p = __fmul_rn(w, v[k]);
        acc[k] = FIRST ? p : __fadd_rn(acc[k], p);
    }
}

__device__ inline int up_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// x (N,H,W,CV*8) -> y (N,2H,2W,CV*8)
template <typename T, int MODE>
__global__ __launch_bounds__(UP_THREADS) void upsample2x_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint32_t total, int H, int W,
                                                                   int CV, FastDiv dCV, FastDiv dW, FastDiv dH) {
    const uint32_t chunks = (total + UP_CHUNK - 1) / UP_CHUNK;
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t e = c * UP_CHUNK + threadIdx.x;
        if (e >= total) continue;
        const uint32_t pix = fdiv(e, dCV), cv = e - pix * CV;
        const uint32_t row = fdiv(pix, dW), j = pix - row * W;
        const uint32_t n = fdiv(row, dH), i = row - n * H;
        const size_t ystride = (size_t)2 * W * CV * 8;                                    // one output row, in elements
        T* yp = y + (((size_t)n * 2 * H + 2 * i) * 2 * W + 2 * j) * CV * 8 + (size_t)cv * 8;   // output (2i, 2j)
        if constexpr (MODE == SGG_UPSAMPLE_NEAREST) {
            Vec8<T> v;
            v.load(x + (size_t)e * 8);
            v.store(yp); v.store(yp + (size_t)CV * 8);
            v.store(yp + ystride); v.store(yp + ystride + (size_t)CV * 8);
        } else {
            const int ri[3] = {up_clamp((int)i - 1, H - 1), (int)i, up_clamp((int)i + 1, H - 1)};
            const int ci[3] = {up_clamp((int)j - 1, W - 1), (int)j, up_clamp((int)j + 1, W - 1)};
            Vec8<T> v[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[r][q].load(x + ((((size_t)n * H + ri[r]) * W + ci[q]) * CV + cv) * 8);
            float f[3][3][8];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[r][q].unpack(f[r][q]);
            // output (2i + a, 2j + b) takes source rows a, a + 1 and columns b, b + 1 of the 3x3 window; the nearer one weighs 0.75
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float wr0 = a ? 0.75f : 0.25f, wr1 = a ? 0.25f : 0.75f, wc0 = b ? 0.75f : 0.25f, wc1 = b ? 0.25f : 0.75f;
                    float acc[8];
                    up_tap<true>(acc, f[a][b], wr0 * wc0);
                    up_tap<false>(acc, f[a][b + 1], wr0 * wc1);
                    up_tap<false>(acc, f[a + 1][b], wr1 * wc0);
                    up_tap<false>(acc, f[a + 1][b + 1], wr1 * wc1);
                    Vec8<T> o;
                    o.pack(acc);
                    o.store(yp + a * ystride + (size_t)b * CV * 8);
                }
        }
    }
}

// dy (N,2H,2W,CV*8) -> dx (N,H,W,CV*8)
template <typename T, int MODE>
__global__ __launch_bounds__(UP_THREADS) void upsample2x_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, uint32_t total, int H, int W,
                                                                   int CV, FastDiv dCV, FastDiv dW, FastDiv dH) {
    constexpr int TAPS = MODE == SGG_UPSAMPLE_NEAREST ? 2 : 4;           // per axis; source offsets k0 .. k0 + TAPS - 1 from 2i
    constexpr int K0 = MODE == SGG_UPSAMPLE_NEAREST ? 0 : -1;
    const uint32_t chunks = (total + UP_CHUNK - 1) / UP_CHUNK;
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t e = c * UP_CHUNK + threadIdx.x;
        if (e >= total) continue;
        const uint32_t pix = fdiv(e, dCV), cv = e - pix * CV;
        const uint32_t row = fdiv(pix, dW), j = pix - row * W;
        const uint32_t n = fdiv(row, dH), i = row - n * H;
        int ri[TAPS], ci[TAPS];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            ri[k] = up_clamp(2 * (int)i + K0 + k, 2 * H - 1);
            ci[k] = up_clamp(2 * (int)j + K0 + k, 2 * W - 1);
        }
        Vec8<T> v[TAPS][TAPS];
#pragma unroll
        for (int r = 0; r < TAPS; ++r)
#pragma unroll
            for (int q = 0; q < TAPS; ++q) v[r][q].load(dy + ((((size_t)n * 2 * H + ri[r]) * 2 * W + ci[q]) * CV + cv) * 8);
        float acc[8];
#pragma unroll
        for (int r = 0; r < TAPS; ++r)
#pragma unroll
            for (int q = 0; q < TAPS; ++q) {
                float f[8];
                v[r][q].unpack(f);
                if constexpr (MODE == SGG_UPSAMPLE_NEAREST) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] = (r | q) == 0 ? f[k] : __fadd_rn(acc[k], f[k]);
                } else {
                    const float w = ((r == 0 || r == 3) ? 0.25f : 0.75f) * ((q == 0 || q == 3) ? 0.25f : 0.75f);
                    if ((r | q) == 0) up_tap<true>(acc, f, w);
                    else up_tap<false>(acc, f, w);
                }
            }
        Vec8<T> o;
        o.pack(acc);
        o.store(dx + (size_t)e * 8);
    }
}

// the checks both entries share; > 0: nothing to launch
int up_check(const void* in, const void* out, int N, int H, int W, int Cp, int mode, int dtype, int64_t* vecs) {
    if (!in || !out || N < 0 || H < 0 || W < 0 || Cp < 0 || (Cp & 7) || ((uintptr_t)in & 15) || ((uintptr_t)out & 15)) return SGG_EINVAL;
    if (mode != SGG_UPSAMPLE_NEAREST && mode != SGG_UPSAMPLE_BILINEAR) return SGG_EINVAL;
    if (dtype != SGG_F32 && dtype != SGG_BF16) return SGG_EINVAL;
    if (N == 0 || H == 0 || W == 0 || Cp == 0) return 1;
    // (the product of four ints below 2^31 can pass 2^63: divide instead)
    int64_t lim = UP_MAX_VECS;
    for (int64_t d : {(int64_t)N, (int64_t)H, (int64_t)W, (int64_t)(Cp / 8)}) lim /= d;
    if (lim == 0) return SGG_EUNSUPPORTED;
    *vecs = (int64_t)N * H * W * (Cp / 8);
    return SGG_OK;
}

template <typename T, int MODE, bool BWD>
void up_launch_as(const void* in, void* out, int64_t vecs, int H, int W, int Cp, hipStream_t s) {
    const int64_t chunks = (vecs + UP_CHUNK - 1) / UP_CHUNK;
    const dim3 grid((unsigned)(chunks < UP_GRID_BLOCKS ? chunks : UP_GRID_BLOCKS)), block(UP_THREADS);
    const int CV = Cp / 8;
    const FastDiv dCV = make_fastdiv((uint32_t)CV), dW = make_fastdiv((uint32_t)W), dH = make_fastdiv((uint32_t)H);
    if constexpr (BWD)
        hipLaunchKernelGGL((upsample2x_bwd_kernel<T, MODE>), grid, block, 0, s, (const T*)in, (T*)out, (uint32_t)vecs, H, W, CV, dCV, dW, dH);
    else
        hipLaunchKernelGGL((upsample2x_fwd_kernel<T, MODE>), grid, block, 0, s, (const T*)in, (T*)out, (uint32_t)vecs, H, W, CV, dCV, dW, dH);
}

template <bool BWD> int up_launch(const void* in, void* out, int N, int H, int W, int Cp, int mode, int dtype, void* stream) {
    int64_t vecs = 0;
    const int rc = up_check(in, out, N, H, W, Cp, mode, dtype, &vecs);
    if (rc) return rc > 0 ? SGG_OK : rc;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SGG_F32 && mode == SGG_UPSAMPLE_NEAREST) up_launch_as<float, SGG_UPSAMPLE_NEAREST, BWD>(in, out, vecs, H, W, Cp, s);
    else if (dtype == SGG_F32) up_launch_as<float, SGG_UPSAMPLE_BILINEAR, BWD>(in, out, vecs, H, W, Cp, s);
    else if (mode == SGG_UPSAMPLE_NEAREST) up_launch_as<bf16, SGG_UPSAMPLE_NEAREST, BWD>(in, out, vecs, H, W, Cp, s);
    else up_launch_as<bf16, SGG_UPSAMPLE_BILINEAR, BWD>(in, out, vecs, H, W, Cp, s);
    return sgg_check_launch();
}

}  // namespace

extern "C" int sgg_upsample2x_fwd(const void* x, void* y, int N, int H, int W, int Cp, int mode, int dtype, void* stream) {
    return up_launch<false>(x, y, N, H, W, Cp, mode, dtype, stream);
}

extern "C" int sgg_upsample2x_bwd(const void* dy, void* dx, int N, int H, int W, int Cp, int mode, int dtype, void* stream) {
    return up_launch<true>(dy, dx, N, H, W, Cp, mode, dtype, stream);
}
