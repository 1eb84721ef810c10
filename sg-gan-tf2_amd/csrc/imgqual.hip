// imgqual.hip -- paired image-quality sums of the test pass: per image pair (a, b), over the 8-bit colours
//
//   out[n][0] = sum |a - b|,   out[n][1] = sum (a - b)^2      over all H * W * 3 values (integers: exact, order independent)
//   out[n][2] = sum of the SSIM map over the three channels and the (H - 10) * (W - 10) windows that lie inside the image
//
// SSIM is Wang et al.'s in the form of scikit-image's structural_similarity(gaussian_weights=True, sigma=1.5,
// use_sample_covariance=False, data_range=255, channel_axis=-1) [3P-recall]: an 11 x 11 separable Gaussian window
// w_k ~ exp(-k^2 / (2 * 1.5^2)), k = -5..5, normalised to sum 1; per window ux, uy, E[xx], E[yy], E[xy];
//   vx = E[xx] - ux^2,  vy = E[yy] - uy^2,  vxy = E[xy] - ux * uy
//   S  = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),   C1 = (0.01 * 255)^2,  C2 = (0.03 * 255)^2
// and the mean over the map cropped by 5 pixels [3P-recall], i.e. over the windows wholly inside the image: no border mode enters.
//
// Window moments, S and its sums are DOUBLE: the label maps this project scores are piecewise constant, where E[xx] - ux^2
// cancels to nothing and f32 would leave rounding noise of the size of C2; in double identical operands give S == 1.0 exactly
// (numerator and denominator are the same expressions of the same values).  The sum of S has a FIXED order: per thread in
// element order, a fixed shuffle tree per wave, the four waves in order, the blocks' partials in index order by the fold
// launch.  No floating-point atomics, no allocation, no host sync: two launches that can be captured.
#include "common.h"
#include <math.h>

namespace {

constexpr int IQ_THREADS = 256;
constexpr int IQ_TH = 16, IQ_TW = 32;               // valid output pixels (= windows) of a block
constexpr int IQ_TAPS = 11, IQ_R = 5;
constexpr int IQ_SH = IQ_TH + 2 * IQ_R, IQ_SW = IQ_TW + 2 * IQ_R;      // staged pixels: 26 x 42
constexpr int IQ_SWP = 44;                          // staged row pitch in bytes
constexpr int IQ_MAX_HW = 1 << 22;
constexpr int IQ_WAVES = IQ_THREADS / SGG_WAVE;

struct IqWeights { double w[IQ_TAPS]; };            // by value in the kernel arguments (SGPRs)

struct IqOperand {
    const void* p;
    int kind, cs, vec;
};

__device__ inline void iq_load(const IqOperand& o, int64_t i, int& r, int& g, int& b) {                 // o.kind is uniform
    if (o.kind == SGG_BF16) load_colour<SGG_BF16>(o.p, i, o.cs, o.vec != 0, r, g, b);
    else if (o.kind == SGG_F32) load_colour<SGG_F32>(o.p, i, o.cs, o.vec != 0, r, g, b);
    else load_colour<SGG_U8>(o.p, i, o.cs, false, r, g, b);
}

__device__ inline double wave_sum_f64(double v) {                       // a fixed tree: the same lanes meet in the same order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block `t` of image n owns the windows whose top-left pixel lies in [y0, y0 + IQ_TH) x [x0, x0 + IQ_TW) -- cut to the
// (H - 10) x (W - 10) valid extent -- and stages the pixels those windows cover, both operands, quantised, as bytes.  For the
// two integer sums the image is shared out by the same origin: a block counts the pixels of its own IQ_TH x IQ_TW cell, the
// last tile row / column also the 10 rows / columns of the border that follow its windows (all inside its staged window).
// Per channel: the horizontal pass writes the five row-filtered moments of every staged row to LDS (doubles, [moment][row][col]:
// a wave reads 32 consecutive doubles, conflict free), the vertical pass finishes the windows and forms S.
// ws: per image `tiles` doubles (SSIM partials), then `tiles` uint64 (sum |a-b|), then `tiles` uint64 (sum (a-b)^2).
__global__ __launch_bounds__(IQ_THREADS) void image_quality_kernel(const IqOperand A, const IqOperand B, int H, int W, int tiles_x, int tiles,
                                                                  const IqWeights wt, double* __restrict__ ws) {
    __shared__ uint8_t sa[3][IQ_SH][IQ_SWP], sb[3][IQ_SH][IQ_SWP];
    __shared__ double hrow[5][IQ_SH][IQ_TW];
    __shared__ double red_s[IQ_WAVES];
    __shared__ unsigned long long red_i[2][IQ_WAVES];

    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int tyi = t / tiles_x, txi = t - tyi * tiles_x;
    const int y0 = tyi * IQ_TH, x0 = txi * IQ_TW;
    const int vh = H - 2 * IQ_R, vw = W - 2 * IQ_R;
    const int th = min(IQ_TH, vh - y0), tw = min(IQ_TW, vw - x0);                      // this block's windows
    const int own_h = y0 + IQ_TH >= vh ? th + 2 * IQ_R : IQ_TH, own_w = x0 + IQ_TW >= vw ? tw + 2 * IQ_R : IQ_TW;
    const int64_t base = (int64_t)n * H * W;

    uint32_t sad = 0u, ssd = 0u;                     // a block's share: <= 26 * 42 * 3 * 255^2 < 2^32
    for (int e = threadIdx.x; e < IQ_SH * IQ_SW; e += IQ_THREADS) {
        const int ty = e / IQ_SW, tx = e - ty * IQ_SW;
        const int y = y0 + ty, x = x0 + tx;
        int ar = 0, ag = 0, ab = 0, br = 0, bg = 0, bb = 0;
        if (y < H && x < W) {                        // (pixels past the image are staged as zeros and belong to no window)
            const int64_t i = base + (int64_t)y * W + x;
            iq_load(A, i, ar, ag, ab);
            iq_load(B, i, br, bg, bb);
            if (ty < own_h && tx < own_w) {
                const int dr = ar - br, dg = ag - bg, db = ab - bb;
                sad += (uint32_t)(abs(dr) + abs(dg) + abs(db));
                ssd += (uint32_t)(dr * dr + dg * dg + db * db);
            }
        }
        sa[0][ty][tx] = (uint8_t)ar; sa[1][ty][tx] = (uint8_t)ag; sa[2][ty][tx] = (uint8_t)ab;
        sb[0][ty][tx] = (uint8_t)br; sb[1][ty][tx] = (uint8_t)bg; sb[2][ty][tx] = (uint8_t)bb;
    }
    __syncthreads();

    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double ssim = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int e = threadIdx.x; e < IQ_SH * IQ_TW; e += IQ_THREADS) {
            const int row = e / IQ_TW, col = e - row * IQ_TW;
            double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
            for (int k = 0; k < IQ_TAPS; ++k) {                                         // taps ascending
                const int xa = sa[c][row][col + k], xb = sb[c][row][col + k];           // products <= 65025: exact
                mx = fma(wt.w[k], (double)xa, mx);
                my = fma(wt.w[k], (double)xb, my);
                mxx = fma(wt.w[k], (double)(xa * xa), mxx);
                myy = fma(wt.w[k], (double)(xb * xb), myy);
                mxy = fma(wt.w[k], (double)(xa * xb), mxy);
            }
            hrow[0][row][col] = mx; hrow[1][row][col] = my; hrow[2][row][col] = mxx; hrow[3][row][col] = myy; hrow[4][row][col] = mxy;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < IQ_TH * IQ_TW; e += IQ_THREADS) {
            const int row = e / IQ_TW, col = e - row * IQ_TW;
            double ux = 0.0, uy = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
            for (int k = 0; k < IQ_TAPS; ++k) {
                ux = fma(wt.w[k], hrow[0][row + k][col], ux);
                uy = fma(wt.w[k], hrow[1][row + k][col], uy);
                exx = fma(wt.w[k], hrow[2][row + k][col], exx);
                eyy = fma(wt.w[k], hrow[3][row + k][col], eyy);
                exy = fma(wt.w[k], hrow[4][row + k][col], exy);
            }
            const double vx = exx - ux * ux, vy = eyy - uy * uy, vxy = exy - ux * uy;
            const double num = (2.0 * (ux * uy) + C1) * (2.0 * vxy + C2);
            const double den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
            if (row < th && col < tw) ssim += num / den;
        }
        __syncthreads();                             // hrow is rewritten by the next channel
    }

    const double ws_s = wave_sum_f64(ssim);
    const unsigned long long ws_a = wave_sum_u64(sad), ws_q = wave_sum_u64(ssd);
    const int wave = threadIdx.x / SGG_WAVE;
    if ((threadIdx.x & (SGG_WAVE - 1)) == 0) { red_s[wave] = ws_s; red_i[0][wave] = ws_a; red_i[1][wave] = ws_q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red_s[0];
        unsigned long long a = red_i[0][0], q = red_i[1][0];
#pragma unroll
        for (int w = 1; w < IQ_WAVES; ++w) { s += red_s[w]; a += red_i[0][w]; q += red_i[1][w]; }
        double* img_ws = ws + (size_t)n * 3 * tiles;
        unsigned long long* img_wi = reinterpret_cast<unsigned long long*>(img_ws + tiles);
        img_ws[t] = s; img_wi[t] = a; img_wi[tiles + t] = q;
    }
}

// One block per image: the SSIM partials are added in INDEX order by one thread (staged through LDS 256 at a time so the loads
// stay wide), the integer partials in 64 bits by all threads; each sum is converted / written once.
__global__ __launch_bounds__(IQ_THREADS) void image_quality_fold_kernel(const double* __restrict__ ws, int tiles, double* __restrict__ out) {
    __shared__ double chunk[IQ_THREADS];
    __shared__ unsigned long long red_i[2][IQ_WAVES];
    const int n = blockIdx.x;
    const double* img_ws = ws + (size_t)n * 3 * tiles;
    const unsigned long long* img_wi = reinterpret_cast<const unsigned long long*>(img_ws + tiles);
    unsigned long long a = 0ull, q = 0ull;
    for (int i = threadIdx.x; i < tiles; i += IQ_THREADS) { a += img_wi[i]; q += img_wi[tiles + i]; }
    a = wave_sum_u64(a); q = wave_sum_u64(q);
    if ((threadIdx.x & (SGG_WAVE - 1)) == 0) { red_i[0][threadIdx.x / SGG_WAVE] = a; red_i[1][threadIdx.x / SGG_WAVE] = q; }
    double s = 0.0;
    for (int i0 = 0; i0 < tiles; i0 += IQ_THREADS) {
        const int m = min(IQ_THREADS, tiles - i0);
        if ((int)threadIdx.x < m) chunk[threadIdx.x] = img_ws[i0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) s += chunk[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        unsigned long long ta = red_i[0][0], tq = red_i[1][0];
#pragma unroll
        for (int w = 1; w < IQ_WAVES; ++w) { ta += red_i[0][w]; tq += red_i[1][w]; }
        out[3 * n + 0] = (double)ta; out[3 * n + 1] = (double)tq; out[3 * n + 2] = s;
    }
}

int iq_operand(const void* p, int kind, int cs, IqOperand& o) {
    if (!p) return SGG_EINVAL;
    if (kind == SGG_U8) {
        if (cs != 3 && cs != 4) return SGG_EINVAL;
        o.vec = 0;
    } else if (kind == SGG_F32 || kind == SGG_BF16) {
        if (cs < 3) return SGG_EINVAL;
        o.vec = cs == SGG_CPAD && ((uintptr_t)p & 15) == 0;
    } else {
        return SGG_EINVAL;
    }
    o.p = p; o.kind = kind; o.cs = cs;
    return SGG_OK;
}

bool iq_shape_ok(int H, int W) { return H >= IQ_TAPS && W >= IQ_TAPS && (int64_t)H * W <= IQ_MAX_HW; }
int iq_tiles_x(int W) { return (W - 2 * IQ_R + IQ_TW - 1) / IQ_TW; }
int iq_tiles_y(int H) { return (H - 2 * IQ_R + IQ_TH - 1) / IQ_TH; }

}  // namespace

extern "C" size_t sgg_image_quality_workspace(int N, int H, int W) {
    if (N <= 0 || !iq_shape_ok(H, W)) return 0;
    return (size_t)N * 3 * sizeof(double) * (size_t)iq_tiles_x(W) * (size_t)iq_tiles_y(H);
}

extern "C" int sgg_image_quality(const void* a, int kind_a, int cstride_a, const void* b, int kind_b, int cstride_b, int N, int H, int W,
                                 double* out, void* ws, size_t ws_bytes, void* stream) {
    IqOperand A, B;
    int rc = iq_operand(a, kind_a, cstride_a, A);
    if (rc) return rc;
    rc = iq_operand(b, kind_b, cstride_b, B);
    if (rc) return rc;
    if (!out || !ws || N <= 0 || ((uintptr_t)ws & 7) || ((uintptr_t)out & 7)) return SGG_EINVAL;
    if (!iq_shape_ok(H, W)) return SGG_EUNSUPPORTED;
    const int tiles_x = iq_tiles_x(W), tiles = tiles_x * iq_tiles_y(H);
    if ((int64_t)tiles * N > 0x7fffffff) return SGG_EUNSUPPORTED;                       // the grid
    if (ws_bytes < sgg_image_quality_workspace(N, H, W)) return SGG_EWORKSPACE;
    IqWeights wt;                                                                        // the window, in double on the host
    double sum = 0.0;
    for (int k = 0; k < IQ_TAPS; ++k) {
        const double d = (double)(k - IQ_R);
        wt.w[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += wt.w[k];
    }
    for (int k = 0; k < IQ_TAPS; ++k) wt.w[k] /= sum;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(image_quality_kernel, dim3(tiles * N), dim3(IQ_THREADS), 0, s, A, B, H, W, tiles_x, tiles, wt, (double*)ws);
    hipLaunchKernelGGL(image_quality_fold_kernel, dim3(N), dim3(IQ_THREADS), 0, s, (const double*)ws, tiles, out);
    return sgg_check_launch();
}
