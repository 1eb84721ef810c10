// warp.hip -- the augmented training copy's geometric warp (utils.py:80-103: Fliplr, Crop, Affine in random order on the squared
// image) over device-resident uint8 sources.  The host folds a sample's three operations into two 2x3 float64 matrices
// (sggan_amd/data.py: augment_matrices): `fill` maps an output point to the affine operation's input frame (zero fill is decided
// there), `full` maps it to the squared image A = resize(src, (S, S)).  A differs from the source along columns only, so
//   A[y][x][c] = ( sum_k cw[x][k] * src[index[n]][y][cs[x] + k][c] ) / 255                      (band_table((W0, S)))
// and the kernel writes   out[n][y][x] = inside(fill . p) ? bilinear(A, full . p - 0.5) : 0,   p = (x + 0.5, y + 0.5),
// as f32 (N, S, S, 4) with channel 3 zero -- the source of sgg_resample_f32.
//
// One block = 16 x 64 output pixels of one sample.  The maps are affine, so the pixels of A a tile can touch form a window whose
// size the caller knows (data.warp_window); the block first forms that window of A in LDS -- one band reduction per A pixel,
// straight from the uint8 source rows, which L2 serves -- and then every thread takes the four neighbours of its pixels from LDS.
// (At the crop's 0.2-0.6 scale an A pixel is a neighbour of ~10-100 output pixels, so forming A per tile instead of per
// neighbour removes most of the band arithmetic; the values are the same either way.)  Coordinates are float64, evaluated as
// (m0 * px + m1 * py) + m2 without contraction, exactly as data.apply_augment does; sums are f32 in a fixed order: taps
// ascending, then neighbours (y0,x0), (y0,x1), (y1,x0), (y1,x1).  Every index derived from a table or a matrix is clamped to the
// source / the window, so bad parameters give wrong pixels, never an out-of-range access.
#include "common.h"
#include <algorithm>

namespace {

constexpr int WP_TH = 16;           // output rows per block
constexpr int WP_TW = 64;           // output columns per block: the 256 threads are 4 waves of 64 lanes, each wave covers one output row at a time (1 KB stores)
constexpr int WP_THREADS = 256;
constexpr int WP_LDS = 64 * 1024;   // dynamic LDS budget (the default limit)

struct WarpArgs {
    const uint8_t* src; int M, S, W0;
    const int32_t* index; const double* mats;
    const float* cw; const int32_t* cs; int TC;
    float* out; int N;
    int wh, ww;                     // window of A per tile, in pixels
};

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// floor of a coordinate as an int that is safe to convert whatever the matrix holds (NaN -> -1)
__device__ inline int floor_to_int(double f, int S) { return (int)fmin(fmax(f, -1.0), (double)S); }

template <int CS>
__global__ __launch_bounds__(WP_THREADS) void warp_affine_u8_kernel(const WarpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    float4* win = reinterpret_cast<float4*>(lds);                 // [wh][ww] pixels of A
    const int t = threadIdx.x;
    const int n = blockIdx.z;
    const int x0t = blockIdx.x * WP_TW, y0t = blockIdx.y * WP_TH;
    const int S = a.S, TC = a.TC, ww = a.ww, wh = a.wh;
    const int sidx = clampi(a.index[n], 0, a.M - 1);
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = a.mats[(size_t)n * 12 + k];

    // window origin: the smallest neighbour coordinate over the tile = over its four corner pixels (the map is affine)
    double umin = 0.0, vmin = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double px = (double)(x0t + ((c & 1) ? WP_TW - 1 : 0)) + 0.5, py = (double)(y0t + ((c & 2) ? WP_TH - 1 : 0)) + 0.5;
        const double u = ((m[6] * px + m[7] * py) + m[8]) - 0.5, v = ((m[9] * px + m[10] * py) + m[11]) - 0.5;
        umin = c == 0 ? u : fmin(umin, u);
        vmin = c == 0 ? v : fmin(vmin, v);
    }
    const int ox = clampi(floor_to_int(floor(umin), S), 0, S - 1), oy = clampi(floor_to_int(floor(vmin), S), 0, S - 1);

    // the window of A: one column-band reduction per pixel, taps ascending
    const int64_t img_base = (int64_t)sidx * S;
    for (int e = t; e < wh * ww; e += WP_THREADS) {
        const int wy = e / ww, wx = e - wy * ww;
        const int ax = min(ox + wx, S - 1), ay = min(oy + wy, S - 1);
        const int start = clampi(a.cs[ax], 0, a.W0 - TC);
        const float* w = a.cw + (size_t)ax * TC;
        const uint8_t* p = a.src + ((img_base + ay) * a.W0 + start) * CS;
        float r = 0.f, g = 0.f, b = 0.f;
        for (int k = 0; k < TC; ++k) {
            const float wk = w[k];
            if (CS == 4) {
                const uint32_t u = *reinterpret_cast<const uint32_t*>(p + (size_t)k * 4);
                r = fmaf(wk, (float)(u & 255u), r);
                g = fmaf(wk, (float)((u >> 8) & 255u), g);
                b = fmaf(wk, (float)((u >> 16) & 255u), b);
            } else {
                r = fmaf(wk, (float)p[k * 3 + 0], r);
                g = fmaf(wk, (float)p[k * 3 + 1], g);
                b = fmaf(wk, (float)p[k * 3 + 2], b);
            }
        }
        win[e] = make_float4(r / 255.0f, g / 255.0f, b / 255.0f, 0.f);
    }
    __syncthreads();

    const int x = x0t + (t & (WP_TW - 1));
    if (x >= S) return;
    const double px = (double)x + 0.5;
    for (int ry = t / WP_TW; ry < WP_TH; ry += WP_THREADS / WP_TW) {
        const int y = y0t + ry;
        if (y >= S) break;
        const double py = (double)y + 0.5;
        const double fx = (m[0] * px + m[1] * py) + m[2], fy = (m[3] * px + m[4] * py) + m[5];
        const bool inside = fx >= 0.0 && fx <= (double)S && fy >= 0.0 && fy <= (double)S;
        const double u = ((m[6] * px + m[7] * py) + m[8]) - 0.5, v = ((m[9] * px + m[10] * py) + m[11]) - 0.5;
        const double fu = floor(u), fv = floor(v);
        const double bx = u - fu, by = v - fv;
        const int ix = floor_to_int(fu, S), iy = floor_to_int(fv, S);
        const int xa = clampi(clampi(ix, 0, S - 1) - ox, 0, ww - 1), xb = clampi(clampi(ix + 1, 0, S - 1) - ox, 0, ww - 1);
        const int ya = clampi(clampi(iy, 0, S - 1) - oy, 0, wh - 1), yb = clampi(clampi(iy + 1, 0, S - 1) - oy, 0, wh - 1);
        const float w00 = (float)((1.0 - by) * (1.0 - bx)), w01 = (float)((1.0 - by) * bx);
        const float w10 = (float)(by * (1.0 - bx)), w11 = (float)(by * bx);
        const float4 a00 = win[ya * ww + xa], a01 = win[ya * ww + xb], a10 = win[yb * ww + xa], a11 = win[yb * ww + xb];
        float4 o;
        o.x = fmaf(w11, a11.x, fmaf(w10, a10.x, fmaf(w01, a01.x, w00 * a00.x)));
        o.y = fmaf(w11, a11.y, fmaf(w10, a10.y, fmaf(w01, a01.y, w00 * a00.y)));
        o.z = fmaf(w11, a11.z, fmaf(w10, a10.z, fmaf(w01, a01.z, w00 * a00.z)));
        o.w = 0.f;
        if (!inside) o = make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(a.out)[((int64_t)n * S + y) * S + x] = o;
    }
}

}  // namespace

extern "C" int sgg_warp_affine_u8(const uint8_t* src, int M, int S, int W0, int Cs, const int32_t* index, const double* matrices,
                                  const float* col_w, const int32_t* col_start, int col_taps, int win_rows, int win_cols,
                                  float* out, int N, void* stream) {
    if (!src || !index || !matrices || !col_w || !col_start || !out) return SGG_EINVAL;
    if (M <= 0 || S <= 0 || W0 <= 0 || N <= 0 || (Cs != 3 && Cs != 4) || col_taps <= 0 || col_taps > W0) return SGG_EINVAL;
    if (win_rows <= 0 || win_cols <= 0) return SGG_EINVAL;
    if (((uintptr_t)out & 15) != 0 || ((uintptr_t)matrices & 7) != 0 || (Cs == 4 && ((uintptr_t)src & 3) != 0)) return SGG_EINVAL;
    if (N > 65535 || (S + WP_TH - 1) / WP_TH > 65535) return SGG_EUNSUPPORTED;
    const int wh = std::min(win_rows, S), ww = std::min(win_cols, S);
    if ((int64_t)wh * ww * (int64_t)sizeof(float4) > WP_LDS) return SGG_EUNSUPPORTED;
    WarpArgs a;
    a.src = src; a.M = M; a.S = S; a.W0 = W0; a.index = index; a.mats = matrices;
    a.cw = col_w; a.cs = col_start; a.TC = col_taps; a.out = out; a.N = N; a.wh = wh; a.ww = ww;
    const size_t lds = (size_t)wh * ww * sizeof(float4);
    dim3 grid((S + WP_TW - 1) / WP_TW, (S + WP_TH - 1) / WP_TH, N);
    hipStream_t s = (hipStream_t)stream;
    if (Cs == 3) hipLaunchKernelGGL((warp_affine_u8_kernel<3>), grid, dim3(WP_THREADS), lds, s, a);
    else hipLaunchKernelGGL((warp_affine_u8_kernel<4>), grid, dim3(WP_THREADS), lds, s, a);
    return sgg_check_launch();
}
