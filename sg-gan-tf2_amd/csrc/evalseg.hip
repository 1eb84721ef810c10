// evalseg.hip -- class-level evaluation of generated segmentation maps: a generated COLOUR image is decoded to
// class labels by the nearest entry of a palette {24-bit colour, class}, optionally scored against a ground-truth class map in
// the same launch, turned into class probabilities (the `probs` input of sgg_dense_crf), and scored on a boundary band.
//
//   q_c   = clamp((int)(((x_c + 1.f) * 0.5f) * 255.f), 0, 255)  for float input (NaN -> 0), the byte itself for uint8 input
//   d2_k  = sum_c (q_c - key_k.c)^2  (int32);   winner = smallest d2, ties to the LOWEST k
//   label = class[winner] if max_dist2 < 0 or d2 <= max_dist2, else other_class
//
// Everything here is integer (the probabilities apart) and order independent: the confusion matrix is counted in per-block LDS
// uint32 counters and flushed with 64-bit global atomic adds, so the same inputs give the same bits whatever the grid.
// The palette travels BY VALUE in the kernel arguments: no device allocation, no copy, and the call can be captured.
#include "common.h"
#include <math.h>

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_K = 64;                        // palette entries
constexpr int EV_MAX_CLASS = 64;                    // n_class: 64 * 64 uint32 LDS counters = 16 KB
constexpr int EV_MAX_R = 8;                         // boundary-band radius
constexpr int EV_TH = 16, EV_TW = 64;               // band: output tile of a block

struct EvPalette {                                  // decode order (ties to the lowest k)
    uint32_t key[EV_MAX_K];
    uint8_t cls[EV_MAX_K];
    int K, other_class, max_dist2;
};
struct EvClassPalette {                             // the same entries grouped by class: class c owns key[start[c] .. start[c + 1])
    uint32_t key[EV_MAX_K];
    uint8_t start[EV_MAX_CLASS + 1];
    int n_class, other_class, max_dist2;
    float neg_inv_2s2;                              // -1 / (2 sigma^2)
};

__device__ inline int dist2(int r, int g, int b, uint32_t key) {
    const int dr = r - (int)(key >> 16), dg = g - (int)((key >> 8) & 0xffu), db = b - (int)(key & 0xffu);
    return dr * dr + dg * dg + db * db;
}

__device__ inline int classify(const EvPalette& pal, int r, int g, int b) {
    int best = 0x7fffffff, cls = 0;
    for (int k = 0; k < pal.K; ++k) {                                  // k is uniform: the entry comes from the kernel arguments
        const int d = dist2(r, g, b, pal.key[k]);
        if (d < best) { best = d; cls = pal.cls[k]; }                  // strict: a tie keeps the lower k
    }
    return (pal.max_dist2 < 0 || best <= pal.max_dist2) ? cls : pal.other_class;
}

__device__ inline void count(uint32_t* cnt, int n_class, int t, int p) {
    if (t < n_class && p < n_class) atomicAdd(&cnt[n_class * t + p], 1u);
}

// One pixel per thread (float input), or four per thread (uint8 input with `vec`: 3 | 4 dword loads, the truth and select bytes
// as one dword each, the labels as one 16-byte store -- as seg_class_vec4_kernel reads its input); pixels past the last whole
// group of four, and every pixel of an input that is not `vec`, take the scalar path of the same launch.
template <int KIND, bool HIST>
__global__ __launch_bounds__(EV_THREADS) void palette_decode_kernel(const void* __restrict__ img, int64_t P, int cs, int vec, const EvPalette pal,
                                                                    int32_t* __restrict__ labels, const uint8_t* __restrict__ truth,
                                                                    const uint8_t* __restrict__ select, int n_class,
                                                                    unsigned long long* __restrict__ hist) {
    __shared__ uint32_t cnt[HIST ? EV_MAX_CLASS * EV_MAX_CLASS : 1];
    const int nbins = n_class * n_class;
    if (HIST) {
        for (int e = threadIdx.x; e < nbins; e += EV_THREADS) cnt[e] = 0u;
        __syncthreads();
    }
    const int64_t tid = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x, nthreads = (int64_t)gridDim.x * EV_THREADS;
    int64_t scalar_from = 0;
    if (KIND == SGG_U8 && vec) {
        const int64_t groups = P / 4;
        scalar_from = groups * 4;
        for (int64_t gi = tid; gi < groups; gi += nthreads) {
            uint32_t w[4];
            const uint32_t* src = static_cast<const uint32_t*>(img) + gi * cs;          // 4 pixels = cs dwords
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = k < cs ? src[k] : 0u;
            uint32_t tw = 0u, sw = 0x01010101u;
            if (HIST) {
                tw = reinterpret_cast<const uint32_t*>(truth)[gi];
                if (select) sw = reinterpret_cast<const uint32_t*>(select)[gi];
            }
            int lab[4];
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                int q[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int b3 = px * 3 + c, b4 = px * 4 + c;                         // byte position for cs = 3 and for cs = 4
                    const uint32_t v3 = w[b3 >> 2] >> (8 * (b3 & 3)), v4 = w[b4 >> 2] >> (8 * (b4 & 3));
                    q[c] = (int)((cs == 3 ? v3 : v4) & 0xffu);
                }
                lab[px] = classify(pal, q[0], q[1], q[2]);
                if (HIST && ((sw >> (8 * px)) & 0xffu)) count(cnt, n_class, (int)((tw >> (8 * px)) & 0xffu), lab[px]);
            }
            if (labels) {
                u32x4 o = {(uint32_t)lab[0], (uint32_t)lab[1], (uint32_t)lab[2], (uint32_t)lab[3]};
                st16(labels + gi * 4, o);
            }
        }
    }
    const bool fvec = KIND != SGG_U8 && vec;
    for (int64_t i = scalar_from + tid; i < P; i += nthreads) {
        int r, g, b;
        load_colour<KIND>(img, i, cs, fvec, r, g, b);
        const int lab = classify(pal, r, g, b);
        if (labels) labels[i] = lab;
        if (HIST && (!select || select[i])) count(cnt, n_class, truth[i], lab);
    }
    if (HIST) {
        __syncthreads();
        for (int e = threadIdx.x; e < nbins; e += EV_THREADS) {
            const uint32_t v = cnt[e];
            if (v) atomicAdd(&hist[e], (unsigned long long)v);
        }
    }
}

// p[n][c][i] = e_c / sum_c e_c,  e_c = exp(-(m_c - m_min) / (2 sigma^2)),  m_c = the smallest d2 over the entries of class c
// (other_class without an entry: the pseudo-distance max_dist2 where that is >= 0), m_min = min_c m_c; classes with no distance
// get exactly 0.  The distances are recomputed in each of the three passes (minimum, sum, store) instead of kept: a per-class
// array indexed by a run-time class would live in scratch, and the K * 3 integer distances are nothing next to the n_class stores.
template <int KIND>
__global__ __launch_bounds__(EV_THREADS) void palette_probs_kernel(const void* __restrict__ img, int N, int HW, int cs, int vec,
                                                                   const EvClassPalette pal, float* __restrict__ probs) {
    const int64_t P = (int64_t)N * HW;
    for (int64_t i = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * EV_THREADS) {
        int r, g, b;
        load_colour<KIND>(img, i, cs, vec != 0, r, g, b);
        const int NONE = 0x7fffffff;
        auto class_dist = [&](int c) {
            int m = NONE;
            const int j1 = pal.start[c + 1];
            for (int j = pal.start[c]; j < j1; ++j) m = min(m, dist2(r, g, b, pal.key[j]));
            if (j1 == pal.start[c] && c == pal.other_class && pal.max_dist2 >= 0) m = pal.max_dist2;
            return m;
        };
        int mmin = NONE;
        for (int c = 0; c < pal.n_class; ++c) mmin = min(mmin, class_dist(c));
        float sum = 0.f;
        for (int c = 0; c < pal.n_class; ++c) {
            const int m = class_dist(c);
            sum += m == NONE ? 0.f : expf((float)(m - mmin) * pal.neg_inv_2s2);
        }
        const int64_t n = i / HW;
        float* o = probs + (size_t)n * pal.n_class * HW + (size_t)(i - n * HW);
        for (int c = 0; c < pal.n_class; ++c) {
            const int m = class_dist(c);
            o[(size_t)c * HW] = m == NONE ? 0.f : expf((float)(m - mmin) * pal.neg_inv_2s2) / sum;
        }
    }
}

// band = 1 where the (2r+1)^2 window, cut to the image, holds a class other than the centre's: the window's minimum differs from
// its maximum.  A block stages its 16 x 64 output tile plus the halo in LDS (coordinates clamped to the image: the clamped pixel
// lies inside the cut window, so it adds nothing new and nothing outside the image is read), takes the row-wise minimum and
// maximum over 2r+1 columns, then the column-wise ones over 2r+1 rows.
__global__ __launch_bounds__(EV_THREADS) void class_boundary_band_kernel(const uint8_t* __restrict__ cls, uint8_t* __restrict__ band, int H, int W, int r) {
    constexpr int MAXH = EV_TH + 2 * EV_MAX_R, MAXW = EV_TW + 2 * EV_MAX_R;
    __shared__ uint8_t tile[MAXH * MAXW];
    __shared__ uint8_t rmin[MAXH * EV_TW], rmax[MAXH * EV_TW];
    const int x0 = blockIdx.x * EV_TW, y0 = blockIdx.y * EV_TH;
    const uint8_t* src = cls + (size_t)blockIdx.z * H * W;
    const int th = EV_TH + 2 * r, tw = EV_TW + 2 * r;
    for (int e = threadIdx.x; e < th * tw; e += EV_THREADS) {
        const int ty = e / tw, tx = e - ty * tw;
        const int y = min(max(y0 + ty - r, 0), H - 1), x = min(max(x0 + tx - r, 0), W - 1);
        tile[ty * MAXW + tx] = src[(size_t)y * W + x];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < th * EV_TW; e += EV_THREADS) {
        const int ty = e / EV_TW, tx = e - ty * EV_TW;
        int lo = 255, hi = 0;
        for (int d = 0; d <= 2 * r; ++d) {
            const int v = tile[ty * MAXW + tx + d];
            lo = min(lo, v); hi = max(hi, v);
        }
        rmin[e] = (uint8_t)lo; rmax[e] = (uint8_t)hi;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < EV_TH * EV_TW; e += EV_THREADS) {
        const int ty = e / EV_TW, tx = e - ty * EV_TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        int lo = 255, hi = 0;
        for (int d = 0; d <= 2 * r; ++d) {
            lo = min(lo, (int)rmin[(ty + d) * EV_TW + tx]); hi = max(hi, (int)rmax[(ty + d) * EV_TW + tx]);
        }
        band[((size_t)blockIdx.z * H + y) * W + x] = lo != hi ? 1 : 0;
    }
}

int ev_grid(int64_t work, int cap) {
    const int64_t b = (work + EV_THREADS - 1) / EV_THREADS;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// the caller's palette, or the library's built-in colour table (sgg_seg_class_table: the one copy, misc.hip) for NULL
int ev_palette(const uint32_t* keys_host, const uint8_t* classes_host, int K, uint32_t* key, uint8_t* cls, int& n) {
    if ((keys_host == nullptr) != (classes_host == nullptr)) return SGG_EINVAL;
    if (!keys_host) {
        n = sgg_seg_class_table(key, cls, EV_MAX_K);
        return n > 0 ? SGG_OK : SGG_EINVAL;
    }
    if (K < 1 || K > EV_MAX_K) return SGG_EINVAL;
    for (int k = 0; k < K; ++k) {
        if (keys_host[k] > 0xffffffu) return SGG_EINVAL;
        key[k] = keys_host[k]; cls[k] = classes_host[k];
    }
    n = K;
    return SGG_OK;
}

// element stride, pixel count and input kind; `vec` = the wide loads apply
int ev_input(const void* img, int kind, int64_t n_pixels, int cstride, int& vec) {
    if (!img || n_pixels <= 0) return SGG_EINVAL;
    if (n_pixels > 0x7fffffff) return SGG_EUNSUPPORTED;
    if (kind == SGG_U8) {
        if (cstride != 3 && cstride != 4) return SGG_EINVAL;
        vec = ((uintptr_t)img & 3) == 0;
    } else if (kind == SGG_F32 || kind == SGG_BF16) {
        if (cstride < 3) return SGG_EINVAL;
        vec = cstride == SGG_CPAD && ((uintptr_t)img & 15) == 0;
    } else {
        return SGG_EINVAL;
    }
    return SGG_OK;
}

template <bool HIST, typename... Args>
void launch_decode(int kind, int grid, hipStream_t s, Args... args) {
    if (kind == SGG_F32) hipLaunchKernelGGL((palette_decode_kernel<SGG_F32, HIST>), dim3(grid), dim3(EV_THREADS), 0, s, args...);
    else if (kind == SGG_BF16) hipLaunchKernelGGL((palette_decode_kernel<SGG_BF16, HIST>), dim3(grid), dim3(EV_THREADS), 0, s, args...);
    else hipLaunchKernelGGL((palette_decode_kernel<SGG_U8, HIST>), dim3(grid), dim3(EV_THREADS), 0, s, args...);
}

}  // namespace

extern "C" int sgg_palette_decode(const void* img, int kind, int64_t n_pixels, int cstride, const uint32_t* keys_host,
                                  const uint8_t* classes_host, int K, int other_class, int max_dist2, int32_t* labels,
                                  const uint8_t* truth, const uint8_t* select, int n_class, uint64_t* hist, void* stream) {
    EvPalette pal;
    int vec = 0;
    int rc = ev_input(img, kind, n_pixels, cstride, vec);
    if (rc) return rc;
    rc = ev_palette(keys_host, classes_host, K, pal.key, pal.cls, pal.K);
    if (rc) return rc;
    if (other_class < 0 || other_class > 255) return SGG_EINVAL;
    if (!labels && !hist) return SGG_EINVAL;                                               // nothing to write
    if ((truth == nullptr) != (hist == nullptr) || (select && !hist)) return SGG_EINVAL;
    if (hist) {
        if (n_class < 1 || n_class > EV_MAX_CLASS) return SGG_EINVAL;
        for (int k = 0; k < pal.K; ++k)
            if (pal.cls[k] >= n_class) return SGG_EINVAL;
    }
    for (int k = pal.K; k < EV_MAX_K; ++k) { pal.key[k] = 0u; pal.cls[k] = 0; }
    pal.other_class = other_class; pal.max_dist2 = max_dist2;
    if (kind == SGG_U8 && (((uintptr_t)labels | (uintptr_t)truth | (uintptr_t)select) & 3)) vec = 0;      // the dword forms of the side arrays
    if (kind == SGG_U8 && ((uintptr_t)labels & 15)) vec = 0;
    const int64_t work = kind == SGG_U8 && vec ? (n_pixels + 3) / 4 : n_pixels;
    hipStream_t s = (hipStream_t)stream;
    if (hist) launch_decode<true>(kind, ev_grid(work, 1024), s, img, n_pixels, cstride, vec, pal, labels, truth, select, n_class, (unsigned long long*)hist);
    else launch_decode<false>(kind, ev_grid(work, 2048), s, img, n_pixels, cstride, vec, pal, labels, truth, select, 1, (unsigned long long*)nullptr);
    return sgg_check_launch();
}

extern "C" int sgg_palette_probs(const void* img, int kind, int N, int HW, int cstride, const uint32_t* keys_host,
                                 const uint8_t* classes_host, int K, int other_class, int max_dist2, int n_class, float sigma,
                                 float* probs, void* stream) {
    uint32_t key[EV_MAX_K];
    uint8_t cls[EV_MAX_K];
    int n = 0, vec = 0;
    if (N <= 0 || HW <= 0) return SGG_EINVAL;
    int rc = ev_input(img, kind, (int64_t)N * HW, cstride, vec);
    if (rc) return rc;
    rc = ev_palette(keys_host, classes_host, K, key, cls, n);
    if (rc) return rc;
    if (!probs || n_class < 1 || n_class > EV_MAX_CLASS || other_class < 0 || other_class > 255 || !(sigma > 0.f)) return SGG_EINVAL;
    for (int k = 0; k < n; ++k)
        if (cls[k] >= n_class) return SGG_EINVAL;
    if (kind == SGG_U8) vec = 0;                                                           // one pixel per thread here
    EvClassPalette pal;
    int j = 0;
    for (int c = 0; c < EV_MAX_CLASS; ++c) {                                              // stable grouping by class
        pal.start[c] = (uint8_t)j;
        for (int k = 0; k < n; ++k)
            if (cls[k] == c) pal.key[j++] = key[k];
    }
    pal.start[EV_MAX_CLASS] = (uint8_t)j;
    for (; j < EV_MAX_K; ++j) pal.key[j] = 0u;
    pal.n_class = n_class; pal.other_class = other_class; pal.max_dist2 = max_dist2;
    pal.neg_inv_2s2 = (float)(-1.0 / (2.0 * (double)sigma * (double)sigma));
    const int64_t P = (int64_t)N * HW;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ev_grid(P, 2048)), blk(EV_THREADS);
    if (kind == SGG_F32) hipLaunchKernelGGL(palette_probs_kernel<SGG_F32>, grid, blk, 0, s, img, N, HW, cstride, vec, pal, probs);
    else if (kind == SGG_BF16) hipLaunchKernelGGL(palette_probs_kernel<SGG_BF16>, grid, blk, 0, s, img, N, HW, cstride, vec, pal, probs);
    else hipLaunchKernelGGL(palette_probs_kernel<SGG_U8>, grid, blk, 0, s, img, N, HW, cstride, vec, pal, probs);
    return sgg_check_launch();
}

extern "C" int sgg_class_boundary_band(const uint8_t* cls, uint8_t* band, int N, int H, int W, int r, void* stream) {
    if (!cls || !band || N <= 0 || H <= 0 || W <= 0 || r < 0 || r > EV_MAX_R) return SGG_EINVAL;
    if (N > 65535 || (H + EV_TH - 1) / EV_TH > 65535) return SGG_EUNSUPPORTED;
    const dim3 grid((W + EV_TW - 1) / EV_TW, (H + EV_TH - 1) / EV_TH, N);
    hipLaunchKernelGGL(class_boundary_band_kernel, grid, dim3(EV_THREADS), 0, (hipStream_t)stream, cls, band, H, W, r);
    return sgg_check_launch();
}
