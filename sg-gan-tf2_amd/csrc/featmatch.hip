// featmatch.hip -- the feature-matching term of the paired step (Wang et al. 2018, pix2pixHD): for L pairs of
// discriminator activations (real_i, fake_i), NHWC with padded channels, given in ONE call
//
//   term   = (1/L) * sum_i  mean over (n,h,w,c < C_real_i) of | fake_i - real_i |
//   grad_i = (weight / (L * count_i)) * sign(fake_i - real_i),   count_i = P_i * C_real_i,   sign(0) = 0 stored as +0
//
// term goes to a 1-element f32 tensor of its own, weight * term is written to or added to the caller's loss scalar (bit 0 of
// `accumulate`, as sgg_l1_loss / sgg_ssim_loss); the reals are constants.  Padded channels (c >= C_real) get a +0 gradient and
// stay out of count_i.  A NaN difference gives a NaN term and a +0 gradient.
//
// Launches: TWO per call whatever L is -- one streaming launch over all layers, one single-block fold.  The per-layer table
// (FmTable) travels BY VALUE in the kernel arguments: no host-to-device copy and no device-resident table, so an eager step whose
// activations move every step and a captured step that must hold nothing the host rewrites are the same call.  A block owns one
// fixed chunk of FM_CHUNK consecutive 16-byte vectors of one layer (chunk0_i = the first block of layer i; the block finds its
// layer by comparing its index against the at most eight chunk0 values, in SGPRs).
//
// Arithmetic: d = (double)fake - (double)real, which is exact for both storage types.  |d| is summed in double in a FIXED order:
//   lane:   over its vectors tid, tid + 256, ... of the chunk in ascending order, the elements of a vector in ascending order;
//   wave:   the butterfly v += xor-shuffle(v, o) for o = 32, 16, 8, 4, 2, 1 (lane 0 reads the result);
//   block:  ((w0 + w1) + w2) + w3 over the four waves -> one double per chunk in the workspace;
//   fold:   layer i = its chunks' doubles added in index order, divided by count_i; term = ((m_0 + m_1) + ...) / L in double,
//           rounded ONCE to f32; the loss scalar takes (float)(weight * term), also one rounding from the double.
// grad_i's magnitude is (float)(weight / (L * count_i)) computed on the host, the sign applied, rounded once to the storage type.
// No atomics, nothing launch-shaped depends on data: runs agree bit for bit.
//
// Shape: a pure streaming kernel (as upsample.hip and dropout.hip): whole 16-byte loads and stores -- 8 bf16 or 4 f32 per lane --
// with 64-bit byte offsets, FM_UNROLL vectors of both inputs in flight per lane before the first is used, the default cache
// policy on the store (the consuming data-gradient kernel reads it next as its addend) and on the loads as in those two files
// (the fake halves are read again by the generator-gradient walk that follows).  Per vector 32 bytes are read and 16 written.
// The fold cannot share l1_final_kernel (misc.hip): that one reads f32 partials and adds them strided over 256 threads, this one
// adds double partials per layer in index order -- sharing the body would mean branching on the caller.
#include "common.h"

namespace {

constexpr int FM_THREADS = 256;
constexpr int FM_CHUNK = 4096;                       // 16-byte vectors per block: 16 per lane
constexpr int FM_UNROLL = 4;                         // vectors of each input a lane has in flight
constexpr int FM_TILE = 512;                         // partials per LDS tile of the fold (4 KB)
constexpr int FM_FOLD_BATCH = 16;                    // LDS reads the fold issues ahead of its in-order adds
constexpr int FM_MAX_LAYERS = SGG_FM_MAX_PAIRS;
constexpr int64_t FM_MAX_VECS = 0x7fffffffll;        // per layer: the vector index is 32-bit

struct FmLayer {
    const char* real;
    const char* fake;
    char* grad;
    int64_t nvec;                                    // 16-byte vectors of the layer (P * Cpad / VEC)
    int Cr, Cp;
    float gmag;                                      // (float)(weight / (L * count))
    int chunk0;                                      // index of the layer's first block / partial
};
struct FmTable {
    FmLayer l[FM_MAX_LAYERS];
    int L, chunks;
};

template <typename T>
__global__ __launch_bounds__(FM_THREADS) void fm_partial_kernel(const FmTable t, double* __restrict__ partial) {
    constexpr int VEC = ET<T>::VEC;
    const int b = (int)blockIdx.x;
    // the layer of this block: the last one whose first chunk is not past b (uniform: scalar selects, static indices only)
    const char* real = t.l[0].real; const char* fake = t.l[0].fake; char* grad = t.l[0].grad;
    int64_t nvec = t.l[0].nvec; int Cr = t.l[0].Cr, Cp = t.l[0].Cp, chunk0 = 0; float gmag = t.l[0].gmag;
#pragma unroll
    for (int i = 1; i < FM_MAX_LAYERS; ++i)
        if (i < t.L && b >= t.l[i].chunk0) {
            real = t.l[i].real; fake = t.l[i].fake; grad = t.l[i].grad;
            nvec = t.l[i].nvec; Cr = t.l[i].Cr; Cp = t.l[i].Cp; chunk0 = t.l[i].chunk0; gmag = t.l[i].gmag;
        }
    const uint32_t n = (uint32_t)nvec;                                   // <= FM_MAX_VECS (checked on the host)
    const uint32_t i0 = (uint32_t)(b - chunk0) * FM_CHUNK;               // < n: the host gives a layer ceil(n / FM_CHUNK) blocks
    const uint32_t i1 = n - i0 < (uint32_t)FM_CHUNK ? n : i0 + FM_CHUNK;
    const bool padded = Cr != Cp;
    const uint32_t vpp = (uint32_t)Cp / VEC;                             // vectors per pixel
    double s = 0.0;
    for (uint32_t base = i0 + threadIdx.x; base < i1; base += FM_THREADS * FM_UNROLL) {
        u32x4 fr[FM_UNROLL], rr[FM_UNROLL];
#pragma unroll
        for (int u = 0; u < FM_UNROLL; ++u) {
            const uint32_t i = base + u * FM_THREADS;
            if (i < i1) { fr[u] = ld16(fake + (size_t)i * 16); rr[u] = ld16(real + (size_t)i * 16); }
        }
#pragma unroll
        for (int u = 0; u < FM_UNROLL; ++u) {
            const uint32_t i = base + u * FM_THREADS;
            if (i < i1) {
                float fv[VEC], rv[VEC], g[VEC];
                ET<T>::unpack(fr[u], fv);
                ET<T>::unpack(rr[u], rv);
                const int c0 = padded ? (int)(i % vpp) * VEC : 0;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const double d = (double)fv[e] - (double)rv[e];
                    const bool in = !padded || c0 + e < Cr;
                    s += in ? fabs(d) : 0.0;
                    g[e] = in ? (d > 0.0 ? gmag : (d < 0.0 ? -gmag : 0.f)) : 0.f;
                }
                st16(grad + (size_t)i * 16, ET<T>::pack(g));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double wsum[FM_THREADS / SGG_WAVE];
    if ((threadIdx.x & (SGG_WAVE - 1)) == 0) wsum[threadIdx.x / SGG_WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[b] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one block: the partials pass through LDS in tiles of FM_TILE doubles (coalesced loads, FM_TILE / FM_THREADS per thread in flight;
// the step at 512x256, batch 8 takes three tiles); thread i < L adds the entries of layer i in index order -- the layers side by
// side, each in its own order, FM_FOLD_BATCH LDS reads issued ahead of the adds that consume them; thread 0 averages the layers
__global__ __launch_bounds__(FM_THREADS) void fm_fold_kernel(const FmTable t, const double* __restrict__ partial, int vec, double weight,
                                                             float* __restrict__ loss, float* __restrict__ term, int accumulate) {
    __shared__ double tile[FM_TILE];
    __shared__ double mean[FM_MAX_LAYERS];
    int c0 = 0, c1 = 0;                                                  // this thread's layer: chunks [c0, c1); threads >= L: none
    double count = 1.0;
#pragma unroll
    for (int i = 0; i < FM_MAX_LAYERS; ++i)
        if ((int)threadIdx.x == i && i < t.L) {
            c0 = t.l[i].chunk0;
            c1 = i + 1 < t.L ? t.l[(i + 1) % FM_MAX_LAYERS].chunk0 : t.chunks;
            count = (double)(t.l[i].nvec * vec / t.l[i].Cp) * (double)t.l[i].Cr;
        }
    double s = 0.0;
    for (int base = 0; base < t.chunks; base += FM_TILE) {               // (uniform bounds: every thread reaches both barriers)
#pragma unroll
        for (int j = 0; j < FM_TILE / FM_THREADS; ++j) {
            const int k = j * FM_THREADS + (int)threadIdx.x;
            tile[k] = base + k < t.chunks ? partial[base + k] : 0.0;
        }
        __syncthreads();
        const int lo = c0 > base ? c0 : base, hi = c1 < base + FM_TILE ? c1 : base + FM_TILE;
        for (int k = lo; k < hi; k += FM_FOLD_BATCH) {
            double v[FM_FOLD_BATCH];
#pragma unroll
            for (int j = 0; j < FM_FOLD_BATCH; ++j) {                    // lo - base <= index <= hi - 1 - base < FM_TILE
                const int q = k + j < hi ? k + j : hi - 1;
                v[j] = tile[q - base];
            }
#pragma unroll
            for (int j = 0; j < FM_FOLD_BATCH; ++j) s += k + j < hi ? v[j] : 0.0;      // (s >= +0: adding +0 leaves its bits)
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < t.L) mean[threadIdx.x] = s / count;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = mean[0];
        for (int i = 1; i < t.L; ++i) m += mean[i];
        m /= (double)t.L;
        *term = (float)m;
        const float l = (float)(weight * m);
        *loss = accumulate ? *loss + l : l;
    }
}

// the checks both entries share: fills the table (pointers aside, which only the launch needs)
int fm_plan(const sgg_fm_pair* pairs, int L, int dtype, bool pointers, FmTable* t) {
    if (!pairs || L < 1 || L > FM_MAX_LAYERS || (dtype != SGG_F32 && dtype != SGG_BF16)) return SGG_EINVAL;
    const int vec = dtype == SGG_BF16 ? 8 : 4;
    for (int i = 0; i < L; ++i) {
        const sgg_fm_pair& p = pairs[i];
        if (p.P <= 0 || p.Cpad <= 0 || p.Cpad % SGG_CPAD || p.C_real < 1 || p.C_real > p.Cpad) return SGG_EINVAL;
        if (pointers && (!p.real || !p.fake || !p.grad || (((uintptr_t)p.real | (uintptr_t)p.fake | (uintptr_t)p.grad) & 15))) return SGG_EINVAL;
    }
    int64_t chunks = 0;
    for (int i = 0; i < L; ++i) {
        const sgg_fm_pair& p = pairs[i];
        if (p.P > FM_MAX_VECS / (p.Cpad / vec)) return SGG_EUNSUPPORTED;
        FmLayer& y = t->l[i];
        y.real = (const char*)p.real; y.fake = (const char*)p.fake; y.grad = (char*)p.grad;
        y.nvec = p.P * (p.Cpad / vec);
        y.Cr = p.C_real; y.Cp = p.Cpad; y.gmag = 0.f;
        y.chunk0 = (int)chunks;
        chunks += (y.nvec + FM_CHUNK - 1) / FM_CHUNK;
    }
    for (int i = L; i < FM_MAX_LAYERS; ++i) t->l[i] = FmLayer{nullptr, nullptr, nullptr, 0, 0, 0, 0.f, 0};
    t->L = L; t->chunks = (int)chunks;                                   // <= 8 * 2^31 / 4096 = 2^22
    return SGG_OK;
}

}  // namespace

extern "C" size_t sgg_feature_match_workspace(const sgg_fm_pair* pairs, int L, int dtype) {
    FmTable t;
    return fm_plan(pairs, L, dtype, false, &t) == SGG_OK ? (size_t)t.chunks * sizeof(double) : 0;
}

extern "C" int sgg_feature_match(const sgg_fm_pair* pairs, int L, float weight, float* loss, float* term, int accumulate, int dtype,
                                 void* ws, size_t ws_bytes, void* stream) {
    FmTable t;
    if (!loss || !term) return SGG_EINVAL;
    const int rc = fm_plan(pairs, L, dtype, true, &t);
    if (rc) return rc;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < (size_t)t.chunks * sizeof(double)) return SGG_EWORKSPACE;
    const int vec = dtype == SGG_BF16 ? 8 : 4;
    for (int i = 0; i < L; ++i)
        t.l[i].gmag = (float)((double)weight / ((double)L * ((double)pairs[i].P * (double)pairs[i].C_real)));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SGG_BF16) hipLaunchKernelGGL(fm_partial_kernel<bf16>, dim3(t.chunks), dim3(FM_THREADS), 0, s, t, (double*)ws);
    else hipLaunchKernelGGL(fm_partial_kernel<float>, dim3(t.chunks), dim3(FM_THREADS), 0, s, t, (double*)ws);
    hipLaunchKernelGGL(fm_fold_kernel, dim3(1), dim3(FM_THREADS), 0, s, t, (const double*)ws, vec, (double)weight, loss, term, accumulate & 1);
    return sgg_check_launch();
}
