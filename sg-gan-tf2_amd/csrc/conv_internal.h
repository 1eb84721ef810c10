// conv_internal.h -- what the conv translation units (conv.hip, conv_halo3.hip, conv_wgrad.hip) share; only they include it.
// Every kernel is defined and launched in exactly one of them; what crosses files is the plain host functions declared at the end.
#pragma once
#include <type_traits>
#include "common.h"
#include <stdlib.h>

#ifdef SGG_LAB
#define SGG_ABLATE_OF(a) ((a).ablate)
#else
#define SGG_ABLATE_OF(a) 0      // the shipped kernels carry no ablation branches
#endif

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

struct ConvArgs {
    const char* src;     // FWD: x (N,H,W,C)    DGRAD: dy (N,Ho,Wo,K)
    const char* wmat;    // FWD: [K][R*S*C]     DGRAD: [C][R*S*K]
    const float* bias;   // per destination channel or nullptr
    char* dst;           // FWD: y (N,Ho,Wo,K)  DGRAD: dx (N,H,W,C)
    const char* addend;  // optional tensor added to the result (same layout as dst): the skip-connection gradient
    const char* fold;    // REFLECT DGRAD: pre-folded gather rows of the border pixels [pixel][tap][K], else nullptr
    float* stats;        // halo 3x3 kernels only: per-(image, pixel chunk, channel) partial sums for the instance norm next to
                         // the conv, [N][chunks][DC][2] f32; nullptr = not wanted.  Forward: (sum, sumsq) of the output.
                         // Data gradient: (sum g, sum g*xhat) of the norm backward that consumes dx, which needs:
    const char* nx;      //   that norm's input (same shape as dst)
    const float* nstats; //   its (mean, rstd)[N][DC]
    const float* ngamma; //   gamma, beta [DC]
    const float* nbeta;
    int nact; float nleak;   // and the activation fused behind it
    // Forward, "normalise on load" (NORM variant of the halo 3x3 kernel): src is the RAW output of the conv before the instance
    // norm in front of this conv; the kernel applies relu(x * A + B) (A = gamma * rstd, B = beta - mean * A, from nstats /
    // ngamma / nbeta; second network of a pair: ngamma2 / nbeta2) to the landed halo rows in LDS and writes the normalised
    // tensor -- which the backward pass needs as this conv's weight-gradient operand -- to nout on the way.
    char* nout;
    const float* ngamma2;
    const float* nbeta2;
    float* partial;      // split-K: f32 slabs [ksplit][pdst][DC]
    int ksplit;          // 1 = no split
    const char* wmat2;   // halo 3x3 kernels, two networks on one stacked batch: images >= nsplit use wmat2 / bias2
    const float* bias2;
    int nsplit;          //   (INT_MAX: one network)
    // Generic GEMM kernel, GROUPED launch of two networks' call sites of one shape (sgg_*_group2): grp = 2 doubles the grid's z
    // dimension; the second group reads / writes at these byte offsets from the pointers above and uses wmat2 / bias2.  Each
    // group is exactly the single-network launch (same tiles, same split-K), so results are bit-identical to two launches.
    int grp;
    size_t net_src, net_dst, net_add, net_part;
    int dst_f32;         // halo 3x3 data gradient, mixed mode: dst is f32 (the gradient chain between instance norms keeps f32)
    int addend_f32;      //   ... and so is the addend
    int ablate;          // lab build only (SGG_ABLATE; always 0 and compiled out otherwise): 1 no in-loop DMA, 2 no LDS reads/MFMAs, 3 = 1 + no barrier,
                         // 5 prologue + epilogue only, 6 prologue only (results in DESIGN.md section 7)
    size_t pdst;         // destination pixels (slab stride)
    int N, H, W, C, K, R, S, stride, pad_t, pad_l, Ho, Wo, reflect;
    int act;
    float leak;
};

// 16 zero bytes that out-of-range DMA lanes read instead of branching.  Internal linkage, one copy per file that uses it: the
// library is built without relocatable device code, so a device global cannot be shared across translation units.
static __device__ __attribute__((aligned(16))) uint32_t g_zero_page[4] = {0u, 0u, 0u, 0u};

// output tile and largest window of the kernels that keep a narrow layer's input halo in LDS (forward, narrow input, weight gradient)
#define HALO_TH 16
#define HALO_TW 32
#define HALO_MAXR 7

// The two 7x7 layers with a 3-channel side (bf16), each shape stated once: the head's forward and the stem's data gradient run
// conv7_narrow_out_kernel (conv.hip), both weight gradients wgrad7_kernel (conv_wgrad.hip).
static inline bool conv7_head_ok(const sgg_conv_desc* d) {      // 64 -> <= 3 (stored 8), 7x7, pad 3
    return sgg_config().n7 && d->dtype == SGG_BF16 && d->R == 7 && d->S == 7 && d->stride == 1 && d->C == 64 && d->K == 8 &&
           d->Ho == d->H && d->Wo == d->W && d->pad_t == 3 && d->pad_l == 3 && d->H >= 8 && d->W >= 8;
}
static inline bool conv7_stem_ok(const sgg_conv_desc* d) {      // <= 3 (stored 8) -> 64, 7x7, REFLECT 3
    return sgg_config().n7 && d->dtype == SGG_BF16 && d->R == 7 && d->S == 7 && d->stride == 1 && d->C == 8 && d->K == 64 &&
           d->Ho == d->H && d->Wo == d->W && d->pad_t == 3 && d->pad_l == 3 && d->pad_mode == SGG_PAD_REFLECT && d->H >= 8 && d->W >= 8;
}

// ---- conv_halo3.hip: the LDS-resident 3x3 stride-1 GEMM
bool halo3_ok(const sgg_conv_desc* d, int mode);                                       // the shape runs this kernel in direction `mode`
int launch_halo3(const ConvArgs& a, int mode, hipStream_t s);                          // picks FOLD / STATS / PAIR / SRC from the arguments
size_t halo3_stats_chunks(const sgg_conv_desc* d);                                     // statistics rows per image: one per (2 x 128 tile, tile row)
int halo3_norm_maxc();                                                                 // most source channels "normalise on load" takes

// ---- conv_wgrad.hip: the weight gradients.  One plan (plan_wgrad) decides the three answers below for a descriptor.
int wgrad_route(const sgg_conv_desc* d);                                               // the kernel run_wgrad launches (an sgg_route)
size_t wgrad_ws_bytes(const sgg_conv_desc* d);                                         // workspace of a single call; two networks: twice that
// (xb, dyb, dwb): the same call site of a SECOND network (sgg_*_bwd_weight_group2), nullptr: one network
int run_wgrad(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, hipStream_t s,
              const void* xb = nullptr, const void* dyb = nullptr, float* dwb = nullptr);
// the all-taps 3x3 kernel sums TWO applications (x, dy), (x2, dy2) of one layer into one dw (sgg_conv2d_bwd_weight_pair / pair2)
struct W9Net { const void* x; const void* dy; const void* x2; const void* dy2; float* dw; };
bool w9_ok(const sgg_conv_desc* d);                                                    // the shape runs that kernel: the pair form exists
bool w9_pair2_ok(const sgg_conv_desc* d);                                              // ... with an even split count: so does the two-network form
int run_w9(const sgg_conv_desc* d, const W9Net& na, const W9Net* nb, int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, hipStream_t s);
#ifdef SGG_LAB
int wgrad_debug_occupancy();                                                           // sgg_debug_occupancy's entry for conv_wgrad_kernel<bf16, 128, 128, 2>
#endif
