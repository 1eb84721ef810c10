// adam.hip -- the optimizer: Keras-form Adam (model.py:199-207) on a flat f32 buffer, with the step counter on the device, the
// linear rate decay (--lr_decay), the gradient guard (--clip_grad_norm / --skip_nonfinite) and the generator weight average
// (--ema_decay) as options of ONE family: five kernels, launched from one place (adam_launch, below).
//
//   gradsq_partial_kernel   guarded only: per GSQ_CHUNK elements of the gradient a sum of squares (double) and a non-finite flag
//   adam_prep_kernel        every entry but sgg_adam: one thread decides lr_t, the counter, the guard's verdict and d_t
//   adam_kernel             the update, scalar grid-stride walk                        (no average)
//   adam_ema_kernel         the update and the average, 16 bytes per lane on 5 streams  (sgg_adam_ema)
//   swap_f32_kernel         bitwise exchange of two buffers (the average <-> the live parameters)
// (DESIGN.md 25 lists which entry point launches which, with which options.)
//
// Nothing on the host after validation, no atomics, fixed summation order: two runs give the same bits, and a launch sequence
// can sit inside a captured HIP graph and be replayed.  The build has -ffp-contract=off and every element goes through the
// one adam_apply, so theta, m and v are the same bits whichever update kernel ran.
#include "common.h"

// One element of the update, on registers: advances m and v and returns what theta loses, theta_new = theta - adam_apply(...).
// (theta is not an argument so that the scalar kernel can fetch it after m and v are on their way out, as it always has: that
// order of its four streams measured 6 us per 11 M elements faster from a cold cache than all four loads up front.)
__device__ __forceinline__ float adam_apply(float g, float& m, float& v, float lr_t, float b1, float b2, float eps, float gs) {
    float gi = g * gs;
    float mi = b1 * m + (1.f - b1) * gi;
    float vi = b2 * v + (1.f - b2) * gi * gi;
    m = mi; v = vi;
    return lr_t * mi / (sqrtf(vi) + eps);
}

// The two pieces of the prep launch's arithmetic: the bias-corrected rate of step t (the formula sgg_adam evaluates on the
// host), and the reference's linear decay of the base rate (model.py:223, commented out there).  The epoch is iterations /
// steps_per_epoch, and `sched` = {steps_per_epoch, epoch_step, epochs} is read from device memory at run time -- never a kernel
// argument -- so a captured launch follows a descriptor that is written after the capture.  lr_e is rounded to f32 once (what
// a Keras learning_rate.assign would hold).
__device__ inline float adam_lr_t(float lr, int64_t t_, float b1, float b2) {
    const double t = (double)t_;
    return (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
}
__device__ inline float adam_sched_rate(int64_t it, const int64_t* sched, float lr) {
    const int64_t spe = sched[0] < 1 ? 1 : sched[0], epoch_step = sched[1], epochs = sched[2];
    const int64_t e = it / spe;
    float lr_e = lr;
    if (!(epochs <= epoch_step || e < epoch_step)) {
        const int64_t left = epochs - e > 0 ? epochs - e : 0;
        lr_e = (float)(((double)lr * (double)left) / (double)(epochs - epoch_step));
    }
    return lr_e;
}

// The chunk walks (sum of squares, update with the average, swap): block b owns elements [e0, e1) = chunk b of CHUNK elements,
// cut at n; v1 is the end of its whole 16-byte groups (e0 is a multiple of 4), [v1, e1) the n % 4 scalar tail.
struct ChunkSpan { int64_t e0, e1, v1; };
template <int CHUNK>
__device__ __forceinline__ ChunkSpan chunk_span(int64_t n) {
    ChunkSpan c;
    c.e0 = (int64_t)blockIdx.x * CHUNK;
    c.e1 = c.e0 + CHUNK < n ? c.e0 + CHUNK : n;
    c.v1 = c.e0 + ((c.e1 - c.e0) & ~(int64_t)3);
    return c;
}

// The 256 threads' (sum, flag) folded by one fixed tree; every thread returns with the block's pair.
__device__ __forceinline__ void block_fold_256(double& s, uint32_t& bad) {
    __shared__ double red[256];
    __shared__ uint32_t flag[256];
    red[threadIdx.x] = s; flag[threadIdx.x] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[threadIdx.x] += red[threadIdx.x + o]; flag[threadIdx.x] |= flag[threadIdx.x + o]; }
        __syncthreads();
    }
    s = red[0]; bad = flag[0];
}

// ---------------------------------------------------------------- the guard's pass over the gradient
// Workspace: a 16-byte decision header {u32 skip, f32 grad_scale * clip, 0, 0} followed by one 16-byte record per chunk.
// The chunk is a constant and the grid is ceil(n / GSQ_CHUNK): neither depends on the device, so neither does the sum.
#define GSQ_CHUNK 8192
struct GsqPartial { double sumsq; uint32_t bad, pad; };
static_assert(sizeof(GsqPartial) == 16, "one 16-byte record per chunk");
static inline int64_t gsq_chunks(int64_t n) { return (n + GSQ_CHUNK - 1) / GSQ_CHUNK; }

__device__ __forceinline__ void gsq_acc(const u32x4& c, double& s, uint32_t& bad) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // NaN / +-Inf by the bit pattern (exponent all ones): a finite sum that overflows is not "non-finite"
        bad |= (c[e] & 0x7f800000u) == 0x7f800000u;
        const double x = (double)__uint_as_float(c[e]);
        s += x * x;                                             // (an f32 squared is exact in double)
    }
}
__global__ __launch_bounds__(256) void gradsq_partial_kernel(const float* g, int64_t n, GsqPartial* part) {
    const ChunkSpan c = chunk_span<GSQ_CHUNK>(n);
    double s = 0.0;
    uint32_t bad = 0;
    // thread t takes the 16-byte groups t, t + 256, ... of the chunk in that order.  A whole chunk (every block but the last)
    // issues its 8 loads back to back -- 32 KiB in flight per block -- before the first is consumed; the last chunk walks
    // what it has, then the n % 4 scalar tail.  Same order either way, so a chunk's sum does not depend on which path ran.
    if (c.e1 - c.e0 == GSQ_CHUNK) {
        u32x4 r[GSQ_CHUNK / 1024];
#pragma unroll
        for (int u = 0; u < GSQ_CHUNK / 1024; ++u) r[u] = ld16(g + c.e0 + 4 * (threadIdx.x + 256 * u));
#pragma unroll
        for (int u = 0; u < GSQ_CHUNK / 1024; ++u) gsq_acc(r[u], s, bad);
    } else {
        for (int64_t i = c.e0 + 4 * threadIdx.x; i + 4 <= c.v1; i += 1024) gsq_acc(ld16(g + i), s, bad);
        if (c.v1 + threadIdx.x < c.e1) {
            u32x4 r = zero16();                                 // (+0.0 squared adds nothing and sets no flag)
            r[0] = __float_as_uint(g[c.v1 + threadIdx.x]);
            gsq_acc(r, s, bad);
        }
    }
    block_fold_256(s, bad);
    if (threadIdx.x == 0) { GsqPartial r; r.sumsq = s; r.bad = bad; r.pad = 0; part[blockIdx.x] = r; }
}

// ---------------------------------------------------------------- the prep launch
// `state` is int64[2]: [0] = iterations (Keras keeps `optimizer.iterations` as a variable too), [1] = scratch (the bits of lr_t
// for the step being applied).  One thread evaluates lr_t in double from t = iterations + 1 and bumps the counter; the update
// kernel reads the float.  The host never touches t.  (Evaluating pow() in every block of the update kernel cost +18 us per
// launch.)  The options, each a nullable pointer:
//   sched      the base rate goes through the linear decay first (NULL: no decay)
//   part       the guard.  One block of 256 threads, not one thread: they fold the chunk records (thread k takes records k,
//              k + 256, ... in order, then the fixed tree) -- a single thread walking the 1 400 - 2 700 records of a generator one
//              dependent load after the other would take longer than the pass that made them.  Thread 0 then decides, in double:
//                norm = sqrt(sumsq) * grad_scale;   skip = any flag;   clip = 1 if max_norm <= 0 or norm <= max_norm, else
//                (float)(max_norm / norm)
//              and writes the header and guard = {last_norm, last_clip, skipped_total, applied_total}.  On skip `iterations`
//              stays and lr_t = 0 is written: bias correction and the decay's epoch count follow APPLIED updates.
//              NULL: one thread; neither `head` nor `guard` is touched.
//   ema_state  {d_t, 1 - d_t} of the average tf.train.ExponentialMovingAverage(decay, num_updates) keeps, d_t = min(decay,
//              (1 + t) / (10 + t)) with t the number of applied updates, this one included; a skipped step keeps both, so the
//              average stays and a resumed run goes on along the ramp.  NULL: no average.
__global__ __launch_bounds__(256) void adam_prep_kernel(int64_t* state, const int64_t* sched, const GsqPartial* part, int chunks,
                                                        uint32_t* head, double* guard, float lr, float b1, float b2, float gs,
                                                        float max_norm, float ema_decay, float* ema_state) {
    bool skip = false;
    if (part) {
        double s = 0.0;
        uint32_t bad = 0;
        for (int k = threadIdx.x; k < chunks; k += 256) { const GsqPartial r = part[k]; s += r.sumsq; bad |= r.bad; }
        block_fold_256(s, bad);
        if (threadIdx.x != 0) return;
        const double norm = sqrt(s) * (double)gs;
        skip = bad != 0;
        float clip = 1.f;
        if (!skip && max_norm > 0.f && !(norm <= (double)max_norm)) clip = (float)((double)max_norm / norm);
        head[0] = skip ? 1u : 0u;
        head[1] = __float_as_uint(gs * clip);                   // the update's gradient factor, formed once in f32
        head[2] = 0u; head[3] = 0u;
        guard[0] = norm; guard[1] = (double)clip;
        guard[2] += skip ? 1.0 : 0.0; guard[3] += skip ? 0.0 : 1.0;
    } else if (threadIdx.x != 0) {
        return;
    }
    float lr_t = 0.f;
    if (!skip) {
        const int64_t it = state[0];
        lr_t = adam_lr_t(sched ? adam_sched_rate(it, sched, lr) : lr, it + 1, b1, b2);
        state[0] = it + 1;
        if (ema_state) {
            const double t = (double)(it + 1), ramp = (1.0 + t) / (10.0 + t);
            const float d = (float)((double)ema_decay < ramp ? (double)ema_decay : ramp);
            ema_state[0] = d;
            ema_state[1] = 1.f - d;
        }
    }
    reinterpret_cast<float*>(state + 1)[0] = lr_t;
}

// ---------------------------------------------------------------- the update
// head == NULL: the launch's grad_scale; otherwise the guard's header decides (skip: every stream keeps its bits) and carries
// grad_scale * clip.  state == NULL (sgg_adam): lr_t is the launch's; otherwise the prep launch's.
__global__ __launch_bounds__(256) void adam_kernel(float* th, const float* g, float* m, float* v, int64_t n, const int64_t* state,
                                                   const uint32_t* head, float lr_t, float b1, float b2, float eps, float gs) {
    if (head) {
        if (head[0]) return;
        gs = __uint_as_float(head[1]);
    }
    if (state) lr_t = reinterpret_cast<const float*>(state + 1)[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float mk = m[i], vk = v[i];
        const float step = adam_apply(g[i], mk, vk, lr_t, b1, b2, eps, gs);
        m[i] = mk; v[i] = vk;
        th[i] = th[i] - step;
    }
}

// The same with a fifth stream, ema = d_t ema + (1 - d_t) theta_new.  Block b owns chunk b of EMA_CHUNK elements.  A whole chunk
// issues its 2 x 5 16-byte loads back to back -- 40 KiB in flight per block -- before the first is consumed; the last chunk
// walks the 16-byte groups it has, then the n % 4 tail one element per thread.  No element is touched by two threads and
// nothing is accumulated across threads.
#define EMA_CHUNK 2048
static_assert(EMA_CHUNK % 1024 == 0, "a whole chunk is EMA_CHUNK / 1024 16-byte groups per thread");
static inline int64_t ema_chunks(int64_t n) { return (n + EMA_CHUNK - 1) / EMA_CHUNK; }

__device__ __forceinline__ void adam_ema_group(u32x4& th, const u32x4& g, u32x4& m, u32x4& v, u32x4& e, float lr_t, float b1, float b2,
                                               float eps, float gs, float d, float omd) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float t = __uint_as_float(th[k]), mk = __uint_as_float(m[k]), vk = __uint_as_float(v[k]);
        t = t - adam_apply(__uint_as_float(g[k]), mk, vk, lr_t, b1, b2, eps, gs);
        th[k] = __float_as_uint(t); m[k] = __float_as_uint(mk); v[k] = __float_as_uint(vk);
        e[k] = __float_as_uint(d * __uint_as_float(e[k]) + omd * t);
    }
}
__global__ __launch_bounds__(256) void adam_ema_kernel(float* th, const float* g, float* m, float* v, float* ema, int64_t n,
                                                       const int64_t* state, const uint32_t* head, const float* ema_state, float b1,
                                                       float b2, float eps, float gs) {
    if (head) {
        if (head[0]) return;
        gs = __uint_as_float(head[1]);
    }
    const float lr_t = reinterpret_cast<const float*>(state + 1)[0];
    const float d = ema_state[0], omd = ema_state[1];
    const ChunkSpan c = chunk_span<EMA_CHUNK>(n);
    if (c.e1 - c.e0 == EMA_CHUNK) {
        constexpr int U = EMA_CHUNK / 1024;
        u32x4 ct[U], cg[U], cm[U], cv[U], ce[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = c.e0 + 4 * (threadIdx.x + 256 * u);
            ct[u] = ld16(th + i); cg[u] = ld16(g + i); cm[u] = ld16(m + i); cv[u] = ld16(v + i); ce[u] = ld16(ema + i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = c.e0 + 4 * (threadIdx.x + 256 * u);
            adam_ema_group(ct[u], cg[u], cm[u], cv[u], ce[u], lr_t, b1, b2, eps, gs, d, omd);
            st16(th + i, ct[u]); st16(m + i, cm[u]); st16(v + i, cv[u]); st16(ema + i, ce[u]);
        }
    } else {
        for (int64_t i = c.e0 + 4 * threadIdx.x; i + 4 <= c.v1; i += 1024) {
            u32x4 ct = ld16(th + i), cg = ld16(g + i), cm = ld16(m + i), cv = ld16(v + i), ce = ld16(ema + i);
            adam_ema_group(ct, cg, cm, cv, ce, lr_t, b1, b2, eps, gs, d, omd);
            st16(th + i, ct); st16(m + i, cm); st16(v + i, cv); st16(ema + i, ce);
        }
        const int64_t i = c.v1 + threadIdx.x;
        if (i < c.e1) {
            float t = th[i], mk = m[i], vk = v[i];
            t = t - adam_apply(g[i], mk, vk, lr_t, b1, b2, eps, gs);
            th[i] = t; m[i] = mk; v[i] = vk;
            ema[i] = d * ema[i] + omd * t;
        }
    }
}

// Bitwise exchange of two buffers, same chunk walk (the payload never passes through a float: NaN bits survive).
__global__ __launch_bounds__(256) void swap_f32_kernel(uint32_t* a, uint32_t* b, int64_t n) {
    const ChunkSpan c = chunk_span<EMA_CHUNK>(n);
    if (c.e1 - c.e0 == EMA_CHUNK) {
        constexpr int U = EMA_CHUNK / 1024;
        u32x4 ca[U], cb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = c.e0 + 4 * (threadIdx.x + 256 * u);
            ca[u] = ld16(a + i); cb[u] = ld16(b + i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = c.e0 + 4 * (threadIdx.x + 256 * u);
            st16(a + i, cb[u]); st16(b + i, ca[u]);
        }
    } else {
        for (int64_t i = c.e0 + 4 * threadIdx.x; i + 4 <= c.v1; i += 1024) {
            const u32x4 ca = ld16(a + i), cb = ld16(b + i);
            st16(a + i, cb); st16(b + i, ca);
        }
        const int64_t i = c.v1 + threadIdx.x;
        if (i < c.e1) { const uint32_t x = a[i]; a[i] = b[i]; b[i] = x; }
    }
}

// ---------------------------------------------------------------- host: the one launch path
// What an entry point asks for, after its own validation.  Which launches run follows from the fields:
//   guarded            the sum-of-squares pass into ws (theta == NULL: that pass alone, sgg_grad_sumsq)
//   state != NULL      the prep launch (one thread, or one block when guarded); NULL: lr_t from the host's step number t
//   n > 0              the update: adam_ema_kernel if ema != NULL, adam_kernel otherwise
struct AdamCall {
    hipStream_t s;
    float* theta; const float* g; float *m, *v, *ema;
    int64_t n;
    int64_t* state; const int64_t* sched;
    bool guarded; double* guard; void* ws;
    float* ema_state;
    int t;
    float lr, b1, b2, eps, gs, max_norm, ema_decay;
};
static int adam_launch(const AdamCall& c) {
    GsqPartial* part = nullptr;
    uint32_t* head = nullptr;
    if (c.guarded) {
        head = (uint32_t*)c.ws;
        part = reinterpret_cast<GsqPartial*>((char*)c.ws + 16);
        hipLaunchKernelGGL(gradsq_partial_kernel, dim3((unsigned)gsq_chunks(c.n)), dim3(256), 0, c.s, c.g, c.n, part);
        const int rc = sgg_check_launch();
        if (rc || !c.theta) return rc;
    }
    float lr_t = 0.f;
    if (c.state) {
        hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(c.guarded ? 256 : 1), 0, c.s, c.state, c.sched, (const GsqPartial*)part,
                           c.guarded ? (int)gsq_chunks(c.n) : 0, head, c.guard, c.lr, c.b1, c.b2, c.gs, c.max_norm, c.ema_decay,
                           c.ema_state);
        const int rc = sgg_check_launch();
        if (rc) return rc;
    } else {
        lr_t = (float)((double)c.lr * sqrt(1.0 - pow((double)c.b2, c.t)) / (1.0 - pow((double)c.b1, c.t)));
    }
    if (c.n == 0) return SGG_OK;
    if (c.ema)
        hipLaunchKernelGGL(adam_ema_kernel, dim3((unsigned)ema_chunks(c.n)), dim3(256), 0, c.s, c.theta, c.g, c.m, c.v, c.ema, c.n,
                           (const int64_t*)c.state, (const uint32_t*)head, (const float*)c.ema_state, c.b1, c.b2, c.eps, c.gs);
    else
        hipLaunchKernelGGL(adam_kernel, dim3(grid_for(c.n, 2048)), dim3(256), 0, c.s, c.theta, c.g, c.m, c.v, c.n,
                           (const int64_t*)c.state, (const uint32_t*)head, lr_t, c.b1, c.b2, c.eps, c.gs);
    return sgg_check_launch();
}

static int grad_guard_args(const float* g, int64_t n, void* ws, size_t ws_bytes) {
    if (!g || !ws || n <= 0 || ((uintptr_t)g & 15) || ((uintptr_t)ws & 15) || gsq_chunks(n) > 0x7fffffff) return SGG_EINVAL;
    if (ws_bytes < sgg_grad_guard_workspace(n)) return SGG_EWORKSPACE;
    return SGG_OK;
}
static inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
static AdamCall adam_call(void* stream, float* theta, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                          float eps, float gs) {
    AdamCall c = {};
    c.s = (hipStream_t)stream; c.theta = theta; c.g = g; c.m = m; c.v = v; c.n = n;
    c.lr = lr; c.b1 = b1; c.b2 = b2; c.eps = eps; c.gs = gs;
    return c;
}

extern "C" {

int sgg_adam(float* theta, const float* g, float* m, float* v, int64_t n, int t, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (!theta || !g || !m || !v || n < 0 || t < 1) return SGG_EINVAL;
    if (n == 0) return SGG_OK;
    AdamCall c = adam_call(stream, theta, g, m, v, n, lr, beta1, beta2, eps, grad_scale);
    c.t = t;
    return adam_launch(c);
}

int sgg_adam_iter(float* theta, const float* g, float* m, float* v, int64_t n, int64_t* state, float lr, float beta1, float beta2,
                  float eps, float grad_scale, void* stream) {
    if (!theta || !g || !m || !v || !state || n < 0) return SGG_EINVAL;
    AdamCall c = adam_call(stream, theta, g, m, v, n, lr, beta1, beta2, eps, grad_scale);
    c.state = state;
    return adam_launch(c);                                      // (n == 0: the counter still advances)
}

int sgg_adam_sched(float* theta, const float* g, float* m, float* v, int64_t n, int64_t* state, const int64_t* sched, float lr,
                   float beta1, float beta2, float eps, float grad_scale, void* stream) {
    if (!theta || !g || !m || !v || !state || !sched || n < 0) return SGG_EINVAL;
    AdamCall c = adam_call(stream, theta, g, m, v, n, lr, beta1, beta2, eps, grad_scale);
    c.state = state; c.sched = sched;
    return adam_launch(c);
}

size_t sgg_grad_guard_workspace(int64_t n) {
    if (n <= 0) return 0;
    return 16 + (size_t)gsq_chunks(n) * sizeof(GsqPartial);
}
int sgg_grad_sumsq(const float* g, int64_t n, void* ws, size_t ws_bytes, void* stream) {
    int rc = grad_guard_args(g, n, ws, ws_bytes);
    if (rc) return rc;
    AdamCall c = {};
    c.s = (hipStream_t)stream; c.g = g; c.n = n; c.guarded = true; c.ws = ws;
    return adam_launch(c);
}
int sgg_adam_guard(float* theta, const float* g, float* m, float* v, int64_t n, int64_t* state, const int64_t* sched, float lr,
                   float beta1, float beta2, float eps, float grad_scale, float max_norm, double* guard, void* ws, size_t ws_bytes,
                   void* stream) {
    if (!theta || !m || !v || !state || !guard) return SGG_EINVAL;
    int rc = grad_guard_args(g, n, ws, ws_bytes);               // (g, n and the workspace, before anything is launched)
    if (rc) return rc;
    AdamCall c = adam_call(stream, theta, g, m, v, n, lr, beta1, beta2, eps, grad_scale);
    c.state = state; c.sched = sched; c.guarded = true; c.guard = guard; c.ws = ws; c.max_norm = max_norm;
    return adam_launch(c);
}

int sgg_adam_ema(float* theta, const float* g, float* m, float* v, float* ema, int64_t n, int64_t* state, const int64_t* sched, float lr,
                 float beta1, float beta2, float eps, float grad_scale, float ema_decay, float* ema_state, float max_norm, int guarded,
                 double* guard, void* ws, size_t ws_bytes, void* stream) {
    if (!theta || !g || !m || !v || !ema || !state || !ema_state || n <= 0 || ema_chunks(n) > 0x7fffffff) return SGG_EINVAL;
    if (!(ema_decay > 0.f && ema_decay < 1.f)) return SGG_EINVAL;
    if (misaligned16(theta) || misaligned16(g) || misaligned16(m) || misaligned16(v) || misaligned16(ema)) return SGG_EINVAL;
    if (guarded) {
        if (!guard) return SGG_EINVAL;
        int rc = grad_guard_args(g, n, ws, ws_bytes);           // (the workspace, before anything is launched)
        if (rc) return rc;
    }
    AdamCall c = adam_call(stream, theta, g, m, v, n, lr, beta1, beta2, eps, grad_scale);
    c.state = state; c.sched = sched; c.guarded = guarded != 0; c.guard = guard; c.ws = ws; c.max_norm = max_norm;
    c.ema = ema; c.ema_state = ema_state; c.ema_decay = ema_decay;
    return adam_launch(c);
}

int sgg_swap_f32(float* a, float* b, int64_t n, void* stream) {
    if (!a || !b || n <= 0 || ema_chunks(n) > 0x7fffffff || misaligned16(a) || misaligned16(b)) return SGG_EINVAL;
    hipLaunchKernelGGL(swap_f32_kernel, dim3((unsigned)ema_chunks(n)), dim3(256), 0, (hipStream_t)stream, (uint32_t*)a, (uint32_t*)b, n);
    return sgg_check_launch();
}

}  // extern "C"
