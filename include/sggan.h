/* sggan.h -- C ABI of the MI355X-native SG-GAN train-step kernels (libsggan.so).
 *
 * Drop-in boundary for the hot path of fhfonsecaa/SG-GAN-TF2.
 * The reference has no FFI layer of its own: its hot path is a chain of stock
 * TensorFlow/Keras ops called from Python (module.py:208-318, model.py:149-200).
 * Each entry point below replaces the TF op(s) at the cited reference call site;
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types.
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *     the caller owns all buffers including workspaces; nothing is allocated,
 *     freed or synchronised inside; calls are stream-ordered on `stream`
 *     (a hipStream_t passed as void*).
 *   - activations are NHWC with the channel count padded to a multiple of 8
 *     (SGG_CPAD); padded channels hold zeros.  dtype selects the storage type
 *     of activations and packed weights: SGG_F32 (parity path, f32 MFMA) or
 *     SGG_BF16 (performance path, bf16 MFMA, f32 accumulate).  Parameters,
 *     gradients of parameters, statistics, logits and losses are always f32.
 *   - return value: SGG_OK (0) or a negative sgg_status; sgg_strerror() names it.
 */
#ifndef SGGAN_H
#define SGGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGG_VERSION 100          /* major*10000 + minor*100 + patch */
#define SGG_CPAD 8               /* activation channel granule */

typedef enum { SGG_OK = 0, SGG_EINVAL = -1, SGG_EUNSUPPORTED = -2, SGG_ELAUNCH = -3, SGG_EWORKSPACE = -4 } sgg_status;
typedef enum { SGG_F32 = 0, SGG_BF16 = 1, SGG_U8 = 2 /* image input of sgg_palette_* and sgg_image_quality only */ } sgg_dtype;
typedef enum { SGG_ACT_NONE = 0, SGG_ACT_RELU = 1, SGG_ACT_LRELU = 2, SGG_ACT_TANH = 3 } sgg_act;
typedef enum { SGG_PAD_ZERO = 0, SGG_PAD_REFLECT = 1 } sgg_pad_mode;

/* Geometry of one convolution  y[n,ho,wo,k] = sum_{r,s,c} xpad[n, ho*stride - pad_t + r, wo*stride - pad_l + s, c] * w[r,s,c,k].
 * pad_mode ZERO : out-of-range taps read 0 (TF 'SAME' is expressed by the caller as
 *                 pad_t/pad_l = the LEADING pads; the trailing pad is implied by Ho/Wo).
 * pad_mode REFLECT: tf.pad(...,"REFLECT") of pad_t (= pad_l) followed by a VALID conv.
 * C and K are the PADDED channel counts (multiples of SGG_CPAD). */
typedef struct sgg_conv_desc {
    int32_t N, H, W, C;      /* conv input  (NHWC)  */
    int32_t K, R, S;         /* conv output channels, kernel height/width */
    int32_t stride;          /* 1 or 2 */
    int32_t pad_t, pad_l;
    int32_t Ho, Wo;          /* conv output spatial size */
    int32_t pad_mode;        /* sgg_pad_mode */
    int32_t dtype;           /* sgg_dtype */
} sgg_conv_desc;

int sgg_version(void);
const char* sgg_strerror(int status);

/* ---- measurement hooks (bench.py's roofline leg; not part of the drop-in surface) -----------------------------------
 * sgg_time_next_launch(start, stop) arms one pair of HIP events for the calling host thread: the next launch of a timed
 * kernel family's MAIN kernel made by that thread -- the 3x3 halo GEMMs (sgg_conv2d_fwd* / _bwd_data* on the
 * residual-block shape), the all-taps weight gradient (sgg_conv2d_bwd_weight*), the instance-norm apply pass
 * (sgg_instnorm_fwd*) -- carries them on its own dispatch packet (hipExtLaunchKernel), so sgg_event_elapsed_ms gives that
 * kernel's begin-to-end time on the launch stream, as rocprofv3's kernel trace does.  Helper launches of the same call
 * (side-tensor gather, slab reduce, norm finalize) are not included.  (NULL, NULL) disarms and returns 1 if the armed
 * pair was consumed by a launch, 0 if not; arming returns the same for the previous pair.  Not for use while a stream is
 * being captured. */
int sgg_event_create(void** ev);
int sgg_event_destroy(void* ev);
int sgg_event_elapsed_ms(void* start, void* stop, float* ms);
int sgg_time_next_launch(void* start, void* stop);
/* Number of nodes captured so far into the graph `stream` is being captured to (-1: the stream is not capturing).  The
 * host-side step recorder (sggan_amd/graph.py) uses it to see that a graph segment is still empty, so that consecutive
 * host actions (gradient all-reduce launches / waits) share one cut instead of recording empty graphs. */
int sgg_stream_capture_nodes(void* stream, int* n);

/* ---- weights -------------------------------------------------------------------
 * Keras kernel (HWIO f32, module.py:211 etc.; for Conv2DTranspose the (kh,kw,out,in)
 * kernel of module.py:254,258 IS the HWIO kernel of the equivalent conv) ->
 *   w_fwd  [Kpad][R*S*Cpad]  (K-major rows, reduction contiguous)  used by conv fwd / deconv bwd-data
 *   w_dgrad[Cpad][R*S*Kpad]                                         used by conv bwd-data / deconv fwd
 * in `dtype`, zero-filled padding.  Either output may be NULL. */
int sgg_pack_conv_weights(const float* w_hwio, int R, int S, int C, int K, int Cpad, int Kpad,
                          int dtype, void* w_fwd, void* w_dgrad, void* stream);

/* The same for every conv layer of a network in one launch (all packed weights go stale together at each optimizer step).
 * items_dev: DEVICE array of n_items entries; pointers are device pointers, w_fwd / w_dgrad may be NULL;
 * max_elems = max over items of taps*Cpad*Kpad. */
typedef struct sgg_pack_item {
    const float* w;      /* HWIO f32 kernel of the layer */
    void* w_fwd;
    void* w_dgrad;
    int32_t taps, C, K, Cpad, Kpad, reserved;
} sgg_pack_item;
int sgg_pack_conv_weights_batch(const sgg_pack_item* items_dev, int n_items, int64_t max_elems, int dtype, void* stream);

/* ---- conv2d: tf.keras.layers.Conv2D (+ tf.pad REFLECT) ---- module.py:210-216,230-232,236,240,262-264,284-311
 * fwd: y = act(conv(x) + bias);  bias may be NULL; bias has Kpad f32 entries.
 * ws: sgg_conv2d_fwd_workspace() bytes (non-zero only for small outputs, which are computed split-K).
 * Status of every conv2d / deconv2d forward and data-gradient entry below (plain, _stats, _mixed, _pair, _normload, _group2),
 * decided in this order before anything is launched: SGG_EINVAL -- a NULL or invalid descriptor, a transposed conv with a
 * padding mode other than zero, a NULL pointer among the required operands, nsplit outside 1..N-1 where a second weight set
 * is given; SGG_EUNSUPPORTED -- the shape or dtype has no such form (the *_supported / *_stats_chunks queries say so
 * beforehand); SGG_EWORKSPACE -- ws is NULL or smaller than the call needs, which is at most what the entry's workspace query reports (a
 * _group2 call: twice that). */
size_t sgg_conv2d_fwd_workspace(const sgg_conv_desc* d);
int sgg_conv2d_fwd(const sgg_conv_desc* d, const void* x, const void* w_fwd, const float* bias,
                   void* y, int act, float leak, void* ws, size_t ws_bytes, void* stream);

/* conv2d forward that also emits, for the instance norm that follows it (module.py:211-212 etc.), the per-image
 * per-channel (sum, sum of squares) of the stored output, split over pixel chunks:
 *   partial[N][chunks][Kpad][2] f32,  chunks = sgg_conv2d_fwd_stats_chunks(d)  (0: this shape has no such epilogue;
 *   currently the bf16 3x3 stride-1 kernel).  No activation (the norm applies it).  Feed partial to
 *   sgg_instnorm_fwd_partial(), which then skips its own statistics pass over the tensor. */
size_t sgg_conv2d_fwd_stats_chunks(const sgg_conv_desc* d);
int sgg_conv2d_fwd_stats(const sgg_conv_desc* d, const void* x, const void* w_fwd, const float* bias, void* y,
                         float* partial, void* ws, size_t ws_bytes, void* stream);
/* bwd_data: dx = conv^T(dy) including the MirrorPadGrad fold for REFLECT (gen_tape.gradient, model.py:196).
 * ws: sgg_conv2d_bwd_data_workspace() bytes (REFLECT: pre-folded gather rows of the border pixels; small outputs: split-K slabs). */
size_t sgg_conv2d_bwd_data_workspace(const sgg_conv_desc* d);
/* addend (nullable, same shape/dtype as dx): dx = conv^T(dy) + addend -- the skip-connection gradient of a
 * residual block (module.py:217) folded into the epilogue.
 * Rounding: dx (+ addend) is accumulated in f32 and rounded to the storage type ONCE, with one exception.  A bf16 REFLECT
 * data gradient without addend on the HALO_NARROW_IN / HALO_DGRAD_NARROW routes (sgg_conv2d_route) is two launches: the
 * main one pads with zeros and stores dx rounded to bf16, the border fold reads that value back, adds MirrorPadGrad's
 * mirrored terms and rounds a SECOND time.  On the pixels those terms reach (rows and columns 1..p and H-1-p..H-2,
 * W-1-p..W-2) dx is bf16(bf16(dx_zero_padded) + mirrored terms); everywhere else, on every other route (N7 folds in f32, the
 * generic GEMM folds dy before it multiplies) and in f32 it is the once-rounded value. */
int sgg_conv2d_bwd_data(const sgg_conv_desc* d, const void* dy, const void* w_dgrad, const void* addend, void* dx,
                        void* ws, size_t ws_bytes, void* stream);

/* conv2d data gradient that also emits the first pass of the instance-norm BACKWARD that consumes dx (the norm in front of
 * this conv in the forward direction, module.py:212-215): partial[N][chunks][Cpad][2] = per pixel chunk (sum g, sum g*xhat),
 * g = dx * act'(gamma*xhat + beta), xhat = (norm_x - mean) * rstd from norm_stats (as written by sgg_instnorm_fwd).
 * chunks = sgg_conv2d_bwd_data_stats_chunks(d) (0: unsupported shape; currently the bf16 3x3 stride-1 kernel).
 * Feed partial to sgg_instnorm_bwd_partial().  ws as for sgg_conv2d_bwd_data. */
size_t sgg_conv2d_bwd_data_stats_chunks(const sgg_conv_desc* d);
int sgg_conv2d_bwd_data_stats(const sgg_conv_desc* d, const void* dy, const void* w_dgrad, const void* addend, void* dx,
                              const void* norm_x, const float* norm_stats, const float* norm_gamma, const float* norm_beta,
                              int norm_act, float norm_leak, float* partial, void* ws, size_t ws_bytes, void* stream);
/* Mixed-precision data gradient (an extension; the reference trains in f32 throughout, gen_tape.gradient model.py:196):
 * bf16 operands, dx written in F32 -- and the addend read as f32 when addend_is_f32 -- so that the gradient chain
 * between the instance norms of the residual blocks is not re-rounded to bf16 at every layer (the norm backward
 * subtracts most of dy; a rounding relative to dy is amplified there).  Supported where
 * sgg_conv2d_bwd_data_mixed_supported(d) returns 1 (the bf16 3x3 stride-1 kernel); ws as for sgg_conv2d_bwd_data. */
int sgg_conv2d_bwd_data_mixed_supported(const sgg_conv_desc* d);
int sgg_conv2d_bwd_data_mixed(const sgg_conv_desc* d, const void* dy, const void* w_dgrad, const void* addend, int addend_is_f32,
                              float* dx, void* ws, size_t ws_bytes, void* stream);
/* The lockstep pair (see sgg_instnorm_*_pair): d describes the STACKED batch (N = both networks' images); images
 * 0..nsplit-1 are convolved with (w, bias), the rest with (w2, bias2), in ONE launch -- where sgg_conv2d_pair_supported(d)
 * returns 1 (the bf16 3x3 stride-1 kernels); elsewhere call the one-network entry points on the two halves. */
int sgg_conv2d_pair_supported(const sgg_conv_desc* d);
int sgg_conv2d_fwd_stats_pair(const sgg_conv_desc* d, const void* x, const void* w_fwd, const float* bias, const void* w_fwd2,
                              const float* bias2, int nsplit, void* y, float* partial, void* ws, size_t ws_bytes, void* stream);
int sgg_conv2d_bwd_data_pair(const sgg_conv_desc* d, const void* dy, const void* w_dgrad, const void* w_dgrad2, int nsplit,
                             const void* addend, void* dx, void* ws, size_t ws_bytes, void* stream);
/* "Normalise on load" -- conv -> InstanceNormalization -> ReLU -> conv (the residual block, module.py:211-215) without the
 * norm's apply pass over the tensor: x_raw is the FIRST conv's raw output, x_stats its (mean, rstd)[N][C]
 * (sgg_instnorm_finalize over the first conv's statistics rows), x_gamma / x_beta the norm's parameters.  The second conv
 * applies relu(x * gamma * rstd + beta - mean * gamma * rstd) to its operand tiles after they land in LDS and writes the
 * normalised tensor to x_norm on the way (the backward pass needs it as this conv's weight-gradient operand).  y, partial:
 * as sgg_conv2d_fwd_stats.  w2 == NULL: one network; else the lockstep pair (images >= nsplit use w2 / bias2 / x_gamma2 /
 * x_beta2).  x_norm, y and partial are bit-identical to sgg_instnorm_fwd_partial(act = RELU) followed by sgg_conv2d_fwd_stats.
 * Supported where sgg_conv2d_fwd_normload_supported(d) returns 1 (bf16, REFLECT 3x3 stride 1, C <= 512). */
int sgg_conv2d_fwd_normload_supported(const sgg_conv_desc* d);
int sgg_conv2d_fwd_stats_normload(const sgg_conv_desc* d, const void* x_raw, const float* x_stats, const float* x_gamma, const float* x_beta,
                                  const float* x_gamma2, const float* x_beta2, void* x_norm, const void* w_fwd, const float* bias,
                                  const void* w_fwd2, const float* bias2, int nsplit, void* y, float* partial,
                                  void* ws, size_t ws_bytes, void* stream);
/* bwd_weight: dw_hwio[R][S][C_real][K_real] f32, overwritten (accumulate=0) or added to (accumulate=1: a network
 * applied twice in one step, model.py:186-187).  ws: sgg_conv2d_bwd_weight_workspace() bytes. */
size_t sgg_conv2d_bwd_weight_workspace(const sgg_conv_desc* d);
int sgg_conv2d_bwd_weight(const sgg_conv_desc* d, const void* x, const void* dy, float* dw_hwio,
                          int C_real, int K_real, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* Weight gradient of TWO applications of one layer in a step (same desc): dw (+)= wgrad(x0, dy0) + wgrad(x1, dy1) with one
 * launch, one set of split slabs and one reduce (the cycle step applies each generator twice, model.py:120-121 by name).
 * sgg_conv2d_bwd_weight_pair_supported() tells whether the shape has this path (the all-taps 3x3 stride-1 kernel);
 * otherwise call sgg_conv2d_bwd_weight twice.  Workspace: sgg_conv2d_bwd_weight_workspace(d). */
int sgg_conv2d_bwd_weight_pair_supported(const sgg_conv_desc* d);
int sgg_conv2d_bwd_weight_pair(const sgg_conv_desc* d, const void* x0, const void* dy0, const void* x1, const void* dy1,
                               float* dw, int C_real, int K_real, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* ... of TWO networks of one architecture, each applied twice (the upstream cycle step's generators): four (x, dy) sets, two dW, ONE
 * launch in which each network gets half the blocks -- half as many f32 slabs to write and reduce.  Same result as two
 * sgg_conv2d_bwd_weight_pair calls up to f32 summation order.  Workspace as for one network. */
int sgg_conv2d_bwd_weight_pair2(const sgg_conv_desc* d, const void* xa0, const void* dya0, const void* xa1, const void* dya1, float* dwa,
                                const void* xb0, const void* dyb0, const void* xb1, const void* dyb1, float* dwb,
                                int Cr, int Kr, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---- grouped launches: the same call site of TWO networks of one architecture in one call (the upstream cycle step runs
 * G_A->B beside G_B->A and D_A beside D_B; module.py:219-318 built twice).  `d` describes ONE network's call (N images per
 * network); x / y (dy / dx, addend) are the STACKED tensors of 2N images, the first network's images first; (w, bias) belong to
 * the first network, (w2, bias2) to the second.  The result is bit for bit that of two single calls -- each group runs the
 * single call's tiles and split-K -- but in ONE launch for the generic GEMM and the stacked-batch halo kernels (two half-size
 * launches of the discriminators' small maps are latency bound); the special 7x7 / narrow kernels run as two launches.
 * ws >= 2 x the single call's workspace.  (3x3 stride-1 shapes with the norm-statistics epilogue or REFLECT fold:
 * sgg_conv2d_fwd_stats_pair / sgg_conv2d_bwd_data_pair.) */
int sgg_conv2d_fwd_group2(const sgg_conv_desc* d, const void* x, const void* w, const float* bias, const void* w2,
                          const float* bias2, void* y, int act, float leak, void* ws, size_t ws_bytes, void* stream);
int sgg_conv2d_bwd_data_group2(const sgg_conv_desc* d, const void* dy, const void* w, const void* w2, const void* addend,
                               void* dx, void* ws, size_t ws_bytes, void* stream);
/* weight gradients of the two networks: their main kernels run back to back into two sets of split slabs, ONE reduce launch sums
 * both (each in the single call's order).  dw / dw2: the two networks' f32 gradients, layouts as sgg_conv2d_bwd_weight.
 * Exception -- the 3x3 all-taps halo shapes (stride 1 pad 1, or stride 2; 64 | C, 128 | K; also as Conv2DTranspose) and the
 * LDS-DMA kernel's shapes (K >= 256 and R*S*C >= 256): ONE main launch in which each network
 * gets half the blocks and half the split slabs (the slabs are that kernel's main memory traffic); the result then equals two
 * single calls up to f32 summation order (~1e-6 relative), not bit for bit. */
int sgg_conv2d_bwd_weight_group2(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, float* dw2, int C_real, int K_real,
                                 int accumulate, void* ws, size_t ws_bytes, void* stream);
int sgg_deconv2d_bwd_weight_group2(const sgg_conv_desc* d, const void* x, const void* dy, float* dw, float* dw2, int C_real, int K_real,
                                   int accumulate, void* ws, size_t ws_bytes, void* stream);
int sgg_deconv2d_fwd_group2(const sgg_conv_desc* d, const void* x, const void* w_dgrad, const float* bias, const void* w_dgrad2,
                            const float* bias2, void* y, int act, float leak, void* ws, size_t ws_bytes, void* stream);
int sgg_deconv2d_bwd_data_group2(const sgg_conv_desc* d, const void* dy, const void* w_fwd, const void* w_fwd2, void* dx,
                                 void* ws, size_t ws_bytes, void* stream);

/* ---- deconv2d: tf.keras.layers.Conv2DTranspose(3x3, s2, 'same') ---- module.py:254,258
 * `d` describes the EQUIVALENT FORWARD CONV whose input is the deconv OUTPUT:
 *   (d->N,H,W,C) = deconv output, (d->Ho,Wo,K) = deconv input, pad_t/pad_l = TF SAME leading pads of that conv.
 * fwd: y[N,H,W,C] = act(conv^T(x[N,Ho,Wo,K]) + bias[C]). */
size_t sgg_deconv2d_fwd_workspace(const sgg_conv_desc* d);
int sgg_deconv2d_fwd(const sgg_conv_desc* d, const void* x, const void* w_dgrad, const float* bias,
                     void* y, int act, float leak, void* ws, size_t ws_bytes, void* stream);
/* the same (no activation) + the per-chunk (sum, sumsq) rows partial[N][chunks][C][2] of the STORED output for the InstanceNormalization
 * behind the layer (module.py:255,259), so that sgg_instnorm_fwd_partial() skips its statistics pass; chunks = sgg_deconv2d_fwd_stats_chunks(d),
 * 0 where the shape has no such epilogue.  w2 != NULL: a stacked batch of two networks, images >= nsplit use w2 / bias2. */
size_t sgg_deconv2d_fwd_stats_chunks(const sgg_conv_desc* d);
int sgg_deconv2d_fwd_stats(const sgg_conv_desc* d, const void* x, const void* w_dgrad, const float* bias, const void* w_dgrad2, const float* bias2,
                           int nsplit, void* y, float* partial, void* ws, size_t ws_bytes, void* stream);
size_t sgg_deconv2d_bwd_data_workspace(const sgg_conv_desc* d);
int sgg_deconv2d_bwd_data(const sgg_conv_desc* d, const void* dy, const void* w_fwd, void* dx,
                          void* ws, size_t ws_bytes, void* stream);
/* dw has the Keras transpose-kernel layout [R][S][C_real(out)][K_real(in)]. */
int sgg_deconv2d_bwd_weight(const sgg_conv_desc* d, const void* x, const void* dy, float* dw,
                            int C_real, int K_real, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---- route query: which kernel a plain call of this geometry launches (host only: nothing is launched, no device is touched)
 * The code is computed by the selection functions the launchers themselves switch on.  It names the kernel family and, for
 * the generic GEMMs, the block tile; SGG_ROUTE_SPLITK is OR-ed in when the GEMM planner splits the reduction (partial slabs
 * + splitk_reduce_kernel).  "Plain": no addend, no paired weights, no statistics epilogue (an addend moves the data gradient
 * of HALO_NARROW_IN / HALO_DGRAD_NARROW shapes to the generic GEMM); the weight-gradient query takes C_real <= 4 for an
 * 8-channel input (S2N's condition -- the image input), as the workspace query does.
 * op: 0 forward, 1 data gradient, 2 weight gradient.  Returns SGG_EINVAL for a bad descriptor or op. */
typedef enum {
    SGG_ROUTE_REG = 1,                 /* reserved, never returned (the retired register-staged GEMM): keeps the numbers below in place */
    SGG_ROUTE_HALO3, SGG_ROUTE_S2HALO, SGG_ROUTE_S2N, SGG_ROUTE_N7, SGG_ROUTE_HALO_NARROW_IN, SGG_ROUTE_HALO_FWD,
    SGG_ROUTE_HALO_DGRAD_NARROW,
    SGG_ROUTE_GLDS_256x256, SGG_ROUTE_GLDS_256x128, SGG_ROUTE_GLDS_128x128, SGG_ROUTE_GLDS_128x64, SGG_ROUTE_GLDS_256x16,
    SGG_ROUTE_W7, SGG_ROUTE_HALO_WGRAD, SGG_ROUTE_W9, SGG_ROUTE_W9S, SGG_ROUTE_WGRAD_V2_ROWFAST, SGG_ROUTE_WGRAD_V2,
    SGG_ROUTE_WGRAD_128x128, SGG_ROUTE_WGRAD_128x64, SGG_ROUTE_WGRAD_128x16,
    SGG_ROUTE_SPLITK = 256             /* bit 8 */
} sgg_route;
int sgg_conv2d_route(const sgg_conv_desc* d, int op);
int sgg_deconv2d_route(const sgg_conv_desc* d, int op);

/* bias gradient: db[c] (+)= sum_p dy[p][c], c < C_real (f32).  ws >= sgg_bias_grad_workspace(P, C) bytes. */
size_t sgg_bias_grad_workspace(int64_t P, int C);
int sgg_bias_grad(const void* dy, float* db, int64_t P, int C, int C_real, int accumulate, int dtype,
                  void* ws, size_t ws_bytes, void* stream);
/* grouped call (see sgg_conv2d_fwd_group2): dy holds two networks' tensors back to back, P pixels each; ws >= 2 x the single call's */
int sgg_bias_grad_group2(const void* dy, float* db, float* db2, int64_t P, int C, int C_real, int accumulate, int dtype,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- instance_norm: tfa.layers.InstanceNormalization ---- module.py:212,216,233,...,308 (spec by name: ops.py:13-22)
 * y = act(gamma*(x-mean)*rstd + beta) (+ residual, added AFTER act; module.py:217 uses act NONE).
 * stats[N][C][2] = (mean, rstd) f32 is written by fwd and read by bwd.
 * ws >= sgg_instnorm_workspace(N, HW, C) bytes. */
size_t sgg_instnorm_workspace(int N, int64_t HW, int C);
int sgg_instnorm_fwd(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                     float* stats, int N, int64_t HW, int C, float eps, int act, float leak, int dtype,
                     void* ws, size_t ws_bytes, void* stream);
/* same, with the statistics pass replaced by precomputed partial sums partial[N][chunks][C][2] (sgg_conv2d_fwd_stats) */
int sgg_instnorm_fwd_partial(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                             float* stats, const float* partial, int chunks, int N, int64_t HW, int C, float eps,
                             int act, float leak, int dtype, void* stream);
/* only the finalize step of the above: stats[N][C][2] = (mean, rstd) from the partial sums (no pass over the tensor) */
int sgg_instnorm_finalize(const float* partial, int chunks, float* stats, int N, int64_t HW, int C, float eps, void* stream);
/* dx = d/dx of the above given dy (w.r.t. the post-activation output); dgamma/dbeta[C_real] f32 overwritten or
 * (accumulate=1) added to.  gamma/beta/stats are indexed over the padded C. */
int sgg_instnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats,
                     void* dx, float* dgamma, float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate,
                     int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream);
/* the same for an F32 dy against bf16 x / dx (mixed mode, see sgg_conv2d_bwd_data_mixed) */
int sgg_instnorm_bwd_mixed(const float* dy, const void* x, const float* gamma, const float* beta, const float* stats, void* dx,
                           float* dgamma, float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak,
                           void* ws, size_t ws_bytes, void* stream);
/* same, with the statistics pass replaced by precomputed partial sums partial[N][chunks][C][2] (sgg_conv2d_bwd_data_stats);
 * ws >= N*C*4 floats */
int sgg_instnorm_bwd_partial(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats, void* dx,
                             float* dgamma, float* dbeta, const float* partial, int chunks, int N, int64_t HW, int C, int C_real,
                             int accumulate, int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream);

/* Skip added BEFORE the activation (generator_unet d3 / d7, module.py:181-184,199-202): y = act(gamma*xhat + beta + skip),
 * act RELU / LRELU / NONE.  Same stats layout and workspace as sgg_instnorm_fwd; the _partial form takes the conv epilogue's
 * partial sums like sgg_instnorm_fwd_partial.
 * Backward: given dy and the stored output y, dskip = dy * act'(y) (the skip path's gradient: written once, by the statistics
 * pass; it may alias dy), dx = the norm's input gradient for dskip, dgamma/dbeta as sgg_instnorm_bwd.  Deterministic. */
int sgg_instnorm_fwd_skip(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* stats,
                          int N, int64_t HW, int C, float eps, int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream);
int sgg_instnorm_fwd_skip_partial(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* stats,
                                  const float* partial, int chunks, int N, int64_t HW, int C, float eps, int act, float leak, int dtype,
                                  void* stream);
int sgg_instnorm_bwd_skip(const void* dy, const void* y, const void* x, const float* gamma, const float* beta, const float* stats,
                          void* dx, void* dskip, float* dgamma, float* dbeta, int N, int64_t HW, int C, int C_real, int accumulate,
                          int act, float leak, int dtype, void* ws, size_t ws_bytes, void* stream);

/* Two networks of the same shape in lockstep on ONE stacked batch (the cycle step's G_A->B / G_B->A and D_A / D_B pairs,
 * model.py:114-133 applied to both translation directions): images 0..nsplit-1 belong to the first network (gamma, beta,
 * dgamma, dbeta), images nsplit..N-1 to the second (gamma2, ...).  Instance norm is per image, so one launch over the 2x larger
 * tensor serves both -- same arithmetic per image as two separate calls (bit-identical), at a higher fraction of HBM bandwidth
 * and half the launches. */
int sgg_instnorm_fwd_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                          const void* residual, void* y, float* stats, int N, int64_t HW, int C, float eps, int act, float leak,
                          int dtype, void* ws, size_t ws_bytes, void* stream);
int sgg_instnorm_fwd_partial_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                                  const void* residual, void* y, float* stats, const float* partial, int chunks, int N, int64_t HW, int C,
                                  float eps, int act, float leak, int dtype, void* stream);
int sgg_instnorm_bwd_pair(const void* dy, const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                          int nsplit, const float* stats, void* dx, float* dgamma, float* dbeta, float* dgamma2, float* dbeta2,
                          int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak, int dtype,
                          void* ws, size_t ws_bytes, void* stream);

/* The skip-before-activation norm of two networks in lockstep (the U-Net generators of the cycle step): arguments as
 * sgg_instnorm_*_skip plus the second network's parameter set, picked by image index as in sgg_instnorm_*_pair.  Workspace and
 * stats layout are those of the single forms; per image the arithmetic and summation order are theirs too, so each half of
 * the stacked result is bit for bit what sgg_instnorm_*_skip gives on that half alone. */
int sgg_instnorm_fwd_skip_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                               const void* skip, void* y, float* stats, int N, int64_t HW, int C, float eps, int act, float leak,
                               int dtype, void* ws, size_t ws_bytes, void* stream);
int sgg_instnorm_fwd_skip_partial_pair(const void* x, const float* gamma, const float* beta, const float* gamma2, const float* beta2, int nsplit,
                                       const void* skip, void* y, float* stats, const float* partial, int chunks, int N, int64_t HW, int C,
                                       float eps, int act, float leak, int dtype, void* stream);
int sgg_instnorm_bwd_skip_pair(const void* dy, const void* y, const void* x, const float* gamma, const float* beta, const float* gamma2,
                               const float* beta2, int nsplit, const float* stats, void* dx, void* dskip, float* dgamma, float* dbeta,
                               float* dgamma2, float* dbeta2, int N, int64_t HW, int C, int C_real, int accumulate, int act, float leak,
                               int dtype, void* ws, size_t ws_bytes, void* stream);

/* ---- lrelu / relu / tanh: tf.keras.layers.LeakyReLU / Activation ---- module.py:213,265,285 (ops.py:36-37) */
int sgg_act_fwd(const void* x, void* y, int64_t n, int act, float leak, int dtype, void* stream);
/* dx = dy * act'(.) evaluated from the OUTPUT y (relu/lrelu: sign of y; tanh: 1-y^2). */
int sgg_act_bwd(const void* dy, const void* y, void* dx, int64_t n, int act, float leak, int dtype, void* stream);
/* out = a + b (residual join of gradients). */
int sgg_add(const void* a, const void* b, void* out, int64_t n, int dtype, void* stream);

/* ---- semantic mask over the adversarial map ---- module.py:312-314
 * out[n,i,j] = sum_{c<C_real} h4[n,i',j',c] * mask[n,i,j,c];  h4 is (N,hh,hw,Cpad) in dtype, mask (N,mh,mw,C_real) f32;
 * (hh,hw) == (mh,mw), or (1,1) broadcast over the mask grid (the 128x128 reference case).  out f32 (N,mh,mw). */
int sgg_mask_reduce_fwd(const void* h4, const float* mask, float* out, int N, int hh, int hw, int mh, int mw,
                        int C_real, int Cpad, int dtype, void* stream);
int sgg_mask_reduce_bwd(const float* dout, const float* mask, void* dh4, int N, int hh, int hw, int mh, int mw,
                        int C_real, int Cpad, int dtype, void* stream);

/* ---- losses ---- model.py:149-166
 * BCE-with-logits against a constant label, global mean:  *loss (+)= weight*mean(...);
 * dlogits[i] (+)= weight*gscale*(sigmoid(x_i)-label)/n.  accumulate bit0: add into *loss; bit1: add into dlogits. */
int sgg_bce_logits(const float* logits, int64_t n, float label, float weight, float gscale, float* loss, float* dlogits,
                   int accumulate, void* stream);
/* L1 (abs_criterion, module.py:336-337): *loss (+)= weight*mean_{p,c<C_real}|a-b|;  db (+)= -weight*gscale*sign(a-b)/(P*C_real)
 * (0 in padded channels).  accumulate bit0: add into *loss; bit1: add into db. */
int sgg_l1_loss(const void* a, const void* b, int64_t P, int C_real, int Cpad, float weight, float gscale, float* loss,
                void* db, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
size_t sgg_l1_loss_workspace(int64_t P, int Cpad);

/* ---- defined-not-wired SG-GAN criteria, used by the cycle-mode step ----
 * LSGAN criterion against a constant target -- mae_criterion (module.py:340-341; squared error despite the name):
 *   *loss (+)= weight*mean((x-t)^2);  dx (+)= weight*gscale*2(x-t)/n.  accumulate bits as sgg_bce_logits. */
int sgg_mse_const(const float* x, int64_t n, float target, float weight, float gscale, float* loss, float* dx,
                  int accumulate, void* stream);
/* segmentation-edge indicator (model.py:108-119): 1 where the REFLECT-padded colour segmentation has a non-zero central
 * difference in x or y on any channel, else 0.  seg (N,H,W,Cpad) in dtype -> out f32 (N,H,W). */
int sgg_seg_edge_weight(const void* seg, float* out, int N, int H, int W, int C_real, int Cpad, int dtype, void* stream);
/* gradient-sensitive loss -- tf_deriv + gradloss_criterion (module.py:325-351): Sobel gx/gy (depthwise, SAME zero pad) of
 * `in` and `target`;  *loss (+)= lambda * mean_pixels( weight * mean_{2C}| |d(in)| - |d(target)| | );
 * din (+)= gscale * d(lambda*loss)/d(in) (NULL: loss only).  accumulate bit0: loss, bit1: din. */
size_t sgg_gradloss_workspace(int N, int H, int W, int C_real);
int sgg_gradloss(const void* in, const void* target, const float* weight, int N, int H, int W, int C_real, int Cpad,
                 float lambda, float gscale, float* loss, void* din, int accumulate, int dtype,
                 void* ws, size_t ws_bytes, void* stream);
/* structural-similarity loss (csrc/ssimloss.hip): sgg_image_quality's SSIM -- 11 x 11 separable Gaussian window,
 * sigma 1.5, the (H-10) * (W-10) windows wholly inside the image -- on the float values as they are, with its gradient.
 *   target, x: (N,H,W,Cpad) in dtype (SGG_F32 | SGG_BF16), Cpad == SGG_CPAD, 1 <= C_real <= Cpad, 16-byte aligned; target is a
 *   constant, x the differentiable operand.  Per image, channel c < C_real and window, with the window means ux (target), uy (x),
 *   exx, eyy, exy:  vx = exx - ux^2, vy = eyy - uy^2, vxy = exy - ux*uy,
 *     A1 = 2 ux uy + C1, A2 = 2 vxy + C2, B1 = ux^2 + uy^2 + C1, B2 = vx + vy + C2, S = A1 A2 / (B1 B2),
 *     C1 = (0.01 * data_range)^2, C2 = (0.03 * data_range)^2;       L = 1 - mean S.
 *   *loss (+)= weight * L, one rounding to f32 (accumulate bit 0: the old value is added before it).  Identical operands: S == 1
 *   exactly, so *loss == 0.0f with accumulate 0.
 *   dx (NULL: loss only, two launches instead of three): (N,H,W,Cpad) in dtype, 16-byte aligned, not x or target;
 *     dx (+)= gscale * weight * dL/dx, one rounding to dtype, where with Nw the number of (image, channel, window) triples
 *     alpha = (2ux A2 - 2ux A1)/(B1 B2) - 2 S uy / B1 + 2 S uy / B2,  beta = 2 A1 / (B1 B2),  gamma = -2 S / B2  per window and
 *     dL/dx[q] = -( (G^T alpha)[q] + target[q] (G^T beta)[q] + x[q] (G^T gamma)[q] ) / Nw,  G^T the adjoint of the valid filter.
 *     accumulate bit 1 clear: padded channels are written as 0; set: dx = round(dx + g), padded channels keep their bits.
 *   Moments, S, coefficients, both adjoint passes and the join are double, every sum in a fixed order (ssimloss.hip's header):
 *   equal operands give equal bits.  No atomics, no allocation, no host sync: capturable.
 *   ws: sgg_ssim_loss_workspace(N, H, W, C_real) bytes (0: the shape is not supported), 16-byte aligned; need not be initialised.
 * Refusals, before any launch and in this order: SGG_EINVAL (a NULL target, x, loss or ws; a misaligned buffer; dx aliasing x or
 * target; N <= 0; C_real outside [1, Cpad]; a dtype other than the two; data_range not finite or <= 0), SGG_EUNSUPPORTED
 * (Cpad != SGG_CPAD, H < 11, W < 11, H * W > 2^22, a grid past the launch limit), SGG_EWORKSPACE (ws_bytes too small). */
size_t sgg_ssim_loss_workspace(int N, int H, int W, int C_real);
int sgg_ssim_loss(const void* target, const void* x, int N, int H, int W, int C_real, int Cpad, float data_range, float weight,
                  float gscale, float* loss, void* dx, int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
/* feature-matching loss (csrc/featmatch.hip; Wang et al. 2018): L pairs of activations in ONE call.
 *   pairs: a HOST array of L entries, 1 <= L <= SGG_FM_MAX_PAIRS, read during the call only; real, fake, grad are device tensors
 *   (P, Cpad) in dtype (SGG_F32 | SGG_BF16), 16-byte aligned, Cpad % 8 == 0, 1 <= C_real <= Cpad, padded channels zero in both
 *   inputs.  real is a constant.  With count_i = P_i * C_real_i:
 *     term      = (1/L) * sum_i (1/count_i) * sum_{p, c < C_real_i} |fake_i - real_i|      -> *term (f32, always overwritten)
 *     *loss (+)= weight * term                                      (accumulate bit 0: the old value is added)
 *     grad_i    = (float)(weight / (L * count_i)) * sign(fake_i - real_i), sign(0) = 0 stored as +0, +0 in padded channels;
 *                 one rounding to dtype; always overwritten.
 *   d = (double)fake - (double)real is exact; |d| is added in double in a fixed order (featmatch.hip's header: lane-strided,
 *   a butterfly over the wave, the waves in order, the chunks of a layer in index order, the layers in order); term and the
 *   loss contribution are each one rounding of a double to f32.  Two launches whatever L is; the table travels in the kernel
 *   arguments: no copy, no atomics, no allocation, no host sync, bitwise reproducible, capturable.
 *   ws: sgg_feature_match_workspace(pairs, L, dtype) bytes (pointers are not read; 0: the arguments are refused), 8-byte aligned.
 * Before any launch, in this order -- SGG_EINVAL: NULL loss, term or pairs, L outside 1..SGG_FM_MAX_PAIRS, an unknown dtype, an
 *   entry with P <= 0, Cpad <= 0, Cpad % 8 != 0, C_real outside [1, Cpad], a NULL or misaligned pointer; SGG_EUNSUPPORTED: a layer of
 *   more than 2^31 - 1 sixteen-byte vectors; SGG_EWORKSPACE: ws NULL, misaligned or short. */
#define SGG_FM_MAX_PAIRS 8
typedef struct {
    const void* real;
    const void* fake;
    void* grad;
    int64_t P;
    int32_t C_real, Cpad;
} sgg_fm_pair;
size_t sgg_feature_match_workspace(const sgg_fm_pair* pairs, int L, int dtype);
int sgg_feature_match(const sgg_fm_pair* pairs, int L, float weight, float* loss, float* term, int accumulate, int dtype,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- optimizer: tf.keras.optimizers.Adam.apply_gradients ---- model.py:199-200,205-207
 * Keras form, over one flat f32 buffer:  m=b1*m+(1-b1)*g; v=b2*v+(1-b2)*g^2;
 * theta -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps);   g is first multiplied by grad_scale (1/world for DP). */
int sgg_adam(float* theta, const float* g, float* m, float* v, int64_t n, int t, float lr, float beta1, float beta2,
             float eps, float grad_scale, void* stream);
/* The same update with the step number kept on the DEVICE: `state` is int64[2] -- state[0] is the counterpart of Keras'
 * `optimizer.iterations` variable (t = state[0] + 1 is used and state[0] incremented), state[1] is scratch.  Two launches
 * (a 1-thread one that evaluates lr_t, then the update); no host-side step state, so the call can be captured into a HIP
 * graph and replayed (the eager per-op dispatch of model.py:168 is what this removes). */
int sgg_adam_iter(float* theta, const float* g, float* m, float* v, int64_t n, int64_t* state, float lr, float beta1,
                  float beta2, float eps, float grad_scale, void* stream);
/* sgg_adam_iter with the reference's linear learning-rate decay (model.py:223) evaluated by the 1-thread launch:
 * `sched` is int64[3] on the DEVICE = {steps_per_epoch, epoch_step, epochs}, read when the launch RUNS (it may be written
 * after the call was captured into a HIP graph).  With e = state[0] / steps_per_epoch (steps_per_epoch clamped to >= 1):
 *   lr_e = lr                                               if epochs <= epoch_step or e < epoch_step
 *   lr_e = (float)(lr * max(epochs - e, 0) / (epochs - epoch_step))   otherwise (in double, one rounding to f32);
 * the update is sgg_adam_iter's with lr_e in place of lr (bit-identical to it).  {1, 0, 0} never decays. */
int sgg_adam_sched(float* theta, const float* g, float* m, float* v, int64_t n, int64_t* state, const int64_t* sched,
                   float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* Guarded update (no counterpart in the reference): the global L2 norm of the gradient is measured on the
 * device, the gradient is clipped to max_norm, and an update whose gradient holds a NaN or +-Inf is skipped.
 *   sgg_grad_sumsq: one pass over g (16-byte aligned, any n > 0).  Every 8192-element chunk leaves a 16-byte record
 *     {double sum of squares, uint32 non-finite flag, 0} at ws + 16 + 16 * chunk; the flag tests the bit pattern (exponent
 *     all ones).  Fixed summation order, no atomics; the chunking depends on n only.
 *   sgg_adam_guard: that pass, a 1-block launch that folds the records in a fixed order and decides, then the update.
 *       norm = sqrt(sum) * grad_scale         (double)
 *       skip = any flag set
 *       clip = 1 if max_norm <= 0 or norm <= max_norm, else (float)(max_norm / norm)      (1 on skip)
 *     Not skipped: sgg_adam_sched's step (sched == NULL: sgg_adam_iter's) with g * (grad_scale * clip), the factor formed
 *     once in f32 -- with clip == 1 bit-identical to those calls.  Skipped: theta, m, v and state[0] keep their bits and
 *     the scratch rate is written as 0.  guard is double[4] on the DEVICE = {last_norm, last_clip, skipped_total,
 *     applied_total}, read and written by the launches only (the call can be captured; max_norm is a launch argument).
 *   ws: sgg_grad_guard_workspace(n) bytes, 16-byte aligned (its first 16 bytes carry the decision to the update launch);
 *   a smaller one returns SGG_EWORKSPACE before anything is launched; NULL pointers or n <= 0 return SGG_EINVAL. */
size_t sgg_grad_guard_workspace(int64_t n);
int sgg_grad_sumsq(const float* g, int64_t n, void* ws, size_t ws_bytes, void* stream);
int sgg_adam_guard(float* theta, const float* g, float* m, float* v, int64_t n, int64_t* state, const int64_t* sched,
                   float lr, float beta1, float beta2, float eps, float grad_scale, float max_norm, double* guard,
                   void* ws, size_t ws_bytes, void* stream);
/* The same updates keeping an exponential moving average of theta beside it, in the update's own launches:
 *   guarded == 0: sgg_adam_sched's launches (sched == NULL: sgg_adam_iter's); guard and ws may be NULL, max_norm is unused.
 *   guarded != 0: sgg_adam_guard's launches with its guard, ws and max_norm.
 * theta, m, v, state[0] (and guard[0..3]) come out bit-identical to those calls.  The prep launch also forms, with t =
 * state[0] AFTER this update's increment,
 *       d_t = (float)min((double)ema_decay, (1 + t) / (10 + t))       (tf.train.ExponentialMovingAverage with num_updates)
 * and writes ema_state = {d_t, 1.f - d_t} (float[2] on the DEVICE); the update launch then does, per element in f32,
 *       ema[i] = d_t * ema[i] + (1 - d_t) * theta_new[i].
 * A skipped step leaves ema and ema_state with their bits, like theta, m and v; t counts applied updates.  The update launch
 * moves 16 bytes per lane on all five streams: theta, g, m, v and ema must be 16-byte aligned; any n > 0 (scalar tail for
 * n % 4).  No atomics.  NULL pointers, n <= 0, a misaligned buffer or ema_decay outside (0, 1) return SGG_EINVAL, a short ws
 * with guarded SGG_EWORKSPACE -- before anything is launched. */
int sgg_adam_ema(float* theta, const float* g, float* m, float* v, float* ema, int64_t n, int64_t* state, const int64_t* sched,
                 float lr, float beta1, float beta2, float eps, float grad_scale, float ema_decay, float* ema_state,
                 float max_norm, int guarded, double* guard, void* ws, size_t ws_bytes, void* stream);
/* Exchange the contents of two n-element buffers (16-byte aligned, n > 0) bit for bit in one pass. */
int sgg_swap_f32(float* a, float* b, int64_t n, void* stream);

/* ---- spectral norm (no counterpart in the reference): Miyato et al. 2018 for every conv layer of a network, one
 * call per network over a DEVICE table of items (as sgg_pack_conv_weights_batch).  A layer's kernel is the matrix M (rows x K,
 * row-major f32: the HWIO kernel as it is stored, rows = R*S*C_real, K = K_real), u a persistent unit vector of length K.
 *   sgg_spectral_sigma, per item, every sum in double and in an order the shapes alone fix (no atomics; the same bits each run):
 *       t = M u            v = t / sqrt(max(|t|^2, 1e-12))
 *       s = Mt v           u' = s / sqrt(max(|s|^2, 1e-12))
 *     advance != 0: u <- u' in place, sigma = max(vt M u', 1e-12) (= |s|);  advance == 0: u keeps its bits and
 *     sigma = max(vt M u, 1e-12) (= |t|): the value a freshly built or loaded network starts from.  v[rows], sigma[0] and
 *     inv_sigma[0] = (float)(1 / sigma) (the division in double) are written as f32, each rounded once.  Three launches (two
 *     with advance == 0): M is read once, by blocks that take SGG_SPECTRAL_BAND rows each and leave t and their share of Mt t and
 *     |t|^2 in ws; a block per item and 64 columns folds the shares (v, s); one block per item finishes u and sigma.  The launch
 *     shapes depend on (n_items, max_rows, max_K, advance) only: capturable.
 *   sgg_spectral_grad, per item, with dWbar = g as it comes in (the gradient with respect to Wbar = W * inv_sigma):
 *       lambda = (sum dWbar o W) * inv_sigma                  (double, fixed order)
 *       g <- (float)((dWbar - lambda * (v ut)) * inv_sigma)   (in double, one rounding), in place.
 *     u, v and inv_sigma are read as sgg_spectral_sigma left them: they are constants of the differentiation.
 *   max_rows / max_K: upper bounds of the items' rows / K (they size grid and workspace; an item above them, or with a NULL
 *   w / u / v / sigma / inv_sigma -- for sgg_spectral_grad also g -- is left untouched); K <= SGG_SPECTRAL_MAX_K.  w and g rows are read
 *   with 16-byte loads where K % 4 == 0 and the base is 16-byte aligned, with 4-byte loads otherwise: any K, any rows >= 1.
 *   ws: 8-byte aligned, the workspace query's bytes.  Status, before anything is launched: SGG_EINVAL -- items_dev NULL,
 *   n_items <= 0, max_rows <= 0, max_K outside 1..SGG_SPECTRAL_MAX_K; SGG_EWORKSPACE -- ws NULL, misaligned or short. */
#define SGG_SPECTRAL_BAND 32
#define SGG_SPECTRAL_MAX_K 1024
typedef struct sgg_spectral_item {
    const float* w;      /* M */
    float* g;            /* dWbar in, dW out (sgg_spectral_grad; sgg_spectral_sigma ignores it) */
    float* u;            /* K */
    float* v;            /* rows */
    float* sigma;        /* 1 */
    float* inv_sigma;    /* 1 */
    int32_t rows, K;
} sgg_spectral_item;
size_t sgg_spectral_sigma_workspace(int n_items, int max_rows, int max_K);
int sgg_spectral_sigma(const sgg_spectral_item* items_dev, int n_items, int max_rows, int max_K, int advance,
                       void* ws, size_t ws_bytes, void* stream);
size_t sgg_spectral_grad_workspace(int n_items, int max_rows);
int sgg_spectral_grad(const sgg_spectral_item* items_dev, int n_items, int max_rows, int max_K,
                      void* ws, size_t ws_bytes, void* stream);
/* sgg_pack_conv_weights_batch with item i's elements multiplied by scale_dev[i] (a DEVICE float per item, read when the launch
 * runs) in f32 before the single rounding to `dtype`: the same kernel body.  scale_dev NULL returns SGG_EINVAL. */
int sgg_pack_conv_weights_batch_scaled(const sgg_pack_item* items_dev, const float* scale_dev, int n_items, int64_t max_elems,
                                       int dtype, void* stream);

/* ---- data side of the step ----
 * segment_class.py:60-70,95-97: colour -> class index, bit exact.  rgb: uint8 [n_pixels][channels>=3]. */
int sgg_seg_class_map(const uint8_t* rgb, int channels, int64_t n_pixels, uint8_t* out, void* stream);
/* host-side copy of the kernel's colour table (keys = R<<16|G<<8|B); returns the entry count (21). No GPU needed. */
int sgg_seg_class_table(uint32_t* keys_host, uint8_t* vals_host, int capacity);
/* utils.py:158-165 + :197-199 (deviation D1): one-hot of the align-corners nearest resample of the
 * class-index map:  mask[n,i,j,c] = (idx[n, round(i*(H-1)/(oh-1)), round(j*(W-1)/(ow-1))] == c). */
int sgg_onehot_resample(const uint8_t* idx, float* mask, int N, int H, int W, int oh, int ow, int n_classes, void* stream);
/* ---- input pipeline: utils.load_train_data / load_test_data's imread -> resize (-> resize) -> fliplr (utils.py:116-233) over
 * device-resident uint8 sources.  The skimage resize chain is linear and separable; the caller folds it into one banded
 * matrix per axis (sggan_amd/data.py) and this applies
 *   out[n,i,j,c] = ( sum_kr row_w[i][kr] * ( sum_kc col_w[j'][kc] * src[index[n]][row_start[i]+kr][col_start[j']+kc][c] ) ) / 255,
 *   j' = flip[n] ? W-1-j : j,   c < C   (channels C..SGG_CPAD-1 of out are written as zeros),
 * f32 accumulation in that order (kc ascending, then kr ascending), independent of the launch geometry.
 *   src (M,H0,W0,Cs) uint8, Cs = 3 or 4;  index, flip: int32[N] on the DEVICE (the launch is the same every step: graph safe);
 *   row_w f32 [H][row_taps], row_start int32 [H] with 0 <= row_start[i] <= H0 - row_taps; col_* likewise over W / W0;
 *   col_step = the largest col_start[j+1] - col_start[j] (sizes the LDS window; coordinates are clamped inside the kernel,
 *   so tables that break these rules give wrong pixels, not out-of-range accesses);
 *   out (N,H,W,SGG_CPAD) in dtype -- the layout the networks read, so the step passes it through untouched.
 * No workspace.  SGG_EUNSUPPORTED: a tile's column window plus its weights exceed 64 KB of LDS. */
int sgg_resample_u8(const uint8_t* src, int M, int H0, int W0, int Cs, const int32_t* index, const int32_t* flip,
                    const float* row_w, const int32_t* row_start, int row_taps,
                    const float* col_w, const int32_t* col_start, int col_taps, int col_step,
                    void* out, int N, int H, int W, int C, int dtype, void* stream);
/* ---- augmented training copy (utils.py:80-103,180-182; deviation D6): Fliplr, Crop and Affine in a drawn order on
 * the squared image A = resize(src, (S, S)), S = H0, folded by the caller (sggan_amd/data.py: augment_matrices) into two 2x3
 * float64 maps per sample, row major, 12 doubles: `fill` (output point -> the affine's input frame) then `full` (-> A):
 *   p = (x + 0.5, y + 0.5);  out[n][y][x] = 0 where fill.p lies outside [0,S]x[0,S], else the bilinear sample (edge clamp) of
 *   A at full.p - 0.5, with A[y][x][c] = ( sum_k col_w[x][k] * src[index[n]][y][col_start[x] + k][c] ) / 255, c < 3.
 * Coordinates float64, each (m0*px + m1*py) + m2; f32 sums: taps ascending, then neighbours (y0,x0) (y0,x1) (y1,x0) (y1,x1).
 *   src (M,S,W0,Cs) uint8, Cs = 3 or 4 (the 4th source channel is not read); index int32[N], matrices double[N][12],
 *   col_w f32 [S][col_taps], col_start int32 [S] (band_table((W0, S))): all on the DEVICE, so the launch is the same every step;
 *   win_rows x win_cols: the pixels of A one 16 x 64 output tile can touch (data.warp_window), staged in LDS; coordinates are
 *   clamped to the window and the source, so wrong parameters give wrong pixels, not out-of-range accesses;
 *   out (N,S,S,4) f32, channel 3 = 0.  No workspace, no atomics.  SGG_EUNSUPPORTED: the window exceeds 64 KB of LDS. */
int sgg_warp_affine_u8(const uint8_t* src, int M, int S, int W0, int Cs, const int32_t* index, const double* matrices,
                       const float* col_w, const int32_t* col_start, int col_taps, int win_rows, int win_cols,
                       float* out, int N, void* stream);
/* sgg_resample_u8's band resample over an f32 source (N,H0,W0,4) (the warp's output): sample n -> output sample n, values
 * taken as they are (no / 255), the same summation order; c < C <= 4, channels C..SGG_CPAD-1 written as zeros.  Output sample
 * n starts out_stride elements after sample n-1 (>= H*W*SGG_CPAD, a multiple of SGG_CPAD): the copies of a doubled batch are
 * written between its plain samples.  SGG_EUNSUPPORTED: a tile's column window plus its weights exceed 64 KB of LDS. */
int sgg_resample_f32(const float* src, int N, int H0, int W0, const int32_t* flip,
                     const float* row_w, const int32_t* row_start, int row_taps,
                     const float* col_w, const int32_t* col_start, int col_taps, int col_step,
                     void* out, int64_t out_stride, int H, int W, int C, int dtype, void* stream);
/* ---- evaluation (next-row SURVEY 8(f)4): metric._fast_hist (metric.py:18-24) and scores_seg_fake (metric.py:71-77), bit exact
 * hist[n_class*t + p] += 1 for pixels with 0 <= t,p < n_class (uint64 counts, caller zeroes);
 * labels[i] = argmax_c uint8(255*x[i][c]) over the first C_real channels (first maximum wins). */
int sgg_confusion_hist(const int32_t* label_true, const int32_t* label_pred, int64_t n, int n_class, uint64_t* hist, void* stream);
int sgg_argmax_u8_labels(const void* x, int32_t* labels, int64_t P, int C_real, int Cpad, int dtype, void* stream);
/* ---- dense-CRF label refinement: metric.dense_crf (metric.py:49-69; pydensecrf's DenseCRF2D: unary_from_softmax,
 * addPairwiseGaussian(sxy = pos_xy_std, compat = pos_w), addPairwiseBilateral(sxy = bi_xy_std, srgb = bi_rgb_std, compat = bi_w),
 * Potts compatibility, NORMALIZE_SYMMETRIC, inference(max_iter)) with EXACT message passing over all (H*W)^2 pixel pairs
 * (pydensecrf filters through a permutohedral lattice).  The pairwise kernel is never stored.
 *   img (H,W,3) uint8;  exactly one of probs / unary is non-NULL, both (C,H,W) f32: probs -> U = -log(clip(p, 1e-5, 1)) taken
 *   in double and rounded once to f32, unary -> U as given;  q_out (C,H,W) f32 = the marginals after max_iter mean-field steps
 *   (0: softmax(-U)).  C <= 40, H*W <= 2^22 (else SGG_EUNSUPPORTED).  ws: sgg_dense_crf_workspace_bytes(H, W, C) bytes, 16-byte
 *   aligned; a smaller one returns SGG_EWORKSPACE before anything is launched.  Fixed summation order, no atomics: the same
 *   inputs give the same bits. */
size_t sgg_dense_crf_workspace_bytes(int H, int W, int C);
int sgg_dense_crf(const uint8_t* img, const float* probs, const float* unary, int H, int W, int C, int max_iter,
                  float pos_w, float pos_xy_std, float bi_w, float bi_xy_std, float bi_rgb_std, float* q_out,
                  void* ws, size_t ws_bytes, void* stream);
/* ---- class-level evaluation of generated segmentation maps (no counterpart in the reference) ----
 * A generated colour image is decoded to class labels through a palette of K entries {key = R<<16|G<<8|B, class}, 1 <= K <= 64,
 * given as HOST arrays and passed to the kernels by value (nothing is allocated or copied: the calls can be captured); both
 * NULL selects the library's built-in table (sgg_seg_class_table, K ignored).
 *   img: [n_pixels][cstride] of kind SGG_F32 / SGG_BF16 (cstride >= 3, the first three channels used; cstride = SGG_CPAD with a
 *        16-byte aligned base takes one 16-byte load per pixel) or SGG_U8 (cstride = 3 | 4; dword loads, four pixels per thread).
 *   colour: float input q_c = (int)(((x_c + 1.f) * 0.5f) * 255.f) in f32, clamped to 0..255, NaN -> 0 (utils.inverse_transform
 *        inside [-1,1]); uint8 input: the byte.   d2_k = sum_c (q_c - key_k.c)^2 (int32); the smallest wins, ties to the LOWEST k;
 *        label = class[k] if max_dist2 < 0 or d2 <= max_dist2, else other_class (0..255).
 * sgg_palette_decode -- outputs, each optional, at least one required:
 *   labels int32 [n_pixels];
 *   truth uint8 [n_pixels] + hist uint64 [n_class^2] (both or neither, 1 <= n_class <= 64): hist[n_class*t + p] += 1 for every
 *   pixel with t, p < n_class -- and, where select uint8 [n_pixels] is given, select != 0.  Counted in per-block LDS counters and
 *   added with 64-bit atomics: exact, order independent, accumulates into what hist holds.
 *   SGG_EINVAL before any launch: NULL img, K out of range, a key above 0xFFFFFF, other_class out of range, no output, truth
 *   without hist (or the reverse), select without hist, n_class out of range or <= a palette class.  n_pixels < 2^31.
 * sgg_palette_probs -- probs f32 (N, n_class, HW) from img (N, HW, cstride): with m_c = the smallest d2 over the entries of
 *   class c (other_class, where no entry names it and max_dist2 >= 0: the pseudo-distance max_dist2) and m_min = min_c m_c,
 *   e_c = exp(-(m_c - m_min) / (2 sigma^2)), classes with no distance e_c = 0, p = e / sum(e): the `probs` of sgg_dense_crf.
 *   Every palette class must be < n_class <= 64; sigma > 0.
 * sgg_class_boundary_band -- cls uint8 (N,H,W), 0 <= r <= 8: band[n,y,x] = 1 iff a pixel of image n with |dy|, |dx| <= r has a
 *   class other than cls[n,y,x], else 0 (r = 0: all zeros).  Nothing outside an image is read. */
int sgg_palette_decode(const void* img, int kind, int64_t n_pixels, int cstride, const uint32_t* keys_host,
                       const uint8_t* classes_host, int K, int other_class, int max_dist2, int32_t* labels,
                       const uint8_t* truth, const uint8_t* select, int n_class, uint64_t* hist, void* stream);
int sgg_palette_probs(const void* img, int kind, int N, int HW, int cstride, const uint32_t* keys_host,
                      const uint8_t* classes_host, int K, int other_class, int max_dist2, int n_class, float sigma,
                      float* probs, void* stream);
int sgg_class_boundary_band(const uint8_t* cls, uint8_t* band, int N, int H, int W, int r, void* stream);
/* ---- paired image-quality sums (no counterpart in the reference): MAE / PSNR / SSIM of a translation against
 * its target, both taken as 8-bit colour images.
 *   a, b: (N,H,W,cstride) images, the first three channels used, each of its own kind exactly as sgg_palette_decode takes them:
 *        SGG_F32 / SGG_BF16 (cstride >= 3; cstride = SGG_CPAD with a 16-byte aligned base takes one 16-byte load per pixel),
 *        quantised q = (int)(((x + 1.f) * 0.5f) * 255.f) in f32, clamped to 0..255, NaN -> 0; or SGG_U8 (cstride = 3 | 4), the byte.
 *   out double [N][3] on the DEVICE, written (not accumulated) per image n:
 *     out[n][0] = sum |a - b|, out[n][1] = sum (a - b)^2 over all H*W*3 values -- counted as integers (per-block sums, 64-bit
 *        adds, converted once): exact and independent of the grid;
 *     out[n][2] = sum over the three channels and the (H-10)*(W-10) windows wholly inside the image of the SSIM map
 *        S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = (0.01*255)^2, C2 = (0.03*255)^2, with the
 *        moments ux, uy, vx = E[xx] - ux^2, vy, vxy = E[xy] - ux uy under the separable 11 x 11 window w_k ~ exp(-k^2 / (2*1.5^2)),
 *        k = -5..5, normalised to sum 1 (scikit-image's structural_similarity with gaussian_weights=True, sigma=1.5,
 *        use_sample_covariance=False, data_range=255 -- [3P-recall]).  Moments, S and the sums are double; the weights are formed
 *        in double on the host; the order of every sum is fixed (no floating-point atomics): the same inputs give the same
 *        bits, image n of a batch the bits of the call on that image alone, identical operands exactly the window count.
 *   ws: sgg_image_quality_workspace(N, H, W) bytes (0: the shape is not supported), 8-byte aligned; need not be initialised.
 *   Two launches, nothing allocated, no host sync: the call can be captured.
 *   Before any launch -- SGG_EINVAL: NULL a / b / out / ws, a bad kind, cstride outside its kind's range, N <= 0, out or ws not
 *   8-byte aligned; SGG_EUNSUPPORTED: H < 11, W < 11 or H*W > 2^22 (or more than 2^31-1 tiles); SGG_EWORKSPACE: a short ws. */
size_t sgg_image_quality_workspace(int N, int H, int W);
int sgg_image_quality(const void* a, int kind_a, int cstride_a, const void* b, int kind_b, int cstride_b,
                      int N, int H, int W, double* out, void* ws, size_t ws_bytes, void* stream);
/* ---- differentiable augmentation of the discriminators' input (Zhao et al. 2020, policies colour + cutout) ----
 * x, y, dy, dx, addend: dtype [rows][H][W][Cpad], Cpad == SGG_CPAD, 16-byte aligned.  params: float [rows][8] on the DEVICE,
 * 16-byte aligned, one row [b, s, c, y0, x0, ch, cw, 0] per image.  With C = C_real, per pixel p = (y, x) and channel k < C, in f32:
 *     x1 = x + b;   m = (x1[p,0] + ... + x1[p,C-1]) / C;   x2 = x1 + (s - 1) * (x1 - m)
 *     M  = (float)(b + S / (C*H*W)),  S = the sum of x over the image's real channels, in double
 *     x3 = x2 + (c - 1) * (x2 - M);   y = 0 if y0 <= y < y0+ch and x0 <= x < x0+cw (a select), else x3
 *   sgg_diffaug_fwd writes y (out of place: y == x is SGG_EINVAL).  sgg_diffaug_bwd writes the adjoint for the gradient dy of y:
 *     g3 = 0 inside the rectangle, else dy;   Gs = the sum of g3 over the image's real channels, in double;   g2 = c * g3
 *     dx = g2 + (s - 1) * (g2 - mean_k g2[p,:]) + (float)((1 - c) * Gs / (C*H*W))  (+ addend[p,k] when addend != NULL)
 *   Padded channels of y and dx are written as 0.  The row [0, 1, 1, 0, 0, 0, 0, 0] reproduces the values of x (and of dy + addend).
 *   Two launches each (2048-pixel partial sums in a fixed order, then the apply pass, whose every block folds the image's
 *   partials again in the same order): no atomics, nothing allocated, no host sync, the same bits every run.
 *   ws: sgg_diffaug_workspace(rows, H, W) bytes (0: not supported), 8-byte aligned; need not be initialised.
 * sgg_diffaug_draw fills `rows` parameter rows from Philox4x32-10 (Random123's constants), ONE launch: key (seed, 0), counter
 *   (t_lo, t_hi, g, 4 * stream_id + j) with t = *iterations, int64 on the DEVICE and read when the launch RUNS (the call can be
 *   captured; a step counter that advances between replays gives new draws), g = (uint32)(sample_offset + row), j the draw block;
 *   u = (word >> 8) * 2^-24.  j = 0 (policy bit SGG_DIFFAUG_COLOR): b = (u0 - 0.5) * brightness, s = 2 * u1, c = u2 + 0.5, else
 *   b, s, c = 0, 1, 1.  j = 1 (SGG_DIFFAUG_CUTOUT): ch = H / 2, cw = W / 2, y0 = floor(u0 * (H + 1 - ch % 2)) - ch / 2 and x0
 *   likewise from u1 and W (f32 products), else y0 = x0 = ch = cw = 0.
 * Before any launch -- SGG_EINVAL: a NULL or misaligned buffer, rows / H / W <= 0, C_real outside 1..Cpad, a bad dtype, unknown
 *   policy bits, a negative stream_id or sample_offset; SGG_EUNSUPPORTED: Cpad != SGG_CPAD, H*W > 2^26, rows * ceil(H*W / 2048)
 *   >= 2^24 (a launch holds fewer than 2^32 threads, 256 per block); SGG_EWORKSPACE: a short ws. */
#define SGG_DIFFAUG_COLOR 1
#define SGG_DIFFAUG_CUTOUT 2
size_t sgg_diffaug_workspace(int rows, int H, int W);
int sgg_diffaug_draw(float* params, int rows, const int64_t* iterations, uint32_t seed, int64_t sample_offset, int stream_id,
                     int H, int W, int policy_bits, float brightness, void* stream);
int sgg_diffaug_fwd(const void* x, void* y, const float* params, int rows, int H, int W, int C_real, int Cpad, int dtype,
                    void* ws, size_t ws_bytes, void* stream);
int sgg_diffaug_bwd(const void* dy, const float* params, const void* addend, void* dx, int rows, int H, int W, int C_real,
                    int Cpad, int dtype, void* ws, size_t ws_bytes, void* stream);
/* ---- training-mode dropout: one in-place launch, used forward (y = m * scale * x) and backward (dx = m * scale * dy,
 * the same call on the gradient).  The mask is never stored: it is regenerated from counters.
 * x: dtype (SGG_F32 | SGG_BF16) [n_samples][elems_per_sample], modified in place; elems_per_sample a multiple of 8, the base
 *   16-byte aligned.  Element i of sample n belongs to vector e = i / 8 and lane j = i % 8:
 *     r = Philox4x32-10 (the constants of sgg_diffaug_draw), counter (t_lo, t_hi, g, e), key (seed, 1 + stream_id), with
 *         t = *iterations, int64 on the DEVICE and read when the launch RUNS (the call can be captured; a step counter that
 *         advances between replays gives new masks), g = (uint32)(sample_offset + n);
 *     d = (r[j >> 1] >> (16 * (j & 1))) & 0xFFFF;  the element is kept iff d >= threshold.
 *   Key word 1 is never 0, so no stream coincides with sgg_diffaug_draw's key (seed, 0).  The draw depends on the element index
 *   alone, never on dtype or launch shape: f32 and bf16 calls drop the same elements.
 *   threshold = round(rate * 65536) in 0..65535 (the caller's): the drop probability is exactly threshold / 65536.  Kept elements
 *   are multiplied by scale = 65536.f / (65536 - threshold) -- the product formed in f32 and rounded once to the storage type, to
 *   nearest even; rate 0.5 gives scale exactly 2 -- dropped ones become +0.  threshold = 0 keeps every bit of x (nothing is launched).
 *   One 16-byte load and one 16-byte store per vector, no LDS, no atomics, no workspace, no host sync: one launch.
 * Before any launch -- SGG_EINVAL: NULL x or iterations, a negative count, elems_per_sample % 8 != 0, a misaligned base, threshold
 *   outside 0..65535, stream_id outside 0..2^28-1, a negative sample_offset, an unknown dtype; SGG_EUNSUPPORTED: elems_per_sample
 *   > 2^35 (the vector index is a 32-bit counter word) or n_samples > 65535 (the grid's y extent).  n_samples == 0: SGG_OK, no launch. */
int sgg_dropout(void* x, int64_t n_samples, int64_t elems_per_sample, int threshold, const int64_t* iterations, uint32_t seed,
                int64_t sample_offset, int stream_id, int dtype, void* stream);
/* ---- fixed 2x resampling in front of a resize-convolution layer and its adjoint.  NHWC, padded channels.
 * sgg_upsample2x_fwd: x (N,H,W,Cp) -> y (N,2H,2W,Cp).  sgg_upsample2x_bwd: dy (N,2H,2W,Cp) -> dx (N,H,W,Cp) = U^T dy, the adjoint
 *   of the same linear map; N, H, W are the LOW-resolution extents in both.  in and out must not overlap.
 *   SGG_UPSAMPLE_NEAREST:  y[n,p,q,c] = x[n,p>>1,q>>1,c] -- a copy, output bits are input bits; adjoint: the sum of the 2x2 block,
 *     ((d[2i][2j] + d[2i][2j+1]) + d[2i+1][2j]) + d[2i+1][2j+1].
 *   SGG_UPSAMPLE_BILINEAR: half-pixel centres (tf.image.resize, torch align_corners=False).  Per axis of length n:
 *     y[2i] = 0.25 x[max(i-1,0)] + 0.75 x[i], y[2i+1] = 0.75 x[i] + 0.25 x[min(i+1,n-1)]; the 2-D operator is the tensor product
 *     (4 taps per output, weights 9/16, 3/16, 3/16, 1/16).  Adjoint per axis: dx[i] = sum_{k=-1..2} w_k dy[clamp(2i+k, 0, 2n-1)],
 *     w = (0.25, 0.75, 0.75, 0.25) -- the clamped taps are the border terms; 16 taps per result in 2-D.
 *   Arithmetic: f32.  acc = w_0 * v_0, then acc = acc + w_t * v_t over the taps in row-major order of their source offsets (a
 *   clamped tap keeps its place and weight), every product and sum rounded to f32, never contracted; w_t = row weight * column
 *   weight, exact.  One rounding to the storage type (bf16: to nearest even).  Gathers: a thread computes whole results -- no
 *   atomics, no workspace, one launch, bitwise reproducible, capturable.
 * Before any launch -- SGG_EINVAL: a NULL pointer, a negative extent, Cp % 8 != 0, a base that is not 16-byte aligned, an unknown
 *   mode or dtype (SGG_F32 | SGG_BF16); SGG_EUNSUPPORTED: N * H * W * Cp / 8 > 2^31 - 1 (the work-item index is 32-bit).  A zero
 *   extent: SGG_OK, no launch. */
typedef enum { SGG_UPSAMPLE_NEAREST = 0, SGG_UPSAMPLE_BILINEAR = 1 } sgg_upsample_mode;
int sgg_upsample2x_fwd(const void* x, void* y, int N, int H, int W, int Cp, int mode, int dtype, void* stream);
int sgg_upsample2x_bwd(const void* dy, void* dx, int N, int H, int W, int Cp, int mode, int dtype, void* stream);
/* ---- sliced Wasserstein distance of Laplacian-pyramid patches (Karras et al. 2018, section 5; the semantics of
 * PGGAN's metrics/sliced_wasserstein.py [3P-recall]): an unpaired realism score of two image sets.  The sort between
 * sgg_swd_project and sgg_swd_distance is the caller's.
 * sgg_swd_pyramid: img (N,H,W,cstride), the first three channels taken as 8-bit colours exactly as sgg_image_quality takes them
 *   (SGG_U8 with cstride 3 | 4, the byte; SGG_F32 / SGG_BF16 with cstride >= 3, q = (int)(((x + 1.f) * 0.5f) * 255.f) in f32 clamped
 *   to 0..255, NaN -> 0; cstride = SGG_CPAD with a 16-byte aligned base takes one 16-byte load per pixel).  With t = [1,4,6,4,1]/16
 *   and the mirror border without edge repeat (index -1 -> 1, n -> n-2):
 *     G_0 = the image;  G_k = down(G_{k-1}): filter with t (x) t, keep every second row and column starting at 0;
 *     up(x): Z[2i,2j] = x[i,j], other entries 0, filtered with 4 (t (x) t) under the same mirror rule applied to Z;
 *     Lap_{k-1} = G_{k-1} - up(G_k),  Lap_{levels-1} = G_{levels-1}.
 *   pyr: float per image sgg_swd_pyramid_elems(H, W, levels) values, the levels concatenated finest first, each planar
 *   [3][H >> l][W >> l].  The Gaussian chain lives in ws as double; with 8-bit inputs every intermediate is an exact dyadic
 *   rational of at most 47 bits (8 per down, 6 for up), so no sum depends on its order and the float store is the one rounding:
 *   image n of a batch gets the bits of the call on that image alone.  2 * levels launches.
 *   ws: sgg_swd_pyramid_workspace(N, H, W, levels) bytes, 8-byte aligned; need not be initialised.
 * sgg_swd_descriptors: rows [(i * patches + p)][147] of desc, float: the 7x7x3 patch of level `level` of image i around
 *   (cy, cx), flattened (channel, y, x).  cy = 3 + mulhi32(w_y, h - 6), cx = 3 + mulhi32(w_x, w - 6) with h, w the level's size and
 *   mulhi32(a, b) = ((uint64)a * b) >> 32; the words are Philox4x32-10 (the constants of sgg_diffaug_draw) with key (seed, 1) and
 *   counter (g, level, p / 2, 0), g = (uint32)(image_offset + i): words 0, 1 are (w_y, w_x) of patch 2 (p / 2), words 2, 3 those of
 *   patch 2 (p / 2) + 1.  desc points at the first row of this batch inside the set-wide buffer.  One launch.
 * sgg_swd_project: desc [M][147] -> moments double [3][2] = per colour channel (mean, population standard deviation) over all
 *   M * 49 values of the channel (the sum, then the sum of squared deviations from the mean: 256-row partials in double, folded in
 *   index order), and proj double [D][M], proj[d][m] = sum_k z_k dirs[k][d], k ascending, z_k = (desc[m][k] - mean_c) / std_c in
 *   double, 0 where std_c == 0.  dirs: float [147][D].  Five launches.  ws: sgg_swd_project_workspace(M) bytes, 8-byte aligned.
 * sgg_swd_distance: sa, sb double [D][M] (each row sorted by the caller) -> out[d] = sum_m |sa[d][m] - sb[d][m]|, double, thread
 *   t of the row's block takes m = t, t + 256, ..., then a fixed tree.  One launch.
 * All sums have a fixed order (no floating-point atomics), nothing is allocated, no host sync: every call can be captured.
 * Before any launch -- SGG_EINVAL: a NULL or misaligned buffer, a bad kind, cstride outside its kind's range, N / patches / M / D
 *   <= 0, level outside 0..levels-1, a negative image_offset; SGG_EUNSUPPORTED: levels outside 1..5, H or W not divisible by
 *   2^(levels-1), a coarsest level under 7x7, H*W > 2^22, a grid past the launch limits (more than 21845 images in a pyramid call,
 *   65535 in a descriptor call); SGG_EWORKSPACE: a short ws.  The size functions return 0 for unsupported shapes. */
size_t sgg_swd_pyramid_elems(int H, int W, int levels);
size_t sgg_swd_pyramid_workspace(int N, int H, int W, int levels);
size_t sgg_swd_project_workspace(int64_t M);
int sgg_swd_pyramid(const void* img, int kind, int cstride, int N, int H, int W, int levels, float* pyr, void* ws,
                    size_t ws_bytes, void* stream);
int sgg_swd_descriptors(const float* pyr, int N, int H, int W, int levels, int level, int patches, uint32_t seed,
                        int64_t image_offset, float* desc, void* stream);
int sgg_swd_project(const float* desc, int64_t M, const float* dirs, int D, double* proj, double* moments, void* ws,
                    size_t ws_bytes, void* stream);
int sgg_swd_distance(const double* sa, const double* sb, int D, int64_t M, double* out, void* stream);
/* f32 [P][Cs] -> dtype [P][Cd] with zero fill (Cd >= Cs), and back (drops padded channels). */
int sgg_pad_channels(const float* src, void* dst, int64_t P, int Cs, int Cd, int dtype, void* stream);
int sgg_unpad_channels(const void* src, float* dst, int64_t P, int Cs, int Cd, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGGAN_H */
