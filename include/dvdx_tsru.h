/*
 * dvdx_tsru.h -- C ABI of libdvdx_tsru.so: the pointwise part of the Transformation-based Spatial Recurrent Unit (TSRU_p of Luc et
 * al. 2020, "Transformation-based Adversarial Video Prediction on Large-Scale Data") -- warp the previous state by a predicted
 * flow, blend it with new content -- forward and backward.  The first library of the EXTENSION family (dvd_gan_amd/xsrc/<key>/,
 * include/dvdx_<key>.h, libdvdx_<key>.so, entry points dvdx_<key>_*, constants DVDX_<KEY>_*; dvd_gan_amd/lib.py EXTENSIONS): same
 * conventions as the dvdgan_hip family -- plain C, device pointers + sizes, asynchronous on `stream` (a hipStream_t passed as
 * void*), never synchronises, return value 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.
 * No process-wide state.  Every argument is checked before anything touches the device (the checks need no device).
 *
 * Tensors are channels-last: pixel m = (b * H + y) * W + x of a [B][H][W][..] tensor.  `dtype` (DVD_F32 / DVD_BF16 of
 * dvdgan_hip.h) is the type of the pre-activations `a`, of their gradient `da`, of the state's copy `h_c` and of the flow gradient
 * `dtheta_raw` (the operands of convolutions); the state itself, the raw flow and every other gradient are fp32.  The raw flow of
 * pixel m is theta_raw[m * ldt + 0] (x) and [m * ldt + 1] (y): ldt = 8 reads a convolution's padded fp32 output as it is.
 * a_c(m, k) = a[m * lda + off_c + k], a_u(m, k) = a[m * lda + off_u + k].
 *
 * The expressions, exactly (contraction is off; T-mode functions are common.h's gate_sigmoid<T> / gate_tanh<T>: libm and an IEEE
 * divide for fp32, the hardware exponential and reciprocal for bf16):
 *   tx = d * tanh(theta_raw[m][0]),  ty = d * tanh(theta_raw[m][1])              the flow of pixel m, in pixels
 *   sx = (float)x + tx,  sy = (float)y + ty
 *   the pixel samples only when sx lies in (-1, W) and sy in (-1, H); else warped = 0 and it passes no gradient through the warp
 *   x0 = (int)floorf(sx), wx1 = sx - floorf(sx), wx0 = 1 - wx1                  (y likewise)
 *   w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1
 *   v(j, i) = h_prev[b][j][i][k] inside the frame, 0 outside
 *   warped = fmaf(w11, v(y0+1, x0+1), fmaf(w10, v(y0+1, x0), fmaf(w01, v(y0, x0+1), w00 * v(y0, x0))))
 *            and v(y0, x0) itself when wx1 == 0 and wy1 == 0 (a zero flow moves bits)
 *   u = sigmoid(a_u), c = max(a_c, 0)
 *   h = fmaf(u, warped - c, c)                                                   = u warped + (1 - u) c
 * Backward, given dh (= dh + dh2 where dh2 is given):
 *   da_u = ((dh * (warped - c)) * u) * (1 - u),   da_c = a_c > 0 ? dh * (1 - u) : 0,   g = dh * u
 *   ex(k) = fmaf(wy1, v(y0+1, x0+1) - v(y0+1, x0), wy0 * (v(y0, x0+1) - v(y0, x0)))          d warped / d sx
 *   ey(k) = fmaf(wx1, v(y0+1, x0+1) - v(y0, x0+1), wx0 * (v(y0+1, x0) - v(y0, x0)))          d warped / d sy
 *   dtheta_raw[m][0] = ((sum_k g(k) ex(k)) * d) * (1 - tanh(theta_raw[m][0])^2)              ([1] with ey; rounded to `dtype`)
 *   dh_prev[q][k] = (sum over the pixels p of the window |p - q|_inf <= ceil(d), line by line, within a line left to right,
 *                    acc = fmaf(w, g(p, k), acc) from 0, w = the forward's weight of q in p's cell) [+ addend[q][k]]
 * The channel sum of dtheta: a group of G = min(64, the power of two >= C / 8) neighbouring lanes owns a pixel, lane j adds the
 * channels of the 8-channel vectors j, j + G, ... in ascending order with fmaf, and the lanes are summed by a butterfly of xor
 * shuffles (offsets G/2 .. 1).  |t| <= d makes the window of the transpose exact.  No atomics anywhere: every element has one
 * owner and a fixed order of summation, so two launches give the same bits, and a sample gives the same bits alone and in a batch.
 *
 * Launch shape: flat grids over (pixel, 8-channel vector) -- never one workgroup per sample: the frames on the recurrent chain
 * are 4 x 4 to 32 x 32, and B workgroups would leave a 256-CU device idle behind B latencies.  Below 65536 threads a launch uses
 * one-wave workgroups, so that even a 4 x 4 frame spreads over as many CUs as it has waves.
 */
#ifndef DVDX_TSRU_H
#define DVDX_TSRU_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVDX_TSRU_ABI_VERSION 1
#define DVDX_TSRU_MAX_FLOW 8          /* largest d, in pixels */
#define DVDX_TSRU_MAX_SIDE 1024       /* largest H and W */
#define DVDX_TSRU_THREADS 256         /* threads of a workgroup of a large launch (64 for a small one) */

/* DVDX_TSRU_ABI_VERSION of the build */
int dvdx_tsru_abi_version(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvdx_tsru_strerror(int code);

/* h <- the unit's new state, h_c <- its copy in `dtype` (NULL: not wanted).  h_prev, h [B][H][W][C] fp32; a [B*H*W][lda] `dtype`;
 * theta_raw [B*H*W][ldt] fp32; h_c [B][H][W][C] `dtype`.  Nothing else is written.
 * DVD_E_ARG: a null h_prev / a / theta_raw / h, h == h_prev (the kernel gathers: in place is wrong), a dtype other than
 * DVD_F32 / DVD_BF16, B, H, W or C < 1, d outside (0, DVDX_TSRU_MAX_FLOW] (a NaN too), a negative offset, ldt < 2.
 * DVD_E_SHAPE: C, lda, off_c or off_u no multiple of 8, a channel window that leaves the row (off + C > lda), H or W above
 * DVDX_TSRU_MAX_SIDE, B * H * W * C above 2^31 - 1. */
int dvdx_tsru_forward(int dtype, const float* h_prev, const void* a, int lda, int off_c, int off_u, const float* theta_raw, int ldt,
                      float d, float* h, void* h_c, int B, int H, int W, int C, void* stream);

/* The backward pass of dvdx_tsru_forward on the same operands, two launches.  dh, and dh2 (or NULL), [B][H][W][C] fp32: the
 * state's gradient is their sum (the warp's and the convolutions' share of a step of the time chain).  da [B*H*W][ldda] `dtype`
 * receives da_c at column doff_c and da_u at column doff_u; dtheta_raw [B*H*W][lddt] `dtype`, of which columns 0 and 1 are written
 * (lddt = 8 with the other columns zero is a convolution's operand); dh_prev [B][H][W][C] fp32; addend (fp32,
 * as dh_prev, or NULL) is added to dh_prev; ws: B * H * W * (C + 2) floats of scratch (g [B*H*W][C], then the flow [B*H*W][2]).
 * Refusals as the forward's, with dh, da, dtheta_raw, dh_prev, ws among the pointers, ldda / doff_c / doff_u among the strides
 * and offsets (lddt < 2 as ldt < 2), and dh_prev == dh, dh2 or h_prev among the aliases. */
int dvdx_tsru_backward(int dtype, const float* dh, const float* dh2, const float* h_prev, const void* a, int lda, int off_c, int off_u,
                       const float* theta_raw, int ldt, float d, void* da, int ldda, int doff_c, int doff_u, void* dtheta_raw,
                       int lddt, const float* addend, float* dh_prev, float* ws, int B, int H, int W, int C, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
