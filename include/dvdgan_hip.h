/*
 * dvdgan_hip.h -- C ABI of libdvdgan_hip.so, the MI355X (gfx950) hot path of the DVD-GAN
 * G + D_s + D_t training step.
 *
 * The reference (Harrypotterrrr/DVD-GAN) has no FFI layer: its hot path is torch ATen calls made
 * from nn.Module.forward.  Each entry point below therefore names the reference call site(s)
 * whose vendor kernel it replaces (file:line under /root/reference).  Conventions:
 *   - plain C: device pointers + sizes, no torch types; every call is asynchronous on `stream`
 *     (a hipStream_t passed as void*), never synchronises the device.  Process-wide state is limited to three
 *     caches / debug aids that never change a result: the split-K plan cache of the ConvGRU wavefront (keyed by the
 *     launch geometry, mutex-protected), the optional profiling hooks (dvd_prof_*) and the dvd_debug_* counters;
 *   - return value: 0 = ok, <0 = DVD_E_* (bad argument / unsupported shape / launch failure);
 *   - activations are channels-last: [frames][T][H][W][C] with C padded to a multiple of 8,
 *     row stride `ld*` in ELEMENTS; spatial extents H, W: powers of two take the fast kernels (LDS-staged footprints,
 *     shift indexing), any other extent (latent_dim 3, 6, ... of Generator.py:15) the tap-by-tap kernels with division indexing;
 *   - `dtype` selects the STORAGE / MFMA operand type of activations and packed weights:
 *     DVD_F32 (exact mode, v_mfma_f32_32x32x2_f32) or DVD_BF16 (v_mfma_f32_32x32x16_bf16);
 *     accumulation, statistics, master weights, gradients of weights are always fp32.
 */
#ifndef DVDGAN_HIP_H
#define DVDGAN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVD_F32 0
#define DVD_BF16 1

#define DVD_OK 0
#define DVD_E_ARG (-1)      /* null pointer / non-positive size                                */
#define DVD_E_SHAPE (-2)    /* unsupported shape (C % 8, even kernel, odd extent under a x2 upsample ...) */
#define DVD_E_LAUNCH (-3)   /* hipGetLastError() != hipSuccess after a launch                  */

#define DVD_ACT_NONE 0
#define DVD_ACT_RELU 1
#define DVD_ACT_TANH 2
#define DVD_ACT_SIGMOID 3

int dvd_abi_version(void);              /* bumps when a signature changes                      */
/* Layout handshake: sizeof() of descriptor struct `which` AS THIS LIBRARY WAS COMPILED (0 = dvd_conv_desc, 1 = dvd_wgrad_desc,
 * 2 = dvd_gru_desc, 3 = dvd_sn_item, 4 = dvd_gru_stack_desc, 5 = dvd_pack_item, 6 = dvd_frag_item; -1 = unknown index).  A binding compares it with the size of its own
 * mirror of the struct at load time (dvd_gan_amd/lib.py does; tests/test_abi_cpu.py also checks the stub printed in
 * INTEGRATION.md): a descriptor that grew on one side only is caught before the library reads past the caller's struct.
 * The reference boundary these structs stand in for is the nn.Module constructor / forward argument lists
 * (Module/Generator.py:15, Module/Discriminators.py:219,371). */
#define DVD_STRUCT_CONV 0
#define DVD_STRUCT_WGRAD 1
#define DVD_STRUCT_GRU 2
#define DVD_STRUCT_SN_ITEM 3
#define DVD_STRUCT_GRU_STACK 4
#define DVD_STRUCT_PACK_ITEM 5
#define DVD_STRUCT_FRAG_ITEM 6
int dvd_struct_size(int which);
/* Optional measurement aid for bench.py: bracket every conv launch with HIP events on its stream.
 * kind 0 = conv_igemm (forward / backward-data), 1 = conv_wgrad.  Report drains the records,
 * returns the launch count, total milliseconds and total algorithmic FLOPs (2*M*Cout*C*taps). */
void dvd_prof_enable(int on);
long long dvd_prof_report(int kind, double* total_ms, double* total_flops);
/* The same, split by kernel variant: n / ms / flops are arrays of nvar entries (or NULL); entry 0 = all launches of `kind`,
 * kind 0: 1 = conv_halo 256x128 tile, 2 = conv_halo 128x128, 3 = conv_halo 256x64, 4 = conv_igemm 128x128,
 * 5 = conv_igemm 256x128, 6 = conv_igemm 256x256, 7 / 8 = whole-frame footprint kernel (4x4 / 8x8 frames) 256x128 / 128x128,
 * 9 = thin-input kernel (3 -> 64 channels); kind 1: 1 = filter-row kernel (8-wave tiles), 2 = one-tap kernel, 3 = thin-end kernel,
 * 4 = filter-row kernel, one wave per SIMD. */
long long dvd_prof_report_variants(int kind, int nvar, long long* n, double* ms, double* flops);
const char* dvd_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution, stride 1, "same" zero padding, 1-D/2-D/3-D taps (kt,kh,kw odd).
 *   out[m][co] = epilogue( sum_{tap,ci} in[pos(m)+tap][ci] * w[tap][co][ci] )
 * Replaces F.conv2d / F.conv3d issued by nn.Conv2d / nn.Conv3d at
 *   Module/ConvGRU.py:49-51 (gate convs, split into x-part and h-part),
 *   Module/GResBlock.py:57,64,73, Module/Generator.py:114 (colorize),
 *   Module/Discriminators.py:186-206 (GBlock), :335-366 (Res3dBlock), :221-226,:376-382 (stems),
 *   :94-96 (q/k/v 1x1), and -- run on the flipped/transposed pack -- their backward-data passes.
 * Also fuses: ReLU on the input (GResBlock.py:52,62 / Discriminators.py:186,192), nearest x2
 * upsample of the input (GResBlock.py:55,72) or of the residual, bias, residual add (GResBlock.py:80), ReLU/tanh
 * on the output (Generator.py:113-115), ReLU-mask of a backward-data result.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int dtype;                 /* DVD_F32 | DVD_BF16                                            */
    int frames, T, H, W;       /* OUTPUT grid; M = frames*T*H*W rows. T>1 only for 3-D convs.   */
    int C, ldi;                /* input channels (multiple of 8) and input row stride           */
    int Cout, ldo;             /* output channels, output row stride                            */
    int kt, kh, kw;            /* taps                                                          */
    int up2;                   /* 1: input stored at H/2 x W/2, nearest-upsampled while loading */
    int relu_in;               /* 1: max(x,0) applied to the input while loading                */
    int nsplit;                /* K is cut in nsplit slices (grid.z); >1 requires `ws`          */
    int act;                   /* DVD_ACT_* (direct epilogue only)                              */
    int out_f32;               /* direct epilogue stores fp32 instead of `dtype`                */
    int ldres, ldmask;         /* row strides of res / mask                                     */
    int res_up2;               /* 1: res is stored at H/2 x W/2 ([frames*T][H/2][W/2][ldres]) and read through a
                                  nearest x2 upsample -- the 1x1 shortcut of GResBlock.py:72-73 commutes with the
                                  upsample, so it runs on the small grid and is expanded here                  */
    const void* in;            /* [rows_in][ldi]                                                */
    const void* w;             /* packed [ntaps][Cout][C] (see dvd_pack_conv_weight)            */
    const float* bias;         /* [Cout] or NULL                                                */
    const void* res;           /* [M][ldres] added before act, or NULL                          */
    const void* mask;          /* [M][ldmask]: result multiplied by (mask > 0), or NULL         */
    void* out;                 /* [M][ldo]                                                      */
    float* ws;                 /* non-NULL: raw fp32 partial sums [nsplit][M][Cout] are written
                                  here INSTEAD of the direct epilogue (bias/res/act/mask/out)   */
    const void* wq;            /* optional (bf16): the same weights as `w` in fragment-major order
                                  (dvd_conv_fragment_major); requests for which
                                  dvd_conv_wants_fragment_major() is 1 then read their weight operand
                                  straight from L2 into registers instead of staging it in LDS       */
    int wq_kind;               /* what `wq` holds: 0 / 1 = the fragment-major image, 2 = dvd_conv_thin_image, 3 = dvd_conv_thin_out_image
                                  (the value dvd_conv_wants_fragment_major returned for this request) */
    int pool2;                 /* ABI 12: != 0 -> `out` (and `mask`) live on the HALF-size grid [frames][H/2][W/2][ldo] and receive the
                                  2 x 2 SUMS of the convolution result -- the transpose of a nearest x2 upsample, i.e. the input gradient
                                  of a convolution that read an upsampled input (GResBlock.py:57-58) -- formed on the fp32 accumulators
                                  in the epilogue instead of by a dvd_pool pass over a full-size intermediate.  Served by the
                                  halo-staged kernels only: ask dvd_conv_pool2_ok() first.                                   */
} dvd_conv_desc;
int dvd_conv_forward(const dvd_conv_desc* d, void* stream);
/* 1 when dvd_conv_forward serves `d` with d->pool2 set (square 3 / 5 taps, power-of-two frames >= 16 pixels, one K slice,
 * no residual / activation / ConvGRU epilogue), else 0 (the caller runs the plain request and dvd_pool).  A geometry query: the
 * buffer pointers of `d` (in, w, out) are not looked at, `ws` only as "set or not". */
int dvd_conv_pool2_ok(const dvd_conv_desc* d);
/* Fragment-major weight image: [tap][32-channel chunk][32-column block, padded to whole 128-column tiles][k-half pair][lane]
 * [8 channels] -- 1 KiB per MFMA B fragment, fetched by one coalesced 16-byte load per lane.  `w`: a forward or backward-data
 * pack of dvd_pack_conv_weight ([ntaps][Cout][C], bf16, C % 8 == 0).  Re-run after every re-pack (spectral norm: every forward). */
long long dvd_conv_fragment_major_bytes(int ntaps, int Cout, int C);
int dvd_conv_fragment_major(int dtype, const void* w, void* wq, int ntaps, int Cout, int C, void* stream);
/* n images in one launch per 32 items (ABI 13; `items`: HOST array, copied into the kernel arguments): the packs of a whole ConvGRU. */
typedef struct { const void* w; void* wq; int ntaps, Cout, C; } dvd_frag_item;
int dvd_conv_fragment_major_batched(int dtype, const dvd_frag_item* items, int n, void* stream);
int dvd_conv_wants_fragment_major(const dvd_conv_desc* d);     /* 0 = no (also d == NULL), 1 = fragment-major image, 2 / 3 = the thin-input / thin-output image below;
                                                                  a geometry query as dvd_conv_pool2_ok: in / w / out / wq / wq_kind are not looked at */
/* 3 x 3 (x 3) convolutions from 3 (padded to 8) input channels to 64 output channels (the discriminator stems, the backward-data
 * pass of the RGB layer) fold their KW taps into the K dimension; they take, in `wq`, this image of their [kt*9][64][8] pack:
 * [tap row][k half][channel block][lane][8] (ABI 10). */
long long dvd_conv_thin_image_bytes(int kt);
int dvd_conv_thin_image(const void* w, void* wt, int kt, void* stream);
/* ... and 3 x 3 convolutions from 64 to at most 8 output channels (the RGB layer, the spatial stem's backward-data pass; wants = 3)
 * this image of their [9][rows][64] pack (rows = output rows present in the pack, <= 8): [tap][16-channel step][lane][8] */
long long dvd_conv_thin_out_image_bytes(void);
int dvd_conv_thin_out_image(const void* w, void* wt, int rows, void* stream);

/* Backward-weight of the same convolution:
 *   dw[co*s_co + ci*s_ci + tap*s_tap] += sum_m dy[m][co] * x[pos(m)+tap][ci]       (fp32 atomics)
 * for co < Cout, ci < Cin_real.  With s_co = Cin_real*ntaps, s_ci = ntaps, s_tap = 1 this is the
 * reference nn.Conv{2,3}d .weight.grad layout [co][ci][kt][kh][kw] (autograd of the sites above). */
typedef struct {
    int dtype;
    int frames, T, H, W;       /* grid of dy (= output grid of the forward conv)                */
    int C, ldx;                /* padded channels of x (multiple of 8), row stride              */
    int Cin_real;              /* only ci < Cin_real is written                                  */
    int Cout, Cy, ldy;         /* real out channels, padded channels present in dy, row stride  */
    int kt, kh, kw;
    int up2, relu_in;          /* same meaning as in dvd_conv_desc (applied to x)               */
    int msplit;                /* row range is cut in msplit slices (grid.z); >=1               */
    long long s_co, s_ci, s_tap;
    const void* x;
    const void* dy;
    float* dw;
    float* dbias;              /* optional: dbias[co] += sum_m dy[m][co] (bias gradient, fused: the workgroups of a
                                  channel tile already stream every dy row and take the 32-row steps in turn; with
                                  `ws` their partial sums go through the workspace and are added in a fixed order,
                                  without it the centre-tap workgroups add with atomics), co < Cout; NULL = skip */
    float* ws;                 /* optional workspace of dvd_conv_wgrad_ws_floats(d) floats: row slices write
                                  their partial tiles there with plain stores and a second kernel reduces
                                  them into dw (deterministic, no atomics).  NULL = fp32 atomics on dw.
                                  With a workspace, 3 x 3 layers over a x2-upsampled input (up2, GResBlock.py:57-58) whose
                                  Cout is a multiple of 64 are worked on the INPUT grid (four dy phases as output channels,
                                  2 / 3 of the products; same bf16 products, another fp32 summation order); without one
                                  they take the direct x2 tiles                                              */
    int overwrite;             /* 1: dw = result instead of dw += result (dense [co][ci][tap] dw only): no zero fill by the caller */
} dvd_wgrad_desc;
int dvd_conv_wgrad(const dvd_wgrad_desc* d, void* stream);
long long dvd_conv_wgrad_ws_floats(const dvd_wgrad_desc* d);   /* 0 = no workspace needed (single slice) */

/* fp32 master weight [Cout][Cin][ntaps] (reference layout) -> the two operand packs:
 *   wf[tap][co][ci_pad]          forward            (Cin padded with zeros to Cip, multiple of 8)
 *   wd[flip(tap)][ci_pad][co_pad] backward-data     (Cout padded to Cop, multiple of 8)
 * every element divided by *sigma when sigma != NULL (spectral norm, Normalization.py:30-31).
 * co_off/co_tot place this weight as rows [co_off, co_off+Cout) of a wider fused pack
 * (e.g. update|reset|out gates, q|k|v): wf row length stays Cip, wd row length is co_tot. */
int dvd_pack_conv_weight(int dtype, const float* w, const float* sigma, int Cout, int Cin, int ntaps,
                         int Cip, int co_off, int co_tot_f, int co_tot_d, void* wf, void* wd,
                         int kt, int kh, int kw, int ci_off, int ci_tot, void* stream);
/* ci_off/ci_tot: the master tensor is [Cout][ci_tot][ntaps] and only input channels
 * [ci_off, ci_off+Cin) are packed (x-part / h-part of a ConvGRU gate, ConvGRU.py:16-18). */
/* The same for n requests in ONE launch per 24 items (ABI 13): the x-part / h-part packs of the three gates of every layer of a
 * ConvGRU (Module/ConvGRU.py:16-18, :104-133: 18 fills per three-layer ConvGRU) were 18 launches of ~18 us in front of its first
 * convolution.  `items` is a HOST array (copied into the kernel arguments); fields as the arguments of dvd_pack_conv_weight. */
typedef struct {
    const float* w; const float* sigma; void* wf; void* wd;
    int Cout, Cin, ntaps, Cip, co_off, co_tot_f, co_tot_d, kt, kh, kw, ci_off, ci_tot;
} dvd_pack_item;
int dvd_pack_conv_weight_batched(int dtype, const dvd_pack_item* items, int n, void* stream);

/* Layout / dtype conversion at the module boundary (reference tensors are NCHW-style fp32):
 *   to_cl:   src fp32 [F][C][P]  -> dst [F][P][Cp]  (pad channels zero-filled)
 *   from_cl: src      [F][P][Cp] -> dst fp32 [F][C][P]
 * F = frames (arbitrary leading dims), P = spatial positions per frame.  `f_outer/f_inner` let the
 * frame index be permuted on the way: src frame (a,b) of an [A][B] grid <-> dst frame (b,a) when
 * swap_ab != 0 (b-major reference frames <-> t-major internal frames, Generator.py:103-106). */
int dvd_to_channels_last(int dtype, const float* src, void* dst, long long F, int C, long long P,
                         int Cp, int A, int B, int swap_ab, void* stream);
int dvd_from_channels_last(int dtype, const void* src, float* dst, long long F, int C, long long P,
                           int Cp, int A, int B, int swap_ab, void* stream);
/* dst[i] = (dst type)src[i], n elements (any n: eight per thread, then a scalar tail); src / dst dtype given separately
 * (fp32 -> bf16 rounds to nearest even).  No scaling and no accumulation: dst is overwritten. */
int dvd_convert(int src_dtype, const void* src, int dst_dtype, void* dst, long long n, void* stream);


/* ------------------------------------------------------------------------------------------
 * ConvGRU layer, serial half (Module/ConvGRU.py:29-54 for ONE layer, all T steps; the T loop of
 * Module/Generator.py:87-97 runs inside the library).  The caller supplies the batched x-path
 * pre-activations gx[t] = Wx * x_t + b (columns u|r|o, 3*hidden) and receives h_t plus the
 * tensors BPTT needs.  Backward fills dg[t] = d loss / d pre-activation (u|r|o) for every step;
 * weight and input gradients are then batched over T with dvd_conv_wgrad / dvd_conv_forward.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int dtype;
    int T, B, H, W;            /* steps, batch, spatial grid: M = B*H*W rows per step            */
    int hidden, k;             /* hidden channels (multiple of 8), square kernel size            */
    long long gx_stride;       /* elements between gx[t] and gx[t+1]; 0 = same gx for every t    */
    const void* gx;            /* [T|1][M][3*hidden]                                            */
    const void* w_ur;          /* forward pack  [k*k][2*hidden][hidden]  (update|reset, h-part)  */
    const void* w_o;           /* forward pack  [k*k][hidden][hidden]    (out gate, h-part)      */
    const void* wd_ur;         /* backward-data pack [k*k][hidden][2*hidden]                     */
    const void* wd_o;          /* backward-data pack [k*k][hidden][hidden]                       */
    const void* h0;            /* optional initial state [M][hidden] (ConvGRU.py:104), or NULL   */
    void* h_all; void* u_all; void* r_all; void* o_all; void* hr_all;   /* each [T][M][hidden]   */
    float* h32;                /* optional fp32 carry of h, [2][M][hidden] (bf16 mode), or NULL  */
    float* ws;                 /* split-K workspace, see dvd_convgru_ws_floats                   */
    /* backward only */
    const void* dh_out;        /* [T][M][hidden] gradient wrt every h_t, or NULL                 */
    void* dg;                  /* out [T][M][3*hidden]                                           */
    float* carry;              /* scratch [M][hidden] fp32                                       */
    float* dh0;                /* optional out [M][hidden] fp32: gradient wrt h0                 */
    /* forward only */
    int infer;                 /* 1 (sampling path, trainer.py:323-334: no backward will follow): u_all / hr_all are ONE-step
                                  scratch buffers [M][hidden], r and o are not stored (r_all, o_all may be NULL)           */
    /* optional: the four packs once more in fragment-major order (dvd_conv_fragment_major), or NULL -- handed to the recurrent
       convolutions as dvd_conv_desc.wq */
    const void* w_ur_q; const void* w_o_q; const void* wd_ur_q; const void* wd_o_q;
    /* optional (ABI 10): DVD_GRU_TICKETS zero-initialised counters.  When given, a split-K recurrent convolution sums its slices
       and applies the gate math INSIDE the launch (the last workgroup of an output tile to finish does it; nobody waits) instead
       of leaving fp32 slabs to a separate gate kernel: two launches per step and pass instead of four.  Every launch leaves the
       counters at zero; one buffer serves all layers issued on one stream, launches on different streams need their own.
       NULL = slabs + gate kernels (ABI 9 behaviour). */
    unsigned* tickets;
    int combine_max;           /* largest split-K factor combined in-launch; 0 = the library's measured default (4: beyond that the
                                  gate kernel, which spreads the slab reads over the whole chip, is faster)                       */
    int ns_cap;                /* > 0: upper bound on the split-K factor of the recurrent convolutions (tests: the same factors in
                                  the layer-by-layer and the wavefront path -> bit-equal results); 0 = the measured policy        */
} dvd_gru_desc;
#define DVD_GRU_TICKETS 8192
int dvd_convgru_layer_forward(const dvd_gru_desc* d, void* stream);
int dvd_convgru_layer_backward(const dvd_gru_desc* d, void* stream);
/* floats the caller provides as dvd_gru_desc.ws for a layer of this shape (slabs of whole output tiles) */
long long dvd_convgru_ws_floats(int dtype, int B, int H, int W, int hidden, int k);
int dvd_conv_pick_nsplit(int dtype, long long M, int Cout, int C, int ntaps);

/* ------------------------------------------------------------------------------------------
 * A whole ConvGRU (Module/ConvGRU.py:57-133: n_layers chained cells, layer l's input at step t = layer l-1's new state)
 * as a LAYER WAVEFRONT: layer l works on step t while layer l-1 works on step t + 2, so the recurrent convolutions of all
 * layers -- and the x-part convolutions of the layers above the first, now one per step -- are independent of each other
 * and run as GROUPED launches (several convolutions in one grid, their tiles interleaved).  A one-round launch of one
 * layer runs its workgroups in lock step (main loops, then the HBM-bound gate epilogues, overlapping with nothing); in a
 * grouped launch one tile's epilogue runs under another's main loop and the 4 x 4 / 8 x 8 stages issue 2 instead of 6-12
 * dependent launches per step.  Results equal dvd_convgru_layer_* applied layer by layer (bit-equal when the split-K
 * factors are the same: `layer_policy`).  bf16, square power-of-two frames of 4, 8 or >= 16 pixels, 3 x 3 / 5 x 5 filters,
 * fragment-major weight images required, and no grouped launch of the stack's schedule may need more than six members (four
 * layers in steady state: 4 gate + 3 x-part convolutions in one launch on 4, 16 and 32 pixel frames -- not served; on 8 x 8 frames,
 * or for sequences too short to fill the pipeline, they are).  dvd_convgru_stack_ok() says whether a stack is served -- it
 * records the schedule the launch would play and needs no workspace; dvd_convgru_stack_ws_floats() answers 0 and both passes
 * return DVD_E_SHAPE before any launch for a stack it refuses.  Callers fall back to the per-layer entry points otherwise.
 * ---------------------------------------------------------------------------------------- */
#define DVD_GRU_STACK_MAX 4
typedef struct {
    int n_layers;                                   /* 1 .. DVD_GRU_STACK_MAX                                          */
    int layer_policy;                               /* 0: split-K factors chosen per grouped launch; 1: dvd_conv_pick_nsplit per
                                                       convolution, x-part unsplit (the per-layer path's arithmetic, for tests) */
    int run;                                        /* tiles per pattern entry of a grouped launch; 0 = default           */
    int cin[DVD_GRU_STACK_MAX];                     /* stored (padded) input channels of layer l's x-part; l >= 1: hidden of l-1 */
    dvd_gru_desc layer[DVD_GRU_STACK_MAX];          /* as for dvd_convgru_layer_*: same dtype, T, B, H, W in every layer.
                                                       layer[l >= 1].gx ([T][M][3 hidden_l], gx_stride = M * 3 hidden_l) is
                                                       WRITTEN by the forward call; layer[l].ws is not used (`ws` below);
                                                       layer[0].tickets serves the whole stack; backward: layer[n-1].dh_out =
                                                       gradient wrt the top layer's states, layer[l < n-1].dh_out = optional
                                                       gradient wrt that layer's states from outside the stack, or NULL        */
    const void* wx[DVD_GRU_STACK_MAX];              /* l >= 1: x-part forward pack [k*k][3 hidden_l][cin_l] ...               */
    const void* wx_q[DVD_GRU_STACK_MAX];            /* ... its fragment-major image ...                                      */
    const float* bx[DVD_GRU_STACK_MAX];             /* ... and bias [3 hidden_l] (update | reset | out)                      */
    const void* wdx[DVD_GRU_STACK_MAX];             /* backward, l >= 1: x-part backward-data pack [k*k][cin_l][3 hidden_l]   */
    const void* wdx_q[DVD_GRU_STACK_MAX];           /* ... its fragment-major image                                          */
    void* dh_mid[DVD_GRU_STACK_MAX];                /* backward, l >= 1: out [T][M][cin_l] = gradient reaching layer l-1's states
                                                       (x-path of layer l + layer[l-1].dh_out)                               */
    float* ws;                                      /* dvd_convgru_stack_ws_floats(d) floats (split-K slabs of the grouped launches) */
} dvd_gru_stack_desc;
int dvd_convgru_stack_ok(const dvd_gru_stack_desc* d, int backward);
long long dvd_convgru_stack_ws_floats(const dvd_gru_stack_desc* d);
int dvd_convgru_stack_forward(const dvd_gru_stack_desc* d, void* stream);
int dvd_convgru_stack_backward(const dvd_gru_stack_desc* d, void* stream);
/* Test hook (tests/test_gpu_gru_stack.py): out[0] = floats the last dvd_convgru_stack_ws_floats call asked for (0 when no
 * member of any grouped launch is split), out[1] = the largest slab cursor any LAUNCHED group has used since the last reset;
 * reset != 0 clears out[1] afterwards.  After one forward + backward of a stack the two must be equal. */
void dvd_debug_stack_ws(long long* out, int reset);

/* ------------------------------------------------------------------------------------------
 * Batch norm statistics + conditional batch norm (Module/Normalization.py:78-88; F.batch_norm +
 * F.linear + mul/add).  `samp[frame]` = row of the condition matrix used by that frame (this
 * is where the reference's condition mis-ordering, Generator.py:109-110, is expressed).
 * gb = Linear(cond) as [B][2*C] (gamma | beta), computed with dvd_linear_forward.
 * ---------------------------------------------------------------------------------------- */
#define DVD_BN_NREP 16      /* copies of the [2C] sums the statistics kernel spreads its atomics over (dvd_bn_finalize adds them up) */
int dvd_bn_stats(int dtype, const void* x, long long rows, int C, int ld, double* sums /*[DVD_BN_NREP][2C], zeroed*/, void* stream);
int dvd_bn_finalize(double* sums /* read, then reset to zero when `rezero`: a persistent workspace needs no fill per call */,
                    long long rows, int C, float eps, float momentum, int training,
                    float* mean, float* rstd, float* run_mean, float* run_var, int rezero, void* stream);
int dvd_cbn_apply(int dtype, const void* x, void* y, long long frames, int P, int C, int ld, const float* mean,
                  const float* rstd, const float* gb, const int* samp, int relu, void* stream);
/* g: gradient wrt the (ReLU'd) output, x: CBN input.  Produces dx and accumulates dgb[B][2C] (zeroed by the caller);
 * s12[2C] is scratch.  a (the stored output) is NOT read and may be NULL: with relu the mask is re-evaluated from x by the
 * same fused multiply-add the forward used (two HBM passes fewer than reading it). */
int dvd_cbn_backward(int dtype, const void* g, const void* a, const void* x, void* dx, long long frames, int P,
                     int C, int ld, const float* mean, const float* rstd, const float* gb, const int* samp, int B,
                     float* dgb, float* s12, int relu, float* part, void* stream);
/* `part`: optional workspace of dvd_cbn_backward_ws_floats() floats -- the per-(frame, pixel chunk) partial sums of dgb are written
 * there and added per condition row in frame order (run-to-run reproducible); NULL = fp32 atomics straight into dgb. */
long long dvd_cbn_backward_ws_floats(long long frames, int P, int C);
/* The same in two stages, for cross-replica batch norm (the reference leaves it as a TODO, Generator.py:57; autograd of
 * F.batch_norm over a global batch): `reduce` accumulates dgb and writes the two per-channel sums s12[2C]; the caller
 * all-reduces s12 over the replicas; `apply` produces dx with rows_total = frames * P summed over the replicas.
 * dvd_cbn_backward == reduce + apply with rows_total = frames * P. */
int dvd_cbn_backward_reduce(int dtype, const void* g, const void* a, const void* x, long long frames, int P, int C, int ld,
                            const float* mean, const float* rstd, const float* gb, const int* samp, int B, float* dgb,
                            float* s12, int relu, float* part, void* stream);
int dvd_cbn_backward_apply(int dtype, const void* g, const void* a, const void* x, void* dx, long long frames, int P, int C,
                           int ld, const float* mean, const float* rstd, const float* gb, const int* samp, const float* s12,
                           long long rows_total, int relu, void* stream);

/* avg / sum pooling over (pt,2,2) windows and its transpose (nearest replication), channels-last.
 * F.avg_pool2d / F.avg_pool3d at Discriminators.py:197,206,225,249,352,361,380,408 and the
 * gradient of F.interpolate(scale_factor=2) (GResBlock.py:55,72). Output grid given; dvd_unpool writes zeros to the last
 * line / column of an odd output grid (the transpose of a floored pooling). */
int dvd_pool(int dtype, const void* x, void* y, long long frames, int To, int Ho, int Wo, int Hi, int Wi /* input grid: Hi/2 = Ho,
             Wi/2 = Wo; an odd extent loses its last line like F.avg_pool2d */, int ld, int pt, float scale, void* stream);
/* ... followed by a ReLU mask on the output grid (mask: same layout as y): the backward of relu -> nearest x2 -> conv
 * (GResBlock.py:52-57) in one pass instead of a pooling pass plus a masking pass */
int dvd_pool_masked(int dtype, const void* x, const void* mask, void* y, long long frames, int To, int Ho, int Wo, int ld, int pt,
                    float scale, void* stream);
int dvd_unpool(int dtype, const void* x, void* y, long long frames, int To, int Ho, int Wo, int ld, int pt, float scale, void* stream);
int dvd_colsum(int dtype, const void* x, long long rows, int C, int ld, float* out /* += */, void* stream);
int dvd_add(int dtype, const void* a, const void* b, void* out, long long n, void* stream);
int dvd_sum_leading(int dtype, const void* in /*[L][n]*/, void* out /*[n]*/, int L, long long n, void* stream);
int dvd_act_backward(int dtype, const void* dy, const void* y, void* dx, long long n, int act, void* stream);
/* utils.py:77-83 vid_downsample on reference-layout fp32 tensors (+ its backward) and
 * utils.py:60-63 frame gather: rows of L floats copied by index (scatter = transpose). */
int dvd_vid_downsample(const float* src, float* dst, int B, int T, int C, int H, int W, int backward, void* stream);
/* utils.py:77-83 vid_downsample of torch.cat([a, b], 1) without the concatenated clip (D_t's input of the frame-conditional
 * variant: context frames a [B][Ta][C][H][W] followed by generated frames b [B][Tb][C][H][W]).  Forward: dst =
 * [B][C][Ta+Tb][H/2][W/2], the same per-element arithmetic as dvd_vid_downsample.  Backward: the arguments name the same tensors'
 * gradients -- reads d(dst), writes d(b) into `b`; `a` is neither read nor written (may be null): context frames are data. */
int dvd_vid_downsample_cat(const float* a, int Ta, float* b, int Tb, float* dst, int B, int C, int H, int W, int backward,
                           void* stream);
int dvd_row_copy(const float* src, float* dst, const int* idx, long long nrows, long long L, int scatter, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spectral norm (Module/Normalization.py:19-31: mv, mv, norm, dot, div) and its backward
 *   dW_bar += G/sigma - (sum G*W_bar)/sigma^2 * u v^T        (u, v: CURRENT buffers, quirk 7)
 * ---------------------------------------------------------------------------------------- */
int dvd_sn_power_iter(const float* W, int h, int w, float* u, float* v, float* sigma, void* stream);
#define DVD_SN_SCRATCH 512   /* floats of dvd_sn_backward's `scratch`: per-block partial sums of sum G*W_bar, added in a fixed order (no atomics) */
int dvd_sn_backward(const float* G, const float* W, const float* u, const float* v, const float* sigma, int h, int w,
                    float* dW, float* scratch /*DVD_SN_SCRATCH floats*/, void* stream);
int dvd_sn_scale(const float* W, const float* sigma, float* out, long long n, void* stream);
/* The power iterations AND the sigma-normalised MFMA weight images of ALL spectrally normalised convolutions of a network in
 * four launches (the reference runs Normalization.py:19-31 inside every layer's forward): W^T u for every matrix,
 * W v, the finish step (norms, u, v, sigma), the two packs of dvd_pack_conv_weight (whole weight, co_off 0).  `host`: the n
 * items; `dev`: the same array in device memory (the caller uploads it AFTER dvd_sn_batched_prepare has filled the block
 * offsets and reported the scratch size).  wf / wd may be NULL (power iteration only). */
typedef struct {
    const float* W; float* u; float* v; float* sigma;      /* [h][w] fp32, [h], [w], [1]                                    */
    void* wf; void* wd;                                    /* packs [ntaps][cout][cip], [ntaps][cip][cop] in `dtype`, or NULL */
    int h, w;                                              /* matrix view: h = cout, w = cin * ntaps                         */
    int dtype, cout, cin, ntaps, cip, cop;
    int blk_wtu, blk_wv, blk_pack;                         /* first block of this item in the three batched launches (prepare) */
    int pad_;
} dvd_sn_item;
int dvd_sn_batched_prepare(dvd_sn_item* host, int n, long long* scratch_floats);
int dvd_sn_batched(const dvd_sn_item* host, const dvd_sn_item* dev, int n, float* scratch /* *scratch_floats floats */,
                   void* stream);

/* fp32 nn.Linear (Generator.py:75, Normalization.py:80) and nn.Embedding backward (Generator.py:70) */
int dvd_linear_forward(const float* in, const float* W, const float* bias, float* out, int B, int K, int J, void* stream);
int dvd_linear_backward(const float* dout, const float* in, const float* W, float* din, int din_accumulate,
                        float* dW /* += */, float* dbias /* += */, int B, int K, int J, void* stream);
int dvd_embedding_backward(const float* dout, const int* idx, float* dW /* += */, long long n, int D, void* stream);

/* Projection head (Discriminators.py:264-291 / 421-447): relu + spatial sum, SN linear + SN embed */
int dvd_relu_spatial_sum(int dtype, const void* feat, float* hsum, long long F, int P, int C, int ld, void* stream);
int dvd_relu_spatial_sum_backward(int dtype, const float* dh, const void* feat, void* dfeat, long long F, int P, int C,
                                  int ld, void* stream);
int dvd_proj_head_forward(const float* hsum, const float* wl, const float* sl, const float* bias, const float* emb,
                          const float* se, const int* cls, float* out, long long F, int C, void* stream);
int dvd_proj_head_backward(const float* dout, const float* hsum, const float* wl, const float* sl, const float* emb,
                           const float* se, const int* cls, float* dh, float* g_lin, float* g_emb, float* g_bias,
                           long long F, int C, void* stream);

/* Trainer.calc_loss (trainer.py:114-121): *loss += mean(...), dout = grad_scale * d mean / d out */
int dvd_adv_loss(const float* out, long long n, int hinge, int real_flag, float* loss, float* dout, float grad_scale,
                 void* stream);
/* torch.optim.Adam.step (trainer.py:252,268,306) on one flat fp32 buffer */
int dvd_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                  float eps, int step, void* stream);
/* Generator weight average (optim.FlatAdam(ema_decay > 0).step): dvd_adam_step's arithmetic, then
 * ema = decay * ema + (1 - decay) * p_new in the same launch; (1 - decay) is formed in double and rounded once, decay = 0 gives
 * ema == p_new bit for bit.  decay in [0, 1).  Any pointer alignment (16-byte aligned buffers take the vector path).
 * The five buffers must not overlap one another (not checked). */
int dvd_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float beta1,
                      float beta2, float eps, int step, float decay, void* stream);
/* The averaging line alone (callers that step their weights differently; tests/test_gpu_ema.py proves the fused form with it).
 * ema and p must not overlap (not checked). */
int dvd_ema_step(float* ema, const float* p, long long n, float decay, void* stream);
/* Exchange two fp32 buffers in place (Trainer.ema_weights: live weights <-> average around a sampling block).  a == b is a
 * no-op; buffers that overlap in part are not supported (not checked: both would be corrupted). */
int dvd_swap_f32(float* a, float* b, long long n, void* stream);

/* Gradient-norm clipping and non-finite step skipping on the device (no reference counterpart; optim.FlatAdam(clip_norm,
 * skip_nonfinite, norm_log).step; additions: the ABI version stays 13).  Two calls per step, both asynchronous, no hidden sync:
 *
 * dvd_grad_guard reads the flat fp32 gradient once (two launches, no atomics).  Workgroup w owns elements [w * DVD_GUARD_CH,
 * (w + 1) * DVD_GUARD_CH); which thread adds element i, and at which position of its order, depends on i and n only -- not on the
 * alignment of g (16-byte aligned buffers take vector loads, others the same assignment with scalar loads), not on the grid: the
 * result is bit-equal across alignments and reruns.  Each element enters as the exact fp64 product (double)x * (double)x; all
 * additions are fp64, in a fixed order (thread, xor shuffles within the wave, the four waves in order, then the per-workgroup
 * partials in a fixed order).  Elements whose exponent field is all ones (inf / NaN; an integer test on the bits) are counted and
 * left out of the sum.  Then
 *   norm = sqrt(S),  coef = min(1, (double)max_norm / (norm + 1e-6)),  coef32 = (float)coef     (torch's clip_grad_norm_;
 *   exactly 1 for max_norm = +inf: measure only),  skip = skip_nonfinite && bad > 0
 * and `state` (double[DVD_GUARD_STATE], zeroed by the caller before the first call, 8-byte aligned) receives
 *   [0] norm of the finite part   [1] coef32 (0.0 on a skipped step)   [2] bad = number of inf / NaN elements   [3] skip (0 / 1)
 *   [4] steps seen   [5] steps skipped   [6] steps clipped (coef32 < 1 and not skipped)   [7] 0     ([4..6] count calls).
 * ring != NULL with ring_rows = R > 0: row (step - 1) % R of the double[R][4] log receives step, norm, coef32, bad.
 * ws: dvd_grad_guard_ws_bytes(n) bytes, 8-byte aligned, written by every call: with W = ceil(n / DVD_GUARD_CH) workgroups,
 * double partial[W] (sum of squares of each chunk), double S (their sum, norm = sqrt(S)), unsigned bad[W] (counts per chunk).
 * DVD_E_ARG before any launch: g / ws / state null or state / ws not 8-byte aligned, n <= 0, step <= 0, max_norm NaN or <= 0,
 * ring_rows < 0, ring == NULL with ring_rows > 0.  dvd_grad_guard_ws_bytes(n <= 0) = 0.
 *
 * dvd_adam_guard_step is dvd_adam_ema_step (ema != NULL) or dvd_adam_step's arithmetic (ema == NULL) on g[i] * coef32 -- a product
 * rounded on its own, never fused; coef32 == 1 reproduces g[i], so the launch is then bit-equal to the unguarded one -- unless
 * state[3] says skip: then every workgroup returns without touching p, m, v or ema.  `step` is the caller's count (bias
 * correction): a skipped step is not taken back.  DVD_E_ARG: a null pointer other than ema, n <= 0, step <= 0, decay outside
 * [0, 1) when ema is given.  The buffers must not overlap one another (not checked). */
#define DVD_GUARD_CH 16384
#define DVD_GUARD_STATE 8
long long dvd_grad_guard_ws_bytes(long long n);
int dvd_grad_guard(const float* g, long long n, float max_norm, int skip_nonfinite, long long step, void* ws, double* state,
                   double* ring, int ring_rows, void* stream);
int dvd_adam_guard_step(float* p, const float* g, float* m, float* v, float* ema /* may be NULL */, long long n, float lr,
                        float beta1, float beta2, float eps, int step, float decay, const double* state, void* stream);

/* Prediction metrics (metrics.frame_metrics, Trainer.evaluate_prediction; additions: the ABI version stays 13): per-frame MSE and
 * SSIM of F = B * T predicted frames against target frames, C channels of H x W fp32 each, 11 <= H, W <= 256.  Each operand is a
 * base pointer with batch, time and channel strides in ELEMENTS; the H x W planes are contiguous (row stride W).  So `pred` can be
 * the generator's [B][T][C][H][W] and `target` the view [:, :, K:] of a loader clip [B][C][K+T][H][W], without a permuted copy.
 * mse[b * T + t] = mean over C * H * W of (p - t)^2.  ssim[b * T + t] = the mean SSIM index of Wang et al. 2004 over all
 * (H - 10) * (W - 10) "valid" windows and the C channels: 11 x 11 Gaussian window, sigma = 1.5, weights normalised to sum 1,
 * C1 = 0.01^2, C2 = 0.03^2 (L = 1), sigma_x^2 = E[x^2] - mu_x^2.
 * flags: DVD_METRICS_SIGNED = the operands are in [-1, 1]: x <- clamp((x + 1) / 2, 0, 1) on load; DVD_METRICS_QUANTIZE = after
 * that, x <- rint(255 x) / 255.  Unknown bits, sides outside [11, 256], C / T / B < 1: DVD_E_SHAPE, before any launch.
 * Deterministic: a frame's result depends on nothing but that frame's pixels (no atomics; fixed-order sums).  Any base alignment
 * (16-byte aligned planes with W % 4 == 0 take the vector loads).  `ws`: dvd_frame_metrics_ws_bytes bytes (currently 0: may be
 * null). */
#define DVD_METRICS_SIGNED 1
#define DVD_METRICS_QUANTIZE 2
#define DVD_METRICS_MIN_SIDE 11
#define DVD_METRICS_MAX_SIDE 256
long long dvd_frame_metrics_ws_bytes(long long B, int T, int C, int H, int W);
int dvd_frame_metrics(const float* pred, long long p_sb, long long p_st, long long p_sc, const float* target,
                      long long t_sb, long long t_st, long long t_sc, long long B, int T, int C, int H, int W, int flags,
                      float* mse, float* ssim, void* ws, void* stream);

/* Orthogonal regularization of weights (no reference counterpart; Brock et al. 2019, eq. 3; optim.FlatAdam(ortho = beta).step;
 * additions: the ABI version stays 13).  For every item i, a row-major fp32 matrix W_i = p + off_i viewed as [h_i][w_i]:
 *   M_i = W_i W_i^T with its diagonal set to exact zeros,  R(W_i) = 1/2 ||M_i||_F^2,  dR/dW_i = 2 M_i W_i,
 *   g[off_i ...] = fl(g + fl(s * (M_i W_i)))  with s = 2 * strength formed on the host: two roundings, never a fused multiply-add.
 * Both products run on v_mfma_f32_32x32x2_f32 (exact fp32).  The whole table takes two launches (all M_i, then all updates) and,
 * with `penalty` != NULL, a third that leaves *penalty = sum_i R(W_i), unscaled: fp32 elements of M squared and summed in fp64,
 * one slot per tile, the slots added in a fixed order.  No atomics: what an item receives depends on nothing else in the table,
 * and reruns are bit-equal.  Any h >= 1, w >= 1, any 4-byte aligned offsets; an item with h = 1 has an empty M and is skipped.
 * The table is `long long items[n][DVD_ORTHO_COLS]`: the caller fills DVD_ORTHO_OFF / _H / _W (offset in floats, the same in p and
 * g), dvd_ortho_prepare -- host only, no device needed -- fills the planner's columns (workspace offset of M_i, first block of the
 * item in either launch, and the launch order of the items: deepest products first), stores the workspace size in *ws_floats
 * (floats; the workspace must be 8-byte aligned) and returns the number of M tiles (>= 0) or DVD_E_ARG (null pointer, n < 1,
 * h < 1, w < 1, negative offset) / DVD_E_SHAPE (h > DVD_ORTHO_MAX_H, more than 2^31 - 1 blocks or 2^40 elements).
 * dvd_ortho_grad takes the prepared table twice, in host memory (checked against the planner before any launch: DVD_E_ARG when
 * it is not what dvd_ortho_prepare leaves) and in device memory (uploaded once by the caller).  strength must be finite and
 * >= 0.  p, g and ws must not overlap (not checked). */
#define DVD_ORTHO_COLS 8
#define DVD_ORTHO_OFF 0
#define DVD_ORTHO_H 1
#define DVD_ORTHO_W 2
#define DVD_ORTHO_WS 3        /* planner: offset of M_i [h][h] in the workspace, floats                          */
#define DVD_ORTHO_GRAM0 4     /* planner: first block of the item in the Gram launch                             */
#define DVD_ORTHO_APPLY0 5    /* planner: first block of the item in the apply launch                            */
#define DVD_ORTHO_GORDER 6    /* planner: row r holds the index of the item at rank r of the Gram launch         */
#define DVD_ORTHO_AORDER 7    /* planner: the same for the apply launch                                          */
#define DVD_ORTHO_MAX_H 32768
long long dvd_ortho_prepare(long long* items, int n, long long* ws_floats);
int dvd_ortho_grad(const float* p, float* g /* += */, const long long* items_host, const long long* items_dev, int n,
                   float strength, float* ws, double* penalty /* or NULL */, void* stream);

/* 2-D self attention (Discriminators.py:100-119: bmm, softmax, bmm, gamma*out + x) */
int dvd_attention_forward(int dtype, const void* qkv, int ldq, int dq, int koff, int voff, const void* x, int ldx, int C,
                          const float* gamma, void* y, void* att_out, float* A, long long frames, int N, void* stream);
int dvd_attention_backward(int dtype, const void* qkv, int ldq, int dq, int koff, int voff, const void* dy, int ldx,
                           int C, const float* gamma, const void* att_out, const float* A, float* dS, void* dqkv,
                           float* dgamma, long long frames, int N, void* stream);
/* The same block on the matrix cores (bf16 storage, ABI 10): nothing N x N is kept -- the forward leaves `lse` [frames][N]
 * (log-sum-exp of each query's score row), the backward recomputes the probabilities from q, k and lse; D is scratch
 * [frames][N].  q | k | v at columns 0 | 16 | 32 of qkv (16 query / key channels), C = 32 / 64 / 128 = ldx, N = 32 .. 4096 in
 * whole 32-token blocks: dvd_attention_mfma_ok says whether a call qualifies (everything else: the fp32 kernels above). */
int dvd_attention_mfma_ok(int dtype, int ldq, int dq, int koff, int voff, int ldx, int C, int N);
int dvd_attention_mfma_forward(const void* qkv, int ldq, const void* x, int C, const float* gamma, void* y, void* att_out,
                               float* lse, long long frames, int N, void* stream);
int dvd_attention_mfma_backward(const void* qkv, int ldq, const void* dy, int C, const float* gamma, const void* att_out,
                                const float* lse, float* D, void* dqkv /* every q | k | v column is written */,
                                float* dgamma /* += */, long long frames, int N, void* stream);

/* Spatio-temporal self attention (Module/Attention.py:114-185, SelfAttention over the T*H*W token axis; defined by the
 * reference, not invoked by its Generator): queries from `q` (N rows per clip), keys / values from `kv` -- the
 * 2x2x2 max-pooled projections, Nk = N/8 rows per clip, columns [koff,koff+dq) / [voff,voff+C); A is [frames][N][Nk].
 * softmax(q k^T) (:166-167), V A^T (:172), gamma*out + x (:179). */
int dvd_attention_kv_forward(int dtype, const void* q, int ldq, int dq, const void* kv, int ldk, int koff, int voff,
                             const void* x, int ldx, int C, const float* gamma, void* y, void* att_out, float* A,
                             long long frames, int N, int Nk, void* stream);
int dvd_attention_kv_backward(int dtype, const void* q, int ldq, int dq, const void* kv, int ldk, int koff, int voff,
                              const void* dy, int ldx, int C, const float* gamma, const void* att_out, const float* A,
                              float* dS, void* dq_out, void* dkv_out, float* dgamma, long long frames, int N, int Nk,
                              void* stream);
/* nn.MaxPool3d(kernel_size=2, stride=2) of Module/Attention.py:148,164,170 on a channels-last [frames][2To][2Ho][2Wo][ld]
 * tensor and its backward (gradient to the first maximum of each window) */
int dvd_maxpool3d(int dtype, const void* x, void* y, long long frames, int To, int Ho, int Wo, int ld, void* stream);
int dvd_maxpool3d_backward(int dtype, const void* x, const void* dy, void* dx, long long frames, int To, int Ho, int Wo,
                           int ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * SeparableAttnCell (Module/Attention.py:24-111; the T / W / H cells of SeparableAttn, :8-21): attention along ONE axis of a
 * [B, T, W, H, C] channels-last clip, built -- like the reference -- from raw reshapes of the contiguous NCDHW projections
 * (see csrc/sepattn.hip).  q | k | v are columns [0,Cq) | [koff,koff+Cq) | [voff,voff+C) of `qkv` (one fused 1x1 conv);
 * axis: 0 = T, 1 = W, 2 = H; T, W, H even; attended size A <= 64 (DVD_E_SHAPE otherwise: the score / gradient product tiles are
 * 64 x 32; n_frames > 64 or a 128-pixel attended axis is not served).  Every shape / scratch check runs BEFORE the first launch.
 * Work arrays are per call, sized by the caller:
 *   Qf [B][Cq*N], Kp [B][Cq*N/2], Vp [B][C*N/2] fp32, ksel / vsel bytes of the same counts (max-pool winners),
 *   att [B][A][A/2]   (N = T*W*H; dvd_sepattn_work_floats = floats of Qf + Kp + Vp + att per clip)
 * backward additionally: dO [B][C*N], dS like att, dQf / dKp / dVp like Qf / Kp / Vp; writes the q | k | v columns of dqkv
 * and ADDS to dgamma[1].  The residual path (dx += dy) and the 1x1 convolutions belong to the caller.
 * ---------------------------------------------------------------------------------------- */
long long dvd_sepattn_work_floats(int T, int W, int H, int axis, int C, int Cq);
int dvd_sepattn_forward(int dtype, const void* qkv, int ldq, int Cq, int koff, int voff, const void* x, int ldx, int C,
                        const float* gamma, void* y, float* Qf, float* Kp, float* Vp, unsigned char* ksel,
                        unsigned char* vsel, float* att, long long B, int T, int W, int H, int axis, void* stream);
int dvd_sepattn_backward(int dtype, const void* dy, int ldx, int C, int Cq, const float* gamma, const float* Qf,
                         const float* Kp, const float* Vp, const unsigned char* ksel, const unsigned char* vsel,
                         const float* att, float* dO, float* dS, float* dQf, float* dKp, float* dVp, void* dqkv, int ldq,
                         int koff, int voff, float* dgamma, long long B, int T, int W, int H, int axis, void* stream);

/* Real-data input (Dataloader/transform/spatial_transforms.py:38-122,253-268 after the host-side crop / resize): uint8 clips
 * [B][T][H][W][3] -> fp32 [B][3][T][H][W] = ((x / norm_value) - mean[c]) / std[c], clips with flip[b] != 0 mirrored
 * horizontally.  mean_std: device float[6] = mean RGB | std RGB. */
int dvd_clip_to_tensor(const unsigned char* src, const unsigned char* flip, float* dst, long long B, int T, int H, int W,
                       float norm_value, const float* mean_std, void* stream);

/* Device-resident clip store (data.ClipStore.gather; the whole per-step work of Dataloader/datasets/ucf101.py:37-46,178-199 with
 * the training transforms of main.py:42-55 after the JPEG decode; additions: the ABI version stays 13).  `blob`: decoded uint8
 * frames, per video [frame][h][w][3], any byte alignment.  One launch writes fp32 dst [B][3][T][S][S]: for clip b the frames
 * `frame[b][t]` of its video, cropped to the integer box (x0, y0, cw, ch) -- cw != ch allowed --, resized to S x S exactly like
 * Pillow's 8-bit `resize(..., BILINEAR)` (integer arithmetic: acc = 2^21 + sum pix * k, clamp(acc >> 22, 0, 255); the horizontal
 * pass first, rounded to uint8, then the vertical pass on those bytes), mirrored in x when flip != 0, then
 * ((v / norm_value) - mean[c]) / std[c] as dvd_clip_to_tensor writes it.
 * `clips`: long long [B][DVD_CLIP_COLS] followed by the frame indices long long [B][T] (0-based within the video), given twice:
 * in host memory (every check below reads it, before any launch) and the same values in device memory.
 * `tables`: device int32 pool of coefficient tables; the table for in -> S samples at position p is [S][2] (first source sample,
 * count) then [S][ksize] coefficients scaled by 2^22, ksize = 2 * ceil(max(in / S, 1)) + 1, made by Pillow's rule in fp64
 * (data.resize_coeffs).  DVD_CLIP_XTAB / _YTAB = positions (in ints) of the tables for cw -> S and ch -> S.  The contents are the
 * caller's responsibility; whatever they hold, no read leaves the crop box.
 * Served: frame sides <= DVD_CLIP_MAX_SIDE, S <= DVD_CLIP_MAX_OUT, B * T < 2^31; a workgroup handles a band of output rows of one
 * frame whose horizontally resized source rows fit 64 KB of LDS (dvd_clip_gather_band_rows(ch, S) = rows per band, the smallest
 * over the batch is used; 0 = not served: never within the limits above).  DVD_E_SHAPE outside that.
 * DVD_E_ARG: a null pointer, a non-positive size or norm_value == 0, a box outside its frame, a video outside the blob
 * (offset + frames * h * w * 3 > blob_bytes), a frame index outside its video, a table position outside the pool.
 * Deterministic: no atomics, a frame's result depends on that frame, its box and its tables alone. */
#define DVD_CLIP_COLS 11
#define DVD_CLIP_OFF 0        /* byte offset of the video's first frame in the blob */
#define DVD_CLIP_H 1
#define DVD_CLIP_W 2
#define DVD_CLIP_FRAMES 3     /* frames of the video */
#define DVD_CLIP_X0 4
#define DVD_CLIP_Y0 5
#define DVD_CLIP_CW 6
#define DVD_CLIP_CH 7
#define DVD_CLIP_FLIP 8
#define DVD_CLIP_XTAB 9
#define DVD_CLIP_YTAB 10
#define DVD_CLIP_MAX_SIDE 4096
#define DVD_CLIP_MAX_OUT 256
int dvd_clip_gather_band_rows(int crop_h, int S);
int dvd_clip_gather(const unsigned char* blob, long long blob_bytes, const long long* clips_host, const long long* clips_dev,
                    const int* tables, long long table_ints, float* dst, long long B, int T, int S, float norm_value,
                    const float* mean_std, void* stream);

/* Sample sheets (sheets.make_sheets, Trainer.save_samples; trainer.py:323-334's save_image(denorm(clip)) = torchvision's make_grid
 * over the frames of a clip, and the 8-bit quantisation of save_image; additions: the ABI version stays 13).  One launch reads fp32
 * frames and writes 8-bit interleaved RGB sheets, ready for a PNG's deflate.
 * `src`: device fp32 seen as [n_sheets][n_tiles][3][H][W]: the H x W planes contiguous, the sheet, tile and channel strides given
 * in ELEMENTS (>= 0; channel stride >= H * W).  A generated batch [B][T][3][H][W] gives one sheet per clip (tiles = its frames) or,
 * with the first two strides exchanged, one sheet per time step (tiles = the clips); a loader clip [B][3][T][H][W] is served through
 * its strides as well.
 * Geometry: torchvision's make_grid(nrow, padding, pad_value) for a sheet of `total_slots` slots:
 *   xmaps = min(nrow, total_slots), ymaps = ceil(total_slots / xmaps), Hs = ymaps (H + padding) + padding,
 *   Ws = xmaps (W + padding) + padding, slot k has its top-left pixel at row (k / xmaps)(H + padding) + padding, column
 *   (k % xmaps)(W + padding) + padding; borders and the empty slots of the last row hold pad_value.  One deviation: a single
 *   tile keeps its border (torchvision returns a lone image bare).
 * The launch fills slots [first_slot, first_slot + n_tiles) with its tiles.  With DVD_SHEET_FILL it also writes every other byte of
 * the sheets (borders, all other slots, the prefix bytes); without, it writes its own tiles' pixels and nothing else -- so launches
 * on one stream compose a sheet from several sources.
 * Value: with DVD_SHEET_SIGNED x = (v + 1) / 2, else x = v; then x = clamp(x, 0, 1), q = clamp(x * 255 + 0.5, 0, 255), byte = q
 * truncated -- every operation rounded on its own in fp32 (no fused multiply-add), the bytes of
 * `x.add(1).div(2).clamp_(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(uint8)`.  +inf -> 255, -inf -> 0, NaN -> 0.  pad_value is
 * quantised as a [0, 1] value.
 * `dst`: device uint8 [n_sheets][Hs][row_prefix + 3 Ws], tight rows, any alignment.  row_prefix = 1 starts every row with a zero
 * byte (PNG filter type "None"): a sheet is then the input of the IDAT's deflate as it stands.
 * Deterministic: every byte has one writer, no atomics.  All checks come before any launch:
 * DVD_E_ARG: a null pointer, n_sheets / n_tiles / total_slots / nrow < 1, first_slot < 0, first_slot + n_tiles > total_slots,
 *   padding outside [0, DVD_SHEET_MAX_PADDING], row_prefix not 0 / 1, unknown flag bits, a negative stride, a channel stride
 *   below H * W.
 * DVD_E_SHAPE: H or W outside [1, DVD_SHEET_MAX_TILE], Hs or Ws above DVD_SHEET_MAX_SIDE, a source byte offset or the destination
 *   size beyond 2^63 - 1, n_sheets * Hs >= 2^31.
 * dvd_sample_sheet_shape (no GPU needed) returns Hs, Ws and the bytes of ONE sheet, Hs * (row_prefix + 3 Ws), with the same
 * refusals for the arguments it takes. */
#define DVD_SHEET_FILL 1
#define DVD_SHEET_SIGNED 2
#define DVD_SHEET_MAX_TILE 4096
#define DVD_SHEET_MAX_SIDE 16384
#define DVD_SHEET_MAX_PADDING 64
int dvd_sample_sheet_shape(int total_slots, int H, int W, int nrow, int padding, int row_prefix, int* Hs, int* Ws,
                           long long* sheet_bytes);
int dvd_sample_sheet(const float* src, long long s_sheet, long long s_tile, long long s_chan, long long n_sheets, int n_tiles,
                     int H, int W, int first_slot, int total_slots, int nrow, int padding, float pad_value, int row_prefix,
                     int flags, unsigned char* dst, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
