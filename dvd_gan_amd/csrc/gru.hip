// ConvGRU layer: the serial (time-recurrent) half of Module/ConvGRU.py:29-54 for one layer and
// all T steps, forward and BPTT.
//
// The reference evaluates three convolutions per cell-step on cat[x, h].  Here each gate conv is
// split by linearity into its x-part and its h-part:
//     conv(cat[x, h]) = conv_x(x) + conv_h(h)
// The x-parts of all three gates and all T steps do not depend on the recurrence; the caller
// computes them as ONE large batched convolution (gx[t] = Wx * x_t + b, columns u|r|o).  Only the
// h-parts remain on the serial chain and are driven from here, without returning to Python:
//     step t :  [u|r] = sigmoid(gx[t][u|r] + conv(h_{t-1}; Wh_ur))        (one N=2h conv)
//               o     = tanh   (gx[t][o]   + conv(h_{t-1}*r; Wh_o))
//               h_t   = h_{t-1}*(1-u) + o*u                                ConvGRU.py:47-52
// Small spatial sizes (4x4, 8x8) give few output tiles, so these convs run split-K and the gate
// kernels below reduce the fp32 slabs while applying the non-linearities.
// Backward walks t = T-1..0 with two backward-data convs per step; every weight gradient and the
// x-path gradient are batched over all T by the caller afterwards (dg holds d(pre-activation)).
#include "conv_common.h"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <queue>
#include <string>
#include <vector>

namespace {


// acc[0..7] += sum over the ns split-K slabs of 8 floats at `off` (slab s starts s * stride floats further).  The loads of four
// slabs are requested before the first is added: these kernels run a few hundred waves on mostly empty CUs and a loop of
// load -> add -> load is a chain of ns L2 / HBM round trips (16 slabs: 12-19 us per launch).  The additions keep slab order.
__device__ __forceinline__ void slab_sum8(const float* ws, int ns, size_t stride, size_t off, float (&acc)[8]) {
    int s = 0;
    for (; s + 4 <= ns; s += 4) {
        float a[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j) load8<float>(ws + (size_t)(s + j) * stride + off, a[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += a[j][k];
    }
    for (; s < ns; ++s) {
        float a[8];
        load8<float>(ws + (size_t)s * stride + off, a);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += a[k];
    }
}

// u, r, hr for one step.  ws: [ns][M][2h] fp32 partial sums of conv(h_prev; Wh_ur) (ns may be 0).
template <typename T>
__global__ void gru_gates_ur_kernel(const float* ws, int ns, const T* gx, int ldg, const T* hprev, T* u, T* r, T* hr,
                                    long long M, int h) {
    const int cg = h / 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * cg) return;
    const long long row = (unsigned)i / (unsigned)cg;          // M * cg < 2^31 (checked by the layer entry points)
    const int c = (int)(i - row * cg) * 8;
    float pu[8], pr[8], hp[8];
    load8<T>(gx + (size_t)row * ldg + c, pu);
    load8<T>(gx + (size_t)row * ldg + h + c, pr);
    if (hprev) load8<T>(hprev + (size_t)row * h + c, hp);
    {
        const size_t stride = (size_t)M * 2 * h, off = (size_t)row * 2 * h + c;
        int s = 0;
        for (; s + 4 <= ns; s += 4) {
            float a[4][8], b[4][8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                load8<float>(ws + (size_t)(s + j) * stride + off, a[j]);
                load8<float>(ws + (size_t)(s + j) * stride + off + h, b[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k) { pu[k] += a[j][k]; pr[k] += b[j][k]; }
        }
        for (; s < ns; ++s) {
            float a[8], b[8];
            load8<float>(ws + (size_t)s * stride + off, a);
            load8<float>(ws + (size_t)s * stride + off + h, b);
#pragma unroll
            for (int k = 0; k < 8; ++k) { pu[k] += a[k]; pr[k] += b[k]; }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        pu[k] = gate_sigmoid<T>(pu[k]);
        pr[k] = round_to<T>(gate_sigmoid<T>(pr[k]));       // the stored r is the r the cell uses
        hp[k] = hprev ? hp[k] * pr[k] : 0.f;
    }
    store8<T>(u + (size_t)row * h + c, pu);
    if (r) store8<T>(r + (size_t)row * h + c, pr);           // (not kept by an inference-mode forward)
    store8<T>(hr + (size_t)row * h + c, hp);
}

// o, h_t.  ws: [ns][M][h] partial sums of conv(h_prev*r; Wh_o).  h32p/h32n: optional fp32 carry.
template <typename T>
__global__ void gru_out_kernel(const float* ws, int ns, const T* gx, int ldg, const T* hprev, const float* h32p,
                               const T* u, T* o, T* hn, float* h32n, long long M, int h) {
    const int cg = h / 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * cg) return;
    const long long row = (unsigned)i / (unsigned)cg;          // M * cg < 2^31 (checked by the layer entry points)
    const int c = (int)(i - row * cg) * 8;
    float po[8], hp[8], uu[8];
    load8<T>(gx + (size_t)row * ldg + 2 * h + c, po);
    if (h32p) load8<float>(h32p + (size_t)row * h + c, hp);
    else if (hprev) load8<T>(hprev + (size_t)row * h + c, hp);
    else {
#pragma unroll
        for (int k = 0; k < 8; ++k) hp[k] = 0.f;
    }
    load8<T>(u + (size_t)row * h + c, uu);
    slab_sum8(ws, ns, (size_t)M * h, (size_t)row * h + c, po);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        po[k] = round_to<T>(gate_tanh<T>(po[k]));
        hp[k] = hp[k] * (1.f - uu[k]) + po[k] * uu[k];
    }
    if (o) store8<T>(o + (size_t)row * h + c, po);
    store8<T>(hn + (size_t)row * h + c, hp);
    if (h32n) store8<float>(h32n + (size_t)row * h + c, hp);
}

// BPTT, first half of step t: dh = dh_out[t] + carry + sum(slabs);  writes d(pre_u), d(pre_o), new carry.
template <typename T>
__global__ void gru_bwd_out_kernel(const T* dh_out, float* carry, const float* ws, int ns, const T* u, const T* o,
                                   const T* hprev, T* dg, int ldg, long long M, int h) {
    const int cg = h / 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * cg) return;
    const long long row = (unsigned)i / (unsigned)cg;          // M * cg < 2^31 (checked by the layer entry points)
    const int c = (int)(i - row * cg) * 8;
    const size_t off = (size_t)row * h + c;
    float dh[8], t8[8], uu[8], oo[8], hp[8], dpu[8], dpo[8];
    load8<float>(carry + off, dh);
    if (dh_out) {
        load8<T>(dh_out + off, t8);
#pragma unroll
        for (int k = 0; k < 8; ++k) dh[k] += t8[k];
    }
    load8<T>(u + off, uu);
    load8<T>(o + off, oo);
    if (hprev) load8<T>(hprev + off, hp);
    slab_sum8(ws, ns, (size_t)M * h, off, dh);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float hpk = hprev ? hp[k] : 0.f;
        dpo[k] = dh[k] * uu[k] * (1.f - oo[k] * oo[k]);
        dpu[k] = dh[k] * (oo[k] - hpk) * uu[k] * (1.f - uu[k]);
        dh[k] = dh[k] * (1.f - uu[k]);
    }
    store8<float>(carry + off, dh);
    store8<T>(dg + (size_t)row * ldg + c, dpu);
    store8<T>(dg + (size_t)row * ldg + 2 * h + c, dpo);
}

// BPTT, second half: d(h*r) = sum(slabs);  carry += d(hr)*r;  d(pre_r) = d(hr)*h_prev*r(1-r).
template <typename T>
__global__ void gru_bwd_r_kernel(float* carry, const float* ws, int ns, const T* r, const T* hprev, T* dg, int ldg,
                                 long long M, int h) {
    const int cg = h / 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * cg) return;
    const long long row = (unsigned)i / (unsigned)cg;          // M * cg < 2^31 (checked by the layer entry points)
    const int c = (int)(i - row * cg) * 8;
    const size_t off = (size_t)row * h + c;
    float dhr[8], t8[8], rr[8], hp[8], cy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) dhr[k] = 0.f;
    slab_sum8(ws, ns, (size_t)M * h, off, dhr);
    if (hprev) {
        load8<T>(r + off, rr);
        load8<T>(hprev + off, hp);
        load8<float>(carry + off, cy);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cy[k] += dhr[k] * rr[k];
            dhr[k] = dhr[k] * hp[k] * rr[k] * (1.f - rr[k]);
        }
        store8<float>(carry + off, cy);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) dhr[k] = 0.f;
    }
    store8<T>(dg + (size_t)row * ldg + h + c, dhr);
}

// out = carry + sum(slabs): gradient wrt the supplied initial hidden state
__global__ void gru_dh0_kernel(const float* carry, const float* ws, int ns, float* out, long long M, int h) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * h) return;
    float v = carry[i];
    for (int s = 0; s < ns; ++s) v += ws[(size_t)s * M * h + i];
    out[i] = v;
}

}  // namespace

#define S_ ((hipStream_t)stream)
#define BY_DTYPE(dtype, ...)                                                   \
    do {                                                                       \
        if ((dtype) == DVD_BF16) { using T = bf16_t; __VA_ARGS__; }            \
        else if ((dtype) == DVD_F32) { using T = float; __VA_ARGS__; }         \
        else return DVD_E_ARG;                                                 \
    } while (0)

namespace {

// ---- one (layer, step): the pointers of its tensors, the gate epilogues and the convolution descriptor built from them.
// dvd_convgru_layer_* and the wavefront schedule (record_forward / record_backward) both use these and nothing else.
struct FwdStep {
    const char* hprev;                 // h_{t-1}: the previous step's state, the supplied h0 at t = 0, or null
    const char* gx;
    char *u, *r, *o, *hr, *hn;         // (r, o: null in an inference-mode forward)
    const float* h32p; float* h32n;    // fp32 carry of h, ping-pong
};
FwdStep fwd_step(const dvd_gru_desc& d, int t) {
    const size_t esz = d.dtype == DVD_BF16 ? 2 : 4, Mh = (size_t)d.B * d.H * d.W * d.hidden, step = Mh * esz;
    const size_t astep = d.infer ? 0 : step;       // inference: u / h*r are one-step scratch, r and o are not stored at all
    FwdStep s;
    s.hprev = t > 0 ? (const char*)d.h_all + (t - 1) * step : (const char*)d.h0;
    s.gx = (const char*)d.gx + (size_t)t * d.gx_stride * esz;
    s.u = (char*)d.u_all + t * astep; s.r = d.infer ? nullptr : (char*)d.r_all + t * step;
    s.o = d.infer ? nullptr : (char*)d.o_all + t * step; s.hr = (char*)d.hr_all + t * astep;
    s.hn = (char*)d.h_all + t * step;
    s.h32p = (d.h32 && t > 0) ? d.h32 + (size_t)(t & 1) * Mh : nullptr;
    s.h32n = d.h32 ? d.h32 + (size_t)((t + 1) & 1) * Mh : nullptr;
    return s;
}
// modes 1 ([u|r] convolution) and 2 (out-gate convolution)
GruEpi epi_fwd(const dvd_gru_desc& d, const FwdStep& s, int mode) {
    GruEpi g = {};
    g.mode = mode; g.h = d.hidden; g.ldg = 3 * d.hidden; g.gx = s.gx; g.hprev = s.hprev; g.h32p = s.h32p; g.u_in = s.u;
    g.u = s.u; g.r = s.r; g.hr = s.hr; g.o = s.o; g.hn = s.hn; g.h32n = s.h32n;
    return g;
}

// dh_all: [T][M][hidden] gradient wrt the layer's states from above (dvd_gru_desc.dh_out, or the x-path of the next layer of a stack), or null
struct BwdStep { const char *hprev, *u, *r, *o, *dho; char* dg; };
BwdStep bwd_step(const dvd_gru_desc& d, int t, const void* dh_all) {
    const size_t esz = d.dtype == DVD_BF16 ? 2 : 4, step = (size_t)d.B * d.H * d.W * d.hidden * esz;
    BwdStep s;
    s.hprev = t > 0 ? (const char*)d.h_all + (t - 1) * step : (const char*)d.h0;
    s.u = (const char*)d.u_all + t * step; s.r = (const char*)d.r_all + t * step; s.o = (const char*)d.o_all + t * step;
    s.dho = dh_all ? (const char*)dh_all + t * step : nullptr;
    s.dg = (char*)d.dg + t * 3 * step;
    return s;
}
// mode 3: the d(h*r) convolution applies the reset-gate step
GruEpi epi_bwd_r(const dvd_gru_desc& d, const BwdStep& s) {
    GruEpi g = {};
    g.mode = 3; g.h = d.hidden; g.ldg = 3 * d.hidden; g.r = const_cast<char*>(s.r); g.hprev = s.hprev; g.h32n = d.carry; g.o = s.dg;
    return g;
}
// mode 4: the d[u|r] convolution of step t adds into the carry; mode 5 (t > 0): the first half of step t - 1 rides in this conv's epilogue
GruEpi epi_bwd_ur(const dvd_gru_desc& d, int t, const void* dh_all) {
    GruEpi g = {};
    g.mode = 4; g.h = d.hidden; g.ldg = 3 * d.hidden; g.h32n = d.carry;
    if (t > 0) {
        const BwdStep p = bwd_step(d, t - 1, dh_all);
        g.mode = 5; g.gx = p.dho; g.u_in = p.u; g.hr = const_cast<char*>(p.o); g.hprev = p.hprev; g.o = p.dg;
    }
    return g;
}

// a k x k convolution over the M rows of one step.  `out`: with a gate epilogue the tensor it names is not written by the conv itself;
// `ws`: fp32 split-K slabs instead of an output (the gate kernel that follows sums them)
dvd_conv_desc step_conv(const dvd_gru_desc& L, const void* in, int C, int ldi, const void* w, const void* wq, int Cout, int nsplit,
                        void* out, float* ws = nullptr) {
    dvd_conv_desc d = {};
    d.dtype = L.dtype; d.frames = L.B; d.T = 1; d.H = L.H; d.W = L.W; d.C = C; d.ldi = ldi; d.Cout = Cout; d.ldo = Cout;
    d.kt = 1; d.kh = L.k; d.kw = L.k; d.nsplit = nsplit; d.in = in; d.w = w; d.wq = wq; d.wq_kind = 1; d.out = out; d.ws = ws;
    return d;
}

// the elementwise gate kernels: all of a step when its convolution is absent (no previous state) or left slabs, the first BPTT step, dh0
enum GateKernel { GK_GATES_UR, GK_OUT, GK_BWD_OUT, GK_BWD_R, GK_DH0 };
const char* const kGateKernelName[] = {"gates_ur", "out", "bwd_out", "bwd_r", "dh0"};
int gate_kernel(int which, const dvd_gru_desc& d, int t, const void* dh_all, const float* ws, int ns, void* stream) {
    const int h = d.hidden;
    const long long M = (long long)d.B * d.H * d.W;
    const unsigned grid = cdiv(M * (h / 8), 256);
    if (which == GK_GATES_UR || which == GK_OUT) {
        const FwdStep s = fwd_step(d, t);
        if (which == GK_GATES_UR)
            BY_DTYPE(d.dtype, gru_gates_ur_kernel<T><<<grid, 256, 0, S_>>>(ws, ns, (const T*)s.gx, 3 * h, (const T*)s.hprev, (T*)s.u, (T*)s.r,
                                                                            (T*)s.hr, M, h));
        else
            BY_DTYPE(d.dtype, gru_out_kernel<T><<<grid, 256, 0, S_>>>(ws, ns, (const T*)s.gx, 3 * h, (const T*)s.hprev, s.h32p, (const T*)s.u,
                                                                       (T*)s.o, (T*)s.hn, s.h32n, M, h));
    } else if (which == GK_DH0) {
        gru_dh0_kernel<<<cdiv(M * h, 256), 256, 0, S_>>>(d.carry, ws, ns, d.dh0, M, h);
    } else {
        const BwdStep s = bwd_step(d, t, dh_all);
        if (which == GK_BWD_OUT)
            BY_DTYPE(d.dtype, gru_bwd_out_kernel<T><<<grid, 256, 0, S_>>>((const T*)s.dho, d.carry, ws, ns, (const T*)s.u, (const T*)s.o,
                                                                           (const T*)s.hprev, (T*)s.dg, 3 * h, M, h));
        else
            BY_DTYPE(d.dtype, gru_bwd_r_kernel<T><<<grid, 256, 0, S_>>>(d.carry, ws, ns, (const T*)s.r, (const T*)s.hprev, (T*)s.dg, 3 * h, M, h));
    }
    return DVD_OK;
}

}  // namespace

// Split-K factor that brings a conv with few output tiles up to ~two workgroups per CU (measured on the
// full step: target 128 -> 948 ms, 256 -> 922, 384 -> 917, 512 -> 913; re-swept with the halo kernels, where a split
// shape gets the 256 x 128 tile at two workgroups per CU: 512 -> 642 ms, 768 -> 634, 1024 -> 626, 1536 -> 661).
// Per layer (tools/gru_microbench.py, round 2) the optimum depends on the filter: the 3 x 3 layers have a short K loop
// (36-72 steps), so a fused gate epilogue without split-K beats a better-filled split launch + gate kernel there
// (S = 32, h = 128: 13.3 -> 11.1 ms; S = 8 / 16, h = 256: 7.2 -> 5.9 and 11.4 -> 10.6 ms per layer); the 5 x 5 layers
// keep 1024 (S = 16, h = 512: 52.0 vs 60.2 ms at 512).
extern "C" int dvd_conv_pick_nsplit(int dtype, long long M, int Cout, int C, int ntaps) {
    const int bk = dtype == DVD_BF16 ? 32 : 16;
    const long long nk = (long long)ntaps * ((C + bk - 1) / bk);
    const long long tiles = ((M + 127) / 128) * ((Cout + 127) / 128);
    // round 3 (gate math batched in the conv epilogue, tools/gru_microbench.py sweep): a 5 x 5 conv with a short K loop
    // (C = 128: 100 steps) no longer gains from a split plus gate kernel once it has 512 tiles (S = 32, h = 128:
    // 180.5 / 208.7 -> 171.0 / 196.4 us per step forward / backward); the long loops (C = 512: 400 steps) still do
    // (round 4, weights from L2: nk = 200 -- the d[u|r] conv of gru3.l2 -- is better off unsplit too: 187.6 -> 174.2 us per step)
    const long long target = ntaps <= 9 || nk <= 200 ? 512 : 1024;
    long long ns = (target + tiles - 1) / tiles;
    // (cap: 8 since the pixel-major tile order skips the out-of-frame filter rows of the 4 x 4 convs -- their K loops are
    //  shorter, and 16 slabs of 2 MB cost more in the gate kernels than they return: 39.1 / 39.4 -> 34.3 / 34.1 us per step)
    constexpr long long cap = 8;
    if (ns > cap) ns = cap;
    // (round 4, whole-frame footprint kernel: the 3 x 3 layers on 8 x 8 frames -- 18 K steps per slice at 4 -- lose more in the gate
    //  kernel's eight slabs than the fuller launch returns: 114.6 / 111.8 -> 100.6 / 102.1 us per step for gru1.l0 / l2, forward + backward)
    if (ntaps <= 9 && M >= 4096 && ns > 4) ns = 4;
    if (ns > nk) ns = nk;
    if (ns < 1) ns = 1;
    return (int)ns;
}

// Largest split-K factor whose slices are combined inside the launch (by the tile's last workgroup to arrive) instead of by a gate
// kernel.  Measured per layer (tools/gru_microbench.py, B = 64, us per step forward / backward, same box): at 2 slices the combine is
// one 64-128 KB slab read and replaces a launch on the chain -- S = 16 layers 102.0 / 106.1 -> 84.3 / 92.1 (3 x 3), 544.5 / 549.3 ->
// 509.2 / 536.1 (5 x 5); at 4 slices it still gains a little (S = 8, 3 x 3: 50.5 / 53.3 -> 47.6 / 50.9); at 8 the serial read of eight
// slabs by ONE workgroup per tile costs more than the gate kernel, which spreads the same reads over the whole chip (S = 4:
// 33.9 / 35.9 -> 37.9 / 39.4, 67.3 / 69.6 -> 72.6 / 80.3).  Fewer, longer slices so that everything combines in-launch lose as well
// (at most 2 slices everywhere: the S = 4 / 8 layers 56.4 -> 70.4 ms over a pass pair).  dvd_gru_desc.combine_max overrides the 4.
constexpr int kInlaunchMax = 4;

// floats of dvd_gru_desc.ws: nsplit slabs of whole output tiles (up to 256 rows x 256 columns) for the widest of the three
// recurrent convolutions of a layer
extern "C" long long dvd_convgru_ws_floats(int dtype, int B, int H, int W, int hidden, int k) {
    const long long M = (long long)B * H * W, Mp = (M + 255) / 256 * 256;
    const int ntaps = k * k, h = hidden;
    auto need = [&](int Cout, int C) -> long long {
        return (long long)dvd_conv_pick_nsplit(dtype, M, Cout, C, ntaps) * Mp * ((Cout + 255) / 256 * 256);
    };
    long long n = need(2 * h, h);
    if (need(h, h) > n) n = need(h, h);
    if (need(h, 2 * h) > n) n = need(h, 2 * h);
    return n;
}

static int capped_nsplit(const dvd_gru_desc* d, long long M, int Cout, int C, int ntaps) {
    const int ns = dvd_conv_pick_nsplit(d->dtype, M, Cout, C, ntaps);
    return (d->ns_cap > 0 && ns > d->ns_cap) ? d->ns_cap : ns;
}
// shape rules common to both passes of the layer path
static int layer_check(const dvd_gru_desc* d) {
    if (d->T <= 0 || d->B <= 0 || d->hidden <= 0 || !(d->k & 1)) return DVD_E_ARG;
    if (d->hidden & 7) return DVD_E_SHAPE;
    if ((long long)d->B * d->H * d->W * (d->hidden / 8) >= (1ll << 31)) return DVD_E_SHAPE;
    return DVD_OK;
}
// One recurrent convolution of the layer path.  `fused`: the gate math runs in its epilogue (split-K: by the tile's last workgroup);
// otherwise it leaves `ns` fp32 slabs in d->ws for the gate kernel that follows -- none when the step has no previous state.
static int layer_conv(const dvd_gru_desc* d, dvd_conv_desc c, GruEpi g, bool has_prev, bool fused, int& ns, void* stream) {
    ns = 0;
    if (!has_prev) return DVD_OK;
    if (fused) {
        g.slabs = d->ws; g.tickets = d->tickets;
        return dvd_conv_forward_gru(&c, &g, stream);
    }
    ns = c.nsplit; c.out = nullptr; c.ws = d->ws;
    return dvd_conv_forward(&c, stream);
}

extern "C" int dvd_convgru_layer_forward(const dvd_gru_desc* d, void* stream) {
    if (!d || !d->gx || !d->w_ur || !d->w_o || !d->h_all || !d->u_all || !d->hr_all || !d->ws) return DVD_E_ARG;
    if (!d->infer && (!d->r_all || !d->o_all)) return DVD_E_ARG;
    if (int rc = layer_check(d)) return rc;
    const int h = d->hidden, ntaps = d->k * d->k;
    const long long M = (long long)d->B * d->H * d->W;
    const int ns_ur = capped_nsplit(d, M, 2 * h, h, ntaps);
    const int ns_o = capped_nsplit(d, M, h, h, ntaps);
    const int nmax = !d->tickets ? 1 : d->combine_max > 0 ? d->combine_max : kInlaunchMax;    // convs with up to nmax slices apply the gates in their epilogue
    for (int t = 0; t < d->T; ++t) {
        const FwdStep s = fwd_step(*d, t);
        const bool prev = s.hprev != nullptr, fuse_ur = prev && ns_ur <= nmax, fuse_o = prev && ns_o <= nmax;
        int rc, ns;
        rc = layer_conv(d, step_conv(*d, s.hprev, h, h, d->w_ur, d->w_ur_q, 2 * h, ns_ur, s.u), epi_fwd(*d, s, 1), prev, fuse_ur, ns, stream);
        if (!rc && !fuse_ur) rc = gate_kernel(GK_GATES_UR, *d, t, nullptr, d->ws, ns, stream);
        if (rc) return rc;
        rc = layer_conv(d, step_conv(*d, s.hr, h, h, d->w_o, d->w_o_q, h, ns_o, s.hn), epi_fwd(*d, s, 2), prev, fuse_o, ns, stream);
        if (!rc && !fuse_o) rc = gate_kernel(GK_OUT, *d, t, nullptr, d->ws, ns, stream);
        if (rc) return rc;
    }
    return launch_status();
}

extern "C" int dvd_convgru_layer_backward(const dvd_gru_desc* d, void* stream) {
    if (!d || !d->wd_ur || !d->wd_o || !d->h_all || !d->u_all || !d->r_all || !d->o_all || !d->dg || !d->carry || !d->ws)
        return DVD_E_ARG;
    if (int rc = layer_check(d)) return rc;
    const int h = d->hidden, ntaps = d->k * d->k;
    const long long M = (long long)d->B * d->H * d->W;
    const size_t esz = d->dtype == DVD_BF16 ? 2 : 4;
    const int ns_o = capped_nsplit(d, M, h, h, ntaps);        // d(hr)  = convT(d pre_o)
    const int ns_ur = capped_nsplit(d, M, h, 2 * h, ntaps);   // dh    += convT(d pre_u | d pre_r)
    const int nmax = !d->tickets ? 1 : d->combine_max > 0 ? d->combine_max : kInlaunchMax;
    hipError_t e = hipMemsetAsync(d->carry, 0, (size_t)M * h * sizeof(float), S_);
    if (e != hipSuccess) return DVD_E_LAUNCH;
    int ns_pending = 0;      // slabs of the ur backward-data conv of step t+1 waiting in ws
    bool out_done = false;   // first half of this step already applied by the previous step's conv epilogue (mode 5)
    for (int t = d->T - 1; t >= 0; --t) {
        const BwdStep s = bwd_step(*d, t, d->dh_out);
        const bool prev = s.hprev != nullptr, fuse_o = prev && ns_o <= nmax, fuse_ur = prev && ns_ur <= nmax;
        int rc = DVD_OK, ns;
        if (!out_done) rc = gate_kernel(GK_BWD_OUT, *d, t, d->dh_out, d->ws, ns_pending, stream);
        if (rc) return rc;
        rc = layer_conv(d, step_conv(*d, s.dg + (size_t)2 * h * esz, h, 3 * h, d->wd_o, d->wd_o_q, h, ns_o, d->carry), epi_bwd_r(*d, s), prev,
                        fuse_o, ns, stream);
        if (!rc && !fuse_o) rc = gate_kernel(GK_BWD_R, *d, t, d->dh_out, d->ws, ns, stream);
        if (rc) return rc;
        // the [u|r] backward-data conv adds straight into the carry and goes on with the first half of step t-1 unless this is step 0 with an h0
        rc = layer_conv(d, step_conv(*d, s.dg, 2 * h, 3 * h, d->wd_ur, d->wd_ur_q, h, ns_ur, d->carry), epi_bwd_ur(*d, t, d->dh_out), prev,
                        fuse_ur, ns_pending, stream);
        if (rc) return rc;
        out_done = fuse_ur && t > 0;
    }
    if (d->dh0) gate_kernel(GK_DH0, *d, 0, nullptr, d->ws, ns_pending, stream);
    return launch_status();
}

// ============================================================================ layer wavefront over a ConvGRU stack (round 5)
// See include/dvdgan_hip.h (dvd_gru_stack_desc).  Launch pair k of the forward pass:
//   U group:  [u|r] convolution of (layer l, step t = k - 2 l) for every layer with 0 <= t < T
//   O group:  out-gate convolution of the same (l, t), plus the x-part convolution of (layer l >= 1, step k - 2 l + 1) -- its input,
//             layer l-1's state of that step, was finished by the O group of pair k - 1; its result is read by the U group of pair k + 1
// and of the backward pass (layers in reverse, layer l works on step t = T - 1 - (k - 2 (L - 1 - l))):
//   A group:  d(h*r) convolution (epilogue: reset-gate step)
//   B group:  d[u|r] convolution (epilogue: carry + first half of step t - 1), plus for l >= 1 the x-part backward-data convolution of
//             step t (all three gate gradients of the step are complete), whose result is layer l-1's dh_out of step t -- needed by
//             layer l-1's B convolution of step t + 1 in pair k + 1.
// The steps without a previous state (t = 0, no h0) and the first BPTT step of a layer run the elementwise gate kernels.
//
// A pass is RECORDED first (record_forward / record_backward: every launch in issue order, every member's descriptor, epilogue,
// split-K factor and slab offset) and then PLAYED (play).  The sizing query reads the same record, so a launch can only use slab
// offsets the caller was told about; a stack whose record holds a group of more than kGroupMax members is not served at all.
namespace {

struct Member { dvd_conv_desc d; GruEpi g; long long tiles; int kchunks; int gate; };
struct Launch {
    int kind;                 // >= 0: grouped launch of kGroupKind[kind], members [first, first + n) of Schedule::d / g; -1: gate kernel
    int first, n;
    long long ws_end;         // slab cursor behind the group's last member
    int which, layer, t;      // gate kernel: GateKernel, its layer and step
};
struct Schedule {
    bool backward = false;
    std::vector<Launch> ops;
    std::vector<dvd_conv_desc> d;
    std::vector<GruEpi> g;
    long long ws_floats = 0;  // largest slab cursor of any group
    int max_members = 0;
};
// debug bookkeeping behind dvd_debug_stack_ws (tests only): the last sizing answer and the largest slab cursor a PLAYED group used
std::atomic<long long> g_ws_sized{0}, g_ws_high{0};
constexpr int kMaxMember = 2 * DVD_GRU_STACK_MAX;

// kernel family serving a stack: 0 = frames >= 16 pixels (256 x 128 tiles), 2 / 3 = 8 x 8 frames (256- / 128-row tiles), 4 = 4 x 4
int stack_kind(const dvd_gru_stack_desc* s) {
    const dvd_gru_desc& a = s->layer[0];
    if (a.H != a.W || ilog2_exact(a.H) < 0) return -1;
    if (a.H >= 16) return 0;                         // (128 x 128 tiles, three workgroups per CU: 4-8 % slower on the 16 x 16 / 32 x 32 stages)
    if (a.H == 4) return 4;
    if (a.H != 8) return -1;
    long long t256 = 0;                              // tiles of the U group on 256-row tiles
    for (int l = 0; l < s->n_layers; ++l) t256 += (long long)cdiv(a.B, 4) * cdiv(2 * s->layer[l].hidden, 128);
    return t256 >= 256 ? 2 : 3;
}

Member member(const dvd_gru_desc& L, int kind, const void* in, int C, int ldi, const void* w, const void* wq, int Cout, void* out,
              const GruEpi& g = GruEpi{}) {
    Member m = {};
    m.d = step_conv(L, in, C, ldi, w, wq, Cout, 1, out);
    m.g = g;
    m.gate = g.mode != 0;
    m.tiles = (long long)cdiv((long long)L.B * L.H * L.W, kGroupKind[kind].rows) * cdiv(Cout, 128);
    m.kchunks = (C + 31) / 32;
    return m;
}

// ---- split-K factors of a grouped launch: a search over per-member factors against a model of the launch.
// The members of a group differ 5x in K length (3 x 3 on 256 channels beside 5 x 5 on 768): one factor for all of them -- the
// first round-5 policy, "fill 512 workgroups" -- splits short tiles for nothing and leaves the long tiles of the 5 x 5 layer as
// the launch's makespan.  Model: an XCD runs its share of the workgroups on `slots` concurrent slots in the
// order group_dispatch issues them (members by decreasing length); a workgroup costs its K steps plus a fixed prologue / epilogue
// (in K steps), a split tile a little more (slab traffic, the combine by its last workgroup).  Plans are cached per signature.
struct SplitPlan { int ns[2 * DVD_GRU_STACK_MAX]; };
double model_makespan(int n, const long long* tiles, const int* units, const int* ns, int slots, double fixed, double split_cost) {
    int order[2 * DVD_GRU_STACK_MAX];
    double len[2 * DVD_GRU_STACK_MAX];
    for (int i = 0; i < n; ++i) { order[i] = i; len[i] = (double)units[i] / ns[i] + fixed + (ns[i] > 1 ? split_cost : 0.0); }
    std::sort(order, order + n, [&](int a, int b) { return (double)units[a] / ns[a] > (double)units[b] / ns[b]; });
    std::priority_queue<double, std::vector<double>, std::greater<double>> q;
    for (int i = 0; i < slots; ++i) q.push(0.0);
    double end = 0.0;
    for (int oi = 0; oi < n; ++oi) {
        const int i = order[oi];
        const long long w = (tiles[i] * ns[i] + 7) / 8;              // this XCD's workgroups of member i
        for (long long k = 0; k < w; ++k) {
            const double t = q.top() + len[i];
            q.pop(); q.push(t);
            if (t > end) end = t;
        }
    }
    return end;
}
SplitPlan plan_splits(int kind, bool backward, int n, const Member* m, long long cap) {
    static std::map<std::string, SplitPlan> cache;
    static std::mutex mu;
    long long tiles[2 * DVD_GRU_STACK_MAX]; int units[2 * DVD_GRU_STACK_MAX], capi[2 * DVD_GRU_STACK_MAX];
    std::string key;
    key.append((const char*)&kind, sizeof kind); key.push_back(backward ? 1 : 0);
    for (int i = 0; i < n; ++i) {
        tiles[i] = m[i].tiles; units[i] = m[i].kchunks * m[i].d.kh * m[i].d.kw;
        capi[i] = (int)std::min<long long>(cap, m[i].kchunks);
        if (m[i].tiles > 1024) capi[i] = 1;                               // one ticket per tile, 1024 tickets per member
        key.append((const char*)&tiles[i], sizeof tiles[i]); key.append((const char*)&units[i], sizeof units[i]);
        key.append((const char*)&capi[i], sizeof capi[i]);
    }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    const int slots = kGroupKind[kind].slots;
    // fitted on tools/gru_microbench.py stack (B = 64; K steps of the launch's tile shape): a split tile is cheap on 4 x 4 frames
    // (64 KB slabs, few tiles) and dear on 256-row tiles (128 KB slabs; the tile's last workgroup combines, then runs the epilogue):
    // 8 x 8 forward 13.85 -> 12.87 ms with only the 5 x 5 layer split, 4 x 4 5.39 / 6.09 -> 5.03 / 5.56, 16 x 16 backward 46.1 -> 45.0
    const double fixed = kGroupKind[kind].rows == 256 ? 12.0 : 16.0;
    const double split_cost = kind == 4 ? 3.0 : kind == 0 ? 150.0 : backward ? 50.0 : 80.0;
    static const int opts[] = {1, 2, 3, 4, 8};
    SplitPlan best{}; double best_t = 1e30;
    int idx[2 * DVD_GRU_STACK_MAX] = {0};
    if (n > 5) {
        // 5^n combinations stop being "a few ms once" beyond five members (a four-layer stack's six-member groups: 15.6 k makespan
        // simulations under the lock): coordinate descent from the unsplit plan -- one member's factor at a time, until no change helps
        int ns[2 * DVD_GRU_STACK_MAX];
        for (int i = 0; i < n; ++i) ns[i] = 1;
        auto cost = [&]() { int k = 0; for (int i = 0; i < n; ++i) k += ns[i] > 1;
                            return model_makespan(n, tiles, units, ns, slots, fixed, split_cost) * (1.0 + 0.004 * k); };
        best_t = cost();
        for (bool moved = true; moved;) {
            moved = false;
            for (int i = 0; i < n; ++i) {
                const int keep = ns[i]; int pick = keep;
                for (int o : opts) {
                    if (o > capi[i] || o == keep) continue;
                    ns[i] = o;
                    const double t = cost();
                    if (t < best_t * (1.0 - 1e-9)) { best_t = t; pick = o; moved = true; }
                }
                ns[i] = pick;
            }
        }
        for (int i = 0; i < n; ++i) best.ns[i] = ns[i];
    } else
    for (;;) {
        int ns[2 * DVD_GRU_STACK_MAX]; bool ok = true; int nsplit_members = 0;
        for (int i = 0; i < n; ++i) { ns[i] = opts[idx[i]]; if (ns[i] > capi[i]) ok = false; nsplit_members += ns[i] > 1; }
        if (ok) {
            const double t = model_makespan(n, tiles, units, ns, slots, fixed, split_cost) * (1.0 + 0.004 * nsplit_members);
            if (t < best_t) { best_t = t; for (int i = 0; i < n; ++i) best.ns[i] = ns[i]; }
        }
        int j = 0;
        while (j < n && ++idx[j] == (int)(sizeof opts / sizeof opts[0])) idx[j++] = 0;
        if (j == n) break;
    }
    cache[key] = best;
    return best;
}

// Records one grouped launch: the split-K factor of every member and the slab space behind it.  (A group past kGroupMax members is
// only counted: no launch exists for it, and stack_check refuses the stack.)
void record_group(Schedule& sc, const dvd_gru_stack_desc* s, int kind, Member* m, int n) {
    if (n > sc.max_members) sc.max_members = n;
    if (n == 0 || n > kGroupMax) return;
    // measured (tools/gru_microbench.py stack, B = 64): (target, cap) = (768, 4) 5.46 / 6.99 ms forward / backward on 4 x 4 frames,
    // (768, 8) 5.66 / 6.16; 8 x 8 frames: (768, 4) 14.86 / 15.09, (768, 8) 14.93 / 15.95, (384, 4) 14.46 / 16.53, (1536, *) slower
    const long long cap = (kind == 4 && sc.backward) ? 8 : 4;
    SplitPlan plan{};
    if (!s->layer_policy) plan = plan_splits(kind, sc.backward, n, m, cap);
    long long cursor = 0;
    for (int i = 0; i < n; ++i) {
        long long ns = plan.ns[i];
        if (s->layer_policy)
            ns = m[i].gate ? dvd_conv_pick_nsplit(DVD_BF16, (long long)m[i].d.frames * m[i].d.H * m[i].d.W, m[i].d.Cout, m[i].d.C,
                                                  m[i].d.kh * m[i].d.kw) : 1;
        if (s->layer[0].ns_cap > 0 && ns > s->layer[0].ns_cap) ns = s->layer[0].ns_cap;
        if (ns > m[i].kchunks) ns = m[i].kchunks;
        if (ns > 1 && m[i].tiles > 1024) ns = 1;
        m[i].d.nsplit = (int)ns;
        if (ns > 1) {
            if (m[i].g.mode == 0) m[i].g.mode = 6;            // direct epilogue behind the in-launch combine
            m[i].g.slabs = s->ws + cursor; m[i].g.tickets = s->layer[0].tickets;
            cursor += ns * m[i].tiles * kGroupKind[kind].tile_floats;      // accumulators of one output tile
        }
        sc.d.push_back(m[i].d);
        sc.g.push_back(m[i].g);
    }
    if (cursor > sc.ws_floats) sc.ws_floats = cursor;
    sc.ops.push_back(Launch{kind, (int)sc.d.size() - n, n, cursor, 0, 0, 0});
}
void record_gate(Schedule& sc, int which, int layer, int t) { sc.ops.push_back(Launch{-1, 0, 0, 0, which, layer, t}); }

// gradient wrt layer l's states, [T][M][hidden_l]: from outside the stack (top layer) or from the x-path of the layer above
const void* stack_dh(const dvd_gru_stack_desc* s, int l) { return l == s->n_layers - 1 ? s->layer[l].dh_out : s->dh_mid[l + 1]; }

void record_forward(const dvd_gru_stack_desc* s, Schedule& sc) {
    const int L = s->n_layers, T = s->layer[0].T, kind = stack_kind(s);
    // bit l: the x-part of layer l rides in the U group instead of the O group (both are behind its producer).  Measured
    // (tools/gru_microbench.py stack): no difference beyond noise except on 8 x 8 frames, where the top layer's x-part in the
    // U group balances the two launches of a pair (14.63 -> 13.93 ms forward, 15.77 -> 14.76 backward)
    const int x_in_u = s->layer[0].H == 8 ? 4 : 0;
    for (int k = 0; k < T + 2 * (L - 1); ++k)
        for (int phase = 0; phase < 2; ++phase) {                 // 0 = U group, 1 = O group
            Member mem[kMaxMember];
            int n = 0;
            for (int l = 0; l < L; ++l) {
                const dvd_gru_desc& d = s->layer[l];
                const int t = k - 2 * l, h = d.hidden;
                if (t < 0 || t >= T) continue;
                if (t == 0 && !d.h0) {                            // step 0 without a supplied state: gates of the x-part alone
                    record_gate(sc, phase == 0 ? GK_GATES_UR : GK_OUT, l, t);
                    continue;
                }
                const FwdStep st = fwd_step(d, t);
                mem[n++] = phase == 0 ? member(d, kind, st.hprev, h, h, d.w_ur, d.w_ur_q, 2 * h, st.u, epi_fwd(d, st, 1))
                                      : member(d, kind, st.hr, h, h, d.w_o, d.w_o_q, h, st.hn, epi_fwd(d, st, 2));
            }
            for (int l = 1; l < L; ++l)
                if (phase == (((x_in_u >> l) & 1) ? 0 : 1)) {     // x-part of layer l for step k - 2 l + 1
                    const dvd_gru_desc& d = s->layer[l];
                    const int t = k - 2 * l + 1, ci = s->layer[l - 1].hidden;
                    if (t < 0 || t >= T) continue;
                    mem[n] = member(d, kind, fwd_step(s->layer[l - 1], t).hn, ci, ci, s->wx[l], s->wx_q[l], 3 * d.hidden,
                                    const_cast<char*>(fwd_step(d, t).gx));
                    mem[n++].d.bias = s->bx[l];
                }
            record_group(sc, s, kind, mem, n);
        }
}

void record_backward(const dvd_gru_stack_desc* s, Schedule& sc) {
    const int L = s->n_layers, T = s->layer[0].T, kind = stack_kind(s);
    const int dx_in_a = s->layer[0].H == 8 ? 4 : 0;       // bit l: layer l's x-part backward-data rides in the NEXT pair's A group (see x_in_u)
    sc.backward = true;
    // x-part backward-data convolution of (layer l >= 1, step t): the gradient reaching layer l-1's state of that step
    auto dx_member = [&](int l, int t) {
        const dvd_gru_desc& d = s->layer[l];
        const int ci = s->cin[l], h = d.hidden;
        const size_t off = (size_t)t * d.B * d.H * d.W * ci * 2;
        Member m = member(d, kind, bwd_step(d, t, nullptr).dg, 3 * h, 3 * h, s->wdx[l], s->wdx_q[l], ci, (char*)s->dh_mid[l] + off);
        if (s->layer[l - 1].dh_out) { m.d.res = (const char*)s->layer[l - 1].dh_out + off; m.d.ldres = ci; }
        return m;
    };
    for (int k = 0; k < T + 2 * (L - 1); ++k)
        for (int phase = 0; phase < 2; ++phase) {                 // 0 = A group, 1 = B group
            Member mem[kMaxMember];
            int n = 0;
            for (int l = L - 1; l >= 0; --l) {
                const dvd_gru_desc& d = s->layer[l];
                const int t = T - 1 - (k - 2 * (L - 1 - l)), h = d.hidden;
                if (phase == 0 && l > 0 && ((dx_in_a >> l) & 1) && t >= -1 && t + 1 < T) mem[n++] = dx_member(l, t + 1);     // of the step finished in the previous pair
                if (t < 0 || t >= T) continue;
                const BwdStep st = bwd_step(d, t, stack_dh(s, l));
                const bool has_prev = t > 0 || d.h0 != nullptr;
                if (phase == 0) {
                    if (t == T - 1) record_gate(sc, GK_BWD_OUT, l, t);      // first BPTT step of the layer: nothing upstream to ride on
                    if (has_prev) mem[n++] = member(d, kind, st.dg + (size_t)2 * h * 2, h, 3 * h, d.wd_o, d.wd_o_q, h, d.carry, epi_bwd_r(d, st));
                    else record_gate(sc, GK_BWD_R, l, t);
                } else {
                    if (has_prev)                                 // ... and the first half of step t - 1
                        mem[n++] = member(d, kind, st.dg, 2 * h, 3 * h, d.wd_ur, d.wd_ur_q, h, d.carry, epi_bwd_ur(d, t, stack_dh(s, l)));
                    if (l > 0 && !((dx_in_a >> l) & 1)) mem[n++] = dx_member(l, t);
                }
            }
            record_group(sc, s, kind, mem, n);
        }
    for (int l = 0; l < L; ++l)
        if (s->layer[l].dh0) record_gate(sc, GK_DH0, l, 0);
}

void record(const dvd_gru_stack_desc* s, bool backward, Schedule& sc) {
    const size_t groups = 2 * (size_t)(s->layer[0].T + 2 * (s->n_layers - 1));
    sc.ops.reserve(groups + 3 * s->n_layers);
    sc.d.reserve(groups * (2 * s->n_layers - 1));
    sc.g.reserve(groups * (2 * s->n_layers - 1));
    if (backward) record_backward(s, sc); else record_forward(s, sc);
}

// Argument and shape rules, then the schedule itself: a stack is served only if no grouped launch of it needs more than kGroupMax members
int stack_check(const dvd_gru_stack_desc* s, bool backward, Schedule& sc) {
    if (!s || s->n_layers < 1 || s->n_layers > DVD_GRU_STACK_MAX) return DVD_E_ARG;
    const dvd_gru_desc& a = s->layer[0];
    if (a.dtype != DVD_BF16 || a.T <= 0 || a.B <= 0 || !a.tickets || !s->ws) return DVD_E_ARG;
    if (stack_kind(s) < 0) return DVD_E_SHAPE;
    for (int l = 0; l < s->n_layers; ++l) {
        const dvd_gru_desc& d = s->layer[l];
        if (d.dtype != a.dtype || d.T != a.T || d.B != a.B || d.H != a.H || d.W != a.W) return DVD_E_ARG;
        if (d.hidden <= 0 || (d.hidden & 7) || (d.k != 3 && d.k != 5)) return DVD_E_SHAPE;
        if ((long long)d.B * d.H * d.W * (d.hidden / 8) >= (1ll << 31)) return DVD_E_SHAPE;
        if (!d.gx || !d.h_all || !d.u_all || !d.hr_all) return DVD_E_ARG;
        if (l > 0 && (s->cin[l] != s->layer[l - 1].hidden || d.gx_stride != (long long)d.B * d.H * d.W * 3 * d.hidden)) return DVD_E_ARG;
        if (!backward) {
            if (!d.w_ur || !d.w_o || !d.w_ur_q || !d.w_o_q) return DVD_E_ARG;
            if (!d.infer && (!d.r_all || !d.o_all)) return DVD_E_ARG;
            if (l > 0 && (!s->wx[l] || !s->wx_q[l] || !s->bx[l])) return DVD_E_ARG;
        } else {
            if (!d.wd_ur || !d.wd_o || !d.wd_ur_q || !d.wd_o_q || !d.r_all || !d.o_all || !d.dg || !d.carry) return DVD_E_ARG;
            if (l > 0 && (!s->wdx[l] || !s->wdx_q[l] || !s->dh_mid[l])) return DVD_E_ARG;
        }
    }
    record(s, backward, sc);
    return sc.max_members > kGroupMax ? DVD_E_SHAPE : DVD_OK;
}

// Issues a recorded pass on `stream`
int play(const dvd_gru_stack_desc* s, const Schedule& sc, void* stream) {
    if (sc.backward)
        for (int l = 0; l < s->n_layers; ++l) {
            const dvd_gru_desc& d = s->layer[l];
            if (hipMemsetAsync(d.carry, 0, (size_t)d.B * d.H * d.W * d.hidden * sizeof(float), S_) != hipSuccess) return DVD_E_LAUNCH;
        }
    for (const Launch& op : sc.ops) {
        int rc;
        if (op.kind < 0) rc = gate_kernel(op.which, s->layer[op.layer], op.t, stack_dh(s, op.layer), nullptr, 0, stream);
        else {
            for (long long seen = g_ws_high.load(); op.ws_end > seen && !g_ws_high.compare_exchange_weak(seen, op.ws_end);) {}
            rc = dvd_conv_forward_group(&sc.d[op.first], &sc.g[op.first], op.n, op.kind, s->run, stream);
        }
        if (rc) return rc;
    }
    return launch_status();
}

}  // namespace

extern "C" int dvd_convgru_stack_ok(const dvd_gru_stack_desc* d, int backward) {
    dvd_gru_stack_desc t;
    if (!d) return 0;
    t = *d;
    static float dummy;
    if (!t.ws) t.ws = &dummy;                                     // (a geometry / pointer-completeness query: the workspace may not exist yet)
    Schedule sc;
    return stack_check(&t, backward != 0, sc) == DVD_OK ? 1 : 0;
}
extern "C" long long dvd_convgru_stack_ws_floats(const dvd_gru_stack_desc* d) {
    if (!d || d->n_layers < 1 || d->n_layers > DVD_GRU_STACK_MAX || stack_kind(d) < 0) return 0;
    Schedule f, b;
    record(d, false, f);
    record(d, true, b);
    if (std::max(f.max_members, b.max_members) > kGroupMax) return 0;
    const long long need = std::max(f.ws_floats, b.ws_floats);
    g_ws_sized.store(need);
    return need > 0 ? need : 1;
}
// Test hook: out[0] = floats the last dvd_convgru_stack_ws_floats call asked for (0 = no member of any group is split),
// out[1] = the largest slab cursor any grouped launch has used since the last reset.  reset != 0 clears out[1] afterwards.
extern "C" void dvd_debug_stack_ws(long long* out, int reset) {
    if (out) { out[0] = g_ws_sized.load(); out[1] = g_ws_high.load(); }
    if (reset) g_ws_high.store(0);
}
extern "C" int dvd_convgru_stack_forward(const dvd_gru_stack_desc* d, void* stream) {
    Schedule sc;
    const int rc = stack_check(d, false, sc);
    return rc ? rc : play(d, sc, stream);
}
extern "C" int dvd_convgru_stack_backward(const dvd_gru_stack_desc* d, void* stream) {
    Schedule sc;
    const int rc = stack_check(d, true, sc);
    return rc ? rc : play(d, sc, stream);
}

// Test hook (tests/native/stack_schedule.cpp; hidden from the library's exports): the recorded schedule of one pass as text, one line
// per launch in issue order.  Only the geometry is looked at: the pointers of `d` may be placeholders.
extern "C" int dvd_convgru_stack_dump(const dvd_gru_stack_desc* d, int backward, FILE* out) {
    if (!d || d->n_layers < 1 || d->n_layers > DVD_GRU_STACK_MAX || stack_kind(d) < 0) return DVD_E_SHAPE;
    Schedule sc;
    record(d, backward != 0, sc);
    for (const Launch& op : sc.ops) {
        if (op.kind < 0) {
            fprintf(out, "%s h=%d t=%d\n", kGateKernelName[op.which], d->layer[op.layer].hidden, op.t);
            continue;
        }
        fprintf(out, "%s kind=%d", backward ? "bwd" : "fwd", op.kind);
        for (int i = op.first; i < op.first + op.n; ++i) {
            const dvd_conv_desc& c = sc.d[i];
            fprintf(out, " | C=%d ldi=%d Cout=%d k=%d mode=%d bias=%d res=%d ns=%d off=%lld", c.C, c.ldi, c.Cout, c.kh, sc.g[i].mode,
                    c.bias != nullptr, c.res != nullptr, c.nsplit, c.nsplit > 1 ? (long long)(sc.g[i].slabs - d->ws) : -1ll);
        }
        fprintf(out, "\n");
    }
    fprintf(out, "ws=%lld max_members=%d\n", sc.ws_floats, sc.max_members);
    return DVD_OK;
}
