// dvdx_tsru_forward / dvdx_tsru_backward (include/dvdx_tsru.h), built into libdvdx_tsru.so: the pointwise part of the TSRU -- warp
// the previous state by the predicted flow (bilinear, zero fill), blend it with new content -- and its backward pass.  Memory-bound
// gathers over channels-last tensors: a thread owns 8 channels of a pixel, consecutive lanes hold consecutive channel vectors, so
// each of the four taps of a pixel is one coalesced run of the row [C] and every store is a coalesced run too.  The backward pass
// is two launches: the first owns the pixel's gate gradients, leaves g = dh * u and the flow in scratch and reduces the flow
// gradient over the channels inside the wave; the second is the transpose of the warp as a gather -- each dh_prev element has one
// owner, which walks the window of pixels that can reach it in a fixed order.  No atomics, no LDS, no scratch memory.
#include "../../csrc/common.h"
#include "../../../include/dvdx_tsru.h"

// every multiply-add below is written as fmaf or as separate operations: the forward's and the transpose's weights must be the
// same bits, whichever way the compiler would have contracted either
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = DVDX_TSRU_THREADS;
constexpr long long kSmallLaunch = 65536;        // threads below which a launch uses one-wave workgroups

struct Geo {
    int H, W, C, nv;            // nv = C / 8 channel vectors of a pixel
    long long M;                // B * H * W pixels
};

// The bilinear cell of pixel (x, y) displaced by (tx, ty): false when the pixel samples nothing (outside (-1, W) x (-1, H); a NaN
// fails the test).  Only a position that passed is converted to an integer: x0 in [-1, W - 1], y0 in [-1, H - 1].  The one
// expression all three kernels use.
__device__ __forceinline__ bool locate(float tx, float ty, int x, int y, int H, int W, int& x0, int& y0, float& wx1, float& wy1) {
    const float sx = (float)x + tx, sy = (float)y + ty;
    if (!(sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H)) return false;
    const float fx = floorf(sx), fy = floorf(sy);
    x0 = (int)fx;
    y0 = (int)fy;
    wx1 = sx - fx;
    wy1 = sy - fy;
    return true;
}

// the four taps of a cell, 8 channels each, zero where the neighbour's column or line is outside the frame
__device__ __forceinline__ void taps8(const float* frame, int H, int W, int C, int c0, int x0, int y0, float (&v00)[8],
                                      float (&v01)[8], float (&v10)[8], float (&v11)[8]) {
    const bool l = x0 >= 0, r = x0 + 1 < W, t = y0 >= 0, b = y0 + 1 < H;
    const float* p = frame + ((long long)y0 * W + x0) * C + c0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v00[i] = v01[i] = v10[i] = v11[i] = 0.f;
    if (t && l) load8<float>(p, v00);
    if (t && r) load8<float>(p + C, v01);
    if (b && l) load8<float>(p + (long long)W * C, v10);
    if (b && r) load8<float>(p + (long long)W * C + C, v11);
}

// warped state of 8 channels; `in`, the cell and the weights as locate() left them
__device__ __forceinline__ void warp8(bool in, float wx1, float wy1, const float (&v00)[8], const float (&v01)[8],
                                      const float (&v10)[8], const float (&v11)[8], float (&o)[8]) {
    if (!in) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = 0.f;
    } else if (wx1 == 0.f && wy1 == 0.f) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = v00[i];
    } else {
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = fmaf(w11, v11[i], fmaf(w10, v10[i], fmaf(w01, v01[i], w00 * v00[i])));
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void tsru_forward_kernel(Geo g, const float* h_prev, const T* a, int lda, int off_c, int off_u,
                                                                const float* theta_raw, int ldt, float d, float* h, T* h_c) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= g.M * g.nv) return;
    const long long m = idx / g.nv;
    const int c0 = (int)(idx - m * g.nv) * 8;
    const int x = (int)(m % g.W), y = (int)((m / g.W) % g.H);
    const float* frame = h_prev + (m - ((long long)y * g.W + x)) * g.C;
    const float tx = d * gate_tanh<T>(theta_raw[m * ldt]), ty = d * gate_tanh<T>(theta_raw[m * ldt + 1]);
    int x0 = 0, y0 = 0;
    float wx1 = 0.f, wy1 = 0.f;
    const bool in = locate(tx, ty, x, y, g.H, g.W, x0, y0, wx1, wy1);
    float v00[8], v01[8], v10[8], v11[8], hw[8], ac[8], au[8], o[8];
    if (in) taps8(frame, g.H, g.W, g.C, c0, x0, y0, v00, v01, v10, v11);
    warp8(in, wx1, wy1, v00, v01, v10, v11, hw);
    load8<T>(a + m * lda + off_c + c0, ac);
    load8<T>(a + m * lda + off_u + c0, au);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float u = gate_sigmoid<T>(au[i]), c = fmaxf(ac[i], 0.f);
        o[i] = fmaf(u, hw[i] - c, c);
    }
    store8<float>(h + m * g.C + c0, o);
    if (h_c) store8<T>(h_c + m * g.C + c0, o);
}

// First launch of the backward pass.  G lanes (a power of two, <= 64) own a pixel: lane j of the group takes the channel vectors
// j, j + G, ...; every lane of a wave stays to the end (the shuffles need them), lanes past the last pixel add zeros.
template <typename T>
__global__ __launch_bounds__(kThreads) void tsru_backward_gates_kernel(Geo g, int G, const float* dh, const float* dh2, const float* h_prev,
                                                                       const T* a, int lda, int off_c, int off_u, const float* theta_raw,
                                                                       int ldt, float d, T* da, int ldda, int doff_c, int doff_u,
                                                                       T* dtheta_raw, int lddt, float* gbuf, float* flow) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long m = idx / G;
    const int j = (int)(idx - m * G);
    const bool live = m < g.M;
    float sum_x = 0.f, sum_y = 0.f, tanh_x = 0.f, tanh_y = 0.f;
    if (live) {
        const int x = (int)(m % g.W), y = (int)((m / g.W) % g.H);
        const float* frame = h_prev + (m - ((long long)y * g.W + x)) * g.C;
        tanh_x = gate_tanh<T>(theta_raw[m * ldt]);
        tanh_y = gate_tanh<T>(theta_raw[m * ldt + 1]);
        const float tx = d * tanh_x, ty = d * tanh_y;
        int x0 = 0, y0 = 0;
        float wx1 = 0.f, wy1 = 0.f;
        const bool in = locate(tx, ty, x, y, g.H, g.W, x0, y0, wx1, wy1);
        const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
        if (j == 0) {
            flow[2 * m] = tx;
            flow[2 * m + 1] = ty;
        }
        for (int v = j; v < g.nv; v += G) {
            const int c0 = v * 8;
            float v00[8], v01[8], v10[8], v11[8], hw[8], ac[8], au[8], dy[8], dc[8], du[8], gg[8];
            if (in) taps8(frame, g.H, g.W, g.C, c0, x0, y0, v00, v01, v10, v11);
            warp8(in, wx1, wy1, v00, v01, v10, v11, hw);
            load8<T>(a + m * lda + off_c + c0, ac);
            load8<T>(a + m * lda + off_u + c0, au);
            load8<float>(dh + m * g.C + c0, dy);
            if (dh2) {
                float d2[8];
                load8<float>(dh2 + m * g.C + c0, d2);
#pragma unroll
                for (int i = 0; i < 8; ++i) dy[i] += d2[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float u = gate_sigmoid<T>(au[i]), c = fmaxf(ac[i], 0.f);
                du[i] = ((dy[i] * (hw[i] - c)) * u) * (1.f - u);
                dc[i] = ac[i] > 0.f ? dy[i] * (1.f - u) : 0.f;
                gg[i] = dy[i] * u;
                if (in) {
                    const float ex = fmaf(wy1, v11[i] - v10[i], wy0 * (v01[i] - v00[i]));
                    const float ey = fmaf(wx1, v11[i] - v01[i], wx0 * (v10[i] - v00[i]));
                    sum_x = fmaf(gg[i], ex, sum_x);
                    sum_y = fmaf(gg[i], ey, sum_y);
                }
            }
            store8<T>(da + m * ldda + doff_c + c0, dc);
            store8<T>(da + m * ldda + doff_u + c0, du);
            store8<float>(gbuf + m * g.C + c0, gg);
        }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
        sum_x += __shfl_xor(sum_x, o, 64);
        sum_y += __shfl_xor(sum_y, o, 64);
    }
    if (live && j == 0) {
        stf<T>(dtheta_raw + m * lddt, (sum_x * d) * (1.f - tanh_x * tanh_x));
        stf<T>(dtheta_raw + m * lddt + 1, (sum_y * d) * (1.f - tanh_y * tanh_y));
    }
}

// Second launch: dh_prev = warp^T g (+ addend).  The thread owns 8 channels of source pixel q and visits the pixels p of the window
// |p - q|_inf <= R clipped to the frame, line by line; the weights are the forward's, recomputed from the stored flow.
__global__ __launch_bounds__(kThreads) void tsru_backward_warp_kernel(Geo g, int R, const float* gbuf, const float* flow,
                                                                      const float* addend, float* dh_prev) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= g.M * g.nv) return;
    const long long q = idx / g.nv;
    const int c0 = (int)(idx - q * g.nv) * 8;
    const int qx = (int)(q % g.W), qy = (int)((q / g.W) % g.H);
    const long long base = q - ((long long)qy * g.W + qx);            // first pixel of the frame
    const int ylo = max(qy - R, 0), yhi = min(qy + R, g.H - 1), xlo = max(qx - R, 0), xhi = min(qx + R, g.W - 1);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int py = ylo; py <= yhi; ++py) {
        for (int px = xlo; px <= xhi; ++px) {
            const long long p = base + (long long)py * g.W + px;
            int x0, y0;
            float wx1, wy1;
            if (!locate(flow[2 * p], flow[2 * p + 1], px, py, g.H, g.W, x0, y0, wx1, wy1)) continue;
            const int jx = qx - x0, jy = qy - y0;
            if ((unsigned)jx > 1u || (unsigned)jy > 1u) continue;
            const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
            const float w = (jy ? wy1 : wy0) * (jx ? wx1 : wx0);
            float gv[8];
            load8<float>(gbuf + p * g.C + c0, gv);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(w, gv[i], acc[i]);
        }
    }
    if (addend) {
        float ad[8];
        load8<float>(addend + q * g.C + c0, ad);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += ad[i];
    }
    store8<float>(dh_prev + q * g.C + c0, acc);
}

int refusal_shape(int dtype, float d, int B, int H, int W, int C) {
    if ((dtype != DVD_F32 && dtype != DVD_BF16) || B < 1 || H < 1 || W < 1 || C < 1) return DVD_E_ARG;
    if (!(d > 0.f && d <= (float)DVDX_TSRU_MAX_FLOW)) return DVD_E_ARG;
    if (C % 8 || H > DVDX_TSRU_MAX_SIDE || W > DVDX_TSRU_MAX_SIDE) return DVD_E_SHAPE;
    if ((long long)B * H * W * C > 0x7fffffffll) return DVD_E_SHAPE;
    return DVD_OK;
}

// a [rows][ld] tensor read or written at columns [off, off + C)
int refusal_window(int ld, int off, int C) {
    if (ld < 1 || off < 0) return DVD_E_ARG;
    if (ld % 8 || off % 8 || (long long)off + C > ld) return DVD_E_SHAPE;
    return DVD_OK;
}

Geo geo_of(int B, int H, int W, int C) { return Geo{H, W, C, C / 8, (long long)B * H * W}; }

// workgroup size and count of a launch of `threads` threads
void shape_of(long long threads, unsigned& block, unsigned& grid) {
    block = threads < kSmallLaunch ? 64u : (unsigned)kThreads;
    grid = cdiv(threads, block);
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvdx_tsru_abi_version(void) { return DVDX_TSRU_ABI_VERSION; }

extern "C" const char* dvdx_tsru_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG: return "null pointer, output aliasing an input, unknown dtype, non-positive size, negative offset or flow range outside (0, 8]";
    case DVD_E_SHAPE: return "unsupported shape: channels, row stride or offset no multiple of 8, window outside the row, H or W above 1024 or more than 2^31 - 1 elements";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" int dvdx_tsru_forward(int dtype, const float* h_prev, const void* a, int lda, int off_c, int off_u, const float* theta_raw,
                                 int ldt, float d, float* h, void* h_c, int B, int H, int W, int C, void* stream) {
    if (!h_prev || !a || !theta_raw || !h || h == h_prev || ldt < 2) return DVD_E_ARG;
    int bad = refusal_shape(dtype, d, B, H, W, C);
    if (bad == DVD_OK) bad = refusal_window(lda, off_c, C);
    if (bad == DVD_OK) bad = refusal_window(lda, off_u, C);
    if (bad != DVD_OK) return bad;
    const Geo g = geo_of(B, H, W, C);
    unsigned block, grid;
    shape_of(g.M * g.nv, block, grid);
    if (dtype == DVD_F32)
        tsru_forward_kernel<float><<<grid, block, 0, S_>>>(g, h_prev, (const float*)a, lda, off_c, off_u, theta_raw, ldt, d, h, (float*)h_c);
    else
        tsru_forward_kernel<bf16_t><<<grid, block, 0, S_>>>(g, h_prev, (const bf16_t*)a, lda, off_c, off_u, theta_raw, ldt, d, h, (bf16_t*)h_c);
    return launch_status();
}

extern "C" int dvdx_tsru_backward(int dtype, const float* dh, const float* dh2, const float* h_prev, const void* a, int lda, int off_c,
                                  int off_u, const float* theta_raw, int ldt, float d, void* da, int ldda, int doff_c, int doff_u,
                                  void* dtheta_raw, int lddt, const float* addend, float* dh_prev, float* ws, int B, int H, int W, int C,
                                  void* stream) {
    if (!dh || !h_prev || !a || !theta_raw || !da || !dtheta_raw || !dh_prev || !ws || dh_prev == dh || dh_prev == dh2 ||
        dh_prev == h_prev || ldt < 2 || lddt < 2)
        return DVD_E_ARG;
    int bad = refusal_shape(dtype, d, B, H, W, C);
    if (bad == DVD_OK) bad = refusal_window(lda, off_c, C);
    if (bad == DVD_OK) bad = refusal_window(lda, off_u, C);
    if (bad == DVD_OK) bad = refusal_window(ldda, doff_c, C);
    if (bad == DVD_OK) bad = refusal_window(ldda, doff_u, C);
    if (bad != DVD_OK) return bad;
    const Geo g = geo_of(B, H, W, C);
    float* gbuf = ws;
    float* flow = ws + g.M * g.C;
    int G = 1;
    while (G < g.nv && G < 64) G <<= 1;
    unsigned block, grid;
    shape_of(g.M * G, block, grid);
    if (dtype == DVD_F32)
        tsru_backward_gates_kernel<float><<<grid, block, 0, S_>>>(g, G, dh, dh2, h_prev, (const float*)a, lda, off_c, off_u, theta_raw,
                                                                  ldt, d, (float*)da, ldda, doff_c, doff_u, (float*)dtheta_raw, lddt,
                                                                  gbuf, flow);
    else
        tsru_backward_gates_kernel<bf16_t><<<grid, block, 0, S_>>>(g, G, dh, dh2, h_prev, (const bf16_t*)a, lda, off_c, off_u, theta_raw,
                                                                   ldt, d, (bf16_t*)da, ldda, doff_c, doff_u, (bf16_t*)dtheta_raw,
                                                                   lddt, gbuf, flow);
    if (hipGetLastError() != hipSuccess) return DVD_E_LAUNCH;
    shape_of(g.M * g.nv, block, grid);
    tsru_backward_warp_kernel<<<grid, block, 0, S_>>>(g, (int)ceilf(d), gbuf, flow, addend, dh_prev);
    return launch_status();
}
