// dvd_aug_clip_forward / dvd_aug_clip_backward (include/dvdgan_hip_aug.h), built into libdvdgan_hip_aug.so: clip-consistent
// brightness / saturation / contrast / translation / cutout of fp32 frames and the transpose of that map.  Memory-bound: one
// workgroup of 256 threads per frame; sweep 1 (only when contrast is on) is the frame's fp64 sum, sweep 2 owns every output
// pixel once, reads the three channel values of its source pixel and writes the three results -- 16 bytes per lane and channel
// where W % 4 == 0.  The parameter row is wave-uniform, so every stage skip is a uniform branch.  No atomics, no scratch, four
// doubles of LDS.
#include "../common.h"
#include "../../../include/dvdgan_hip_aug.h"

// every multiply-add below is written as fmaf or as separate operations: the bits must not depend on which instance of an
// inlined function the compiler chose to contract (the 16-byte and the dword path must agree to the bit)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = DVD_AUG_THREADS;
constexpr float kThird = 1.f / 3.f;

struct Row {
    float b, s, c;
    int dx, dy, cy0, cx0, cy1, cx1;      // the cutout is rows [cy0, cy1) x columns [cx0, cx1)
    bool shift, cut;
};

// an integer-valued float of the table -> int, clamped so that no later sum of two of them overflows (a NaN gives the lower end)
__device__ __forceinline__ int table_int(float v) {
    const float m = (float)(2 * DVD_AUG_MAX_SIDE);
    return __builtin_amdgcn_readfirstlane((int)fminf(fmaxf(v, -m), m));
}
__device__ __forceinline__ float uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ Row load_row(const float* p) {
    Row r;
    r.b = uniform(p[DVD_AUG_B]);
    r.s = uniform(p[DVD_AUG_S]);
    r.c = uniform(p[DVD_AUG_C]);
    r.dx = table_int(p[DVD_AUG_DX]);
    r.dy = table_int(p[DVD_AUG_DY]);
    r.cy0 = table_int(p[DVD_AUG_CY0]);
    r.cx0 = table_int(p[DVD_AUG_CX0]);
    const int ch = max(table_int(p[DVD_AUG_CH]), 0), cw = max(table_int(p[DVD_AUG_CW]), 0);
    r.cy1 = r.cy0 + ch;
    r.cx1 = r.cx0 + cw;
    r.shift = r.dx != 0 || r.dy != 0;
    r.cut = ch != 0 && cw != 0;
    return r;
}

__device__ __forceinline__ bool in_cut(const Row& r, int h, int w) {
    return r.cut && h >= r.cy0 && h < r.cy1 && w >= r.cx0 && w < r.cx1;
}

// fp64 sum of the n3 = 3 H W floats of a frame, broadcast.  Thread t owns the four-element groups t, t + 256, ... and adds their
// elements in index order -- VEC only widens the load.  MASKED (the backward pass): an element at (h, w) counts when it lies
// outside the cutout and (h - dy, w - dx) lies inside the frame, i.e. when the transform's output there came from a pixel.
template <bool VEC, bool MASKED>
__device__ __forceinline__ double frame_sum(const float* f, int n3, int H, int W, const Row& r, double* part) {
    double acc = 0.0;
    const int HW = H * W, ngroups = (n3 + 3) >> 2;
    for (int q = threadIdx.x; q < ngroups; q += kThreads) {
        const int i = q << 2;
        float v[4];
        if (VEC) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(f + i);
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = i + j < n3 ? f[i + j] : 0.f;
        }
        if (MASKED) {
            const int pix = i % HW;
            int h = pix / W, w = pix - h * W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int sh = h - r.dy, sw = w - r.dx;
                if (in_cut(r, h, w) || sh < 0 || sh >= H || sw < 0 || sw >= W) v[j] = 0.f;
                if (++w == W) { w = 0; if (++h == H) h = 0; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (VEC || i + j < n3) acc += (double)v[j];
    }
    acc = wave_sum_d(acc);
    __syncthreads();                                  // a second sum in one launch would reuse part[]
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// the colour stages of one pixel, in the documented order
__device__ __forceinline__ void colour(float& v0, float& v1, float& v2, const Row& r, float m2) {
    if (r.b != 0.f) { v0 += r.b; v1 += r.b; v2 += r.b; }
    if (r.s != 1.f) {
        const float m1 = ((v0 + v1) + v2) * kThird;
        v0 = fmaf(v0 - m1, r.s, m1); v1 = fmaf(v1 - m1, r.s, m1); v2 = fmaf(v2 - m1, r.s, m1);
    }
    if (r.c != 1.f) { v0 = fmaf(v0 - m2, r.c, m2); v1 = fmaf(v1 - m2, r.c, m2); v2 = fmaf(v2 - m2, r.c, m2); }
}

// ... and their transpose: km = (1 - c) * mean(g2)
__device__ __forceinline__ void colour_t(float& v0, float& v1, float& v2, const Row& r, float km) {
    if (r.c != 1.f) { v0 = fmaf(r.c, v0, km); v1 = fmaf(r.c, v1, km); v2 = fmaf(r.c, v2, km); }
    if (r.s != 1.f) {
        const float ms = (1.f - r.s) * (((v0 + v1) + v2) * kThird);
        v0 = fmaf(r.s, v0, ms); v1 = fmaf(r.s, v1, ms); v2 = fmaf(r.s, v2, ms);
    }
}

// Sweep 2 of both directions over NP = 4 (VEC) or 1 consecutive pixels of a row per thread and iteration.
// Forward: the output pixel (h, w) takes the source pixel (h - dy, w - dx); outside the frame or inside the cutout it is 0.
// Backward: the input pixel (h, w) collects from the gradient pixel (h + dy, w + dx), which counts as 0 outside the frame or
// inside the cutout, and the colour stages' transpose runs on every pixel.
template <bool VEC, bool BACKWARD>
__device__ __forceinline__ void sweep(const float* src, float* dst, int H, int W, const Row& r, float m) {
    constexpr int NP = VEC ? 4 : 1;
    const int HW = H * W, nrun = HW / NP;
    const int oy = BACKWARD ? r.dy : -r.dy, ox = BACKWARD ? r.dx : -r.dx;
    for (int q = threadIdx.x; q < nrun; q += kThreads) {
        const int p = q * NP, h = p / W, w = p - h * W;
        const int sh = h + oy, sw = w + ox;
        float a[3][NP];
        bool live[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            live[j] = sh >= 0 && sh < H && sw + j >= 0 && sw + j < W && !in_cut(r, BACKWARD ? sh : h, BACKWARD ? sw + j : w + j);
            a[0][j] = a[1][j] = a[2][j] = 0.f;
        }
        bool any = false;
#pragma unroll
        for (int j = 0; j < NP; ++j) any = any || live[j];
        if (any) {
            // (signed: sw may be negative.  Row sh exists here; every load checks its column)
            const ptrdiff_t off = (ptrdiff_t)sh * W + sw;
            if (VEC && !(ox & 3) && sw >= 0 && sw + 3 < W) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(src + (off + (ptrdiff_t)c * HW));
                    a[c][0] = t[0]; a[c][1] = t[1]; a[c][2] = t[2]; a[c][3] = t[3];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < NP; ++j)
                        if (sw + j >= 0 && sw + j < W) a[c][j] = src[off + (ptrdiff_t)c * HW + j];
            }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            if (BACKWARD) {
                if (!live[j]) a[0][j] = a[1][j] = a[2][j] = 0.f;
                colour_t(a[0][j], a[1][j], a[2][j], r, m);
            } else {
                colour(a[0][j], a[1][j], a[2][j], r, m);
                if (!live[j]) a[0][j] = a[1][j] = a[2][j] = 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = dst + (size_t)c * HW + p;
            if (VEC) {
                const f32x4 t = {a[c][0], a[c][1], a[c][2], a[c][3]};
                *reinterpret_cast<f32x4*>(d) = t;
            } else {
                d[0] = a[c][0];
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void aug_forward_kernel(const float* x, float* y, const float* params, int frames_per_clip,
                                                               int H, int W) {
    __shared__ double part[4];
    const int n = blockIdx.x, n3 = 3 * H * W;
    const Row r = load_row(params + (size_t)(n / frames_per_clip) * DVD_AUG_COLS);
    const float* xf = x + (size_t)n * n3;
    float m2 = 0.f;
    if (r.c != 1.f) m2 = (float)(frame_sum<VEC, false>(xf, n3, H, W, r, part) / (double)n3 + (double)r.b);
    sweep<VEC, false>(xf, y + (size_t)n * n3, H, W, r, m2);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void aug_backward_kernel(const float* g, float* dx, const float* params, int frames_per_clip,
                                                                int H, int W) {
    __shared__ double part[4];
    const int n = blockIdx.x, n3 = 3 * H * W;
    const Row r = load_row(params + (size_t)(n / frames_per_clip) * DVD_AUG_COLS);
    const float* gf = g + (size_t)n * n3;
    float km = 0.f;
    if (r.c != 1.f) {
        const double S = (r.shift || r.cut) ? frame_sum<VEC, true>(gf, n3, H, W, r, part) : frame_sum<VEC, false>(gf, n3, H, W, r, part);
        km = (1.f - r.c) * (float)(S / (double)n3);
    }
    sweep<VEC, true>(gf, dx + (size_t)n * n3, H, W, r, km);
}

int refusal(const void* x, const void* y, const void* params, long long n_frames, int frames_per_clip, int H, int W) {
    if (!x || !y || !params || x == y || n_frames < 0 || frames_per_clip < 1) return DVD_E_ARG;
    if (H < 1 || H > DVD_AUG_MAX_SIDE || W < 1 || W > DVD_AUG_MAX_SIDE || n_frames > DVD_AUG_MAX_FRAMES) return DVD_E_SHAPE;
    return DVD_OK;
}

bool wide(const void* x, const void* y, int W) { return W % 4 == 0 && ((uintptr_t)x | (uintptr_t)y) % 16 == 0; }

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvd_aug_abi_version(void) { return DVD_AUG_ABI_VERSION; }

extern "C" const char* dvd_aug_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG: return "null pointer, output aliasing the input, negative frame count or frames_per_clip < 1";
    case DVD_E_SHAPE: return "unsupported shape: H or W outside [1, 4096] or more than 16777215 frames";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" int dvd_aug_clip_forward(const float* x, float* y, const float* params, long long n_frames, int frames_per_clip, int H,
                                    int W, void* stream) {
    const int bad = refusal(x, y, params, n_frames, frames_per_clip, H, W);
    if (bad != DVD_OK || n_frames == 0) return bad;
    if (wide(x, y, W)) aug_forward_kernel<true><<<(unsigned)n_frames, kThreads, 0, S_>>>(x, y, params, frames_per_clip, H, W);
    else aug_forward_kernel<false><<<(unsigned)n_frames, kThreads, 0, S_>>>(x, y, params, frames_per_clip, H, W);
    return launch_status();
}

extern "C" int dvd_aug_clip_backward(const float* g, float* dx, const float* params, long long n_frames, int frames_per_clip, int H,
                                     int W, void* stream) {
    const int bad = refusal(g, dx, params, n_frames, frames_per_clip, H, W);
    if (bad != DVD_OK || n_frames == 0) return bad;
    if (wide(g, dx, W)) aug_backward_kernel<true><<<(unsigned)n_frames, kThreads, 0, S_>>>(g, dx, params, frames_per_clip, H, W);
    else aug_backward_kernel<false><<<(unsigned)n_frames, kThreads, 0, S_>>>(g, dx, params, frames_per_clip, H, W);
    return launch_status();
}
