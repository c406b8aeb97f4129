// dvd_geom_clip_forward / dvd_geom_clip_backward (include/dvdgan_hip_geom.h), built into libdvdgan_hip_geom.so: a clip-consistent
// affine warp of fp32 frames (bilinear, zero fill) and the transpose of that map.  Memory-bound gathers: one thread per pixel and
// all three channels, consecutive lanes on consecutive pixels of a line, so every store is a coalesced run and the loads of a wave
// fall on a few neighbouring lines of one frame (L2 serves the overlap).  The row is wave-uniform: the identity test is a uniform
// branch.  The backward pass owns each dx element in one thread and walks a window of output pixels in a fixed order, recomputing
// every weight with the forward's expression: no atomics, no scratch, no LDS.
#include "../common.h"
#include "../../../include/dvdgan_hip_geom.h"

// every multiply-add below is written as fmaf or as separate operations: the forward's and the backward's weights must be the same
// bits, whichever way the compiler would have contracted either
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = DVD_GEOM_THREADS;

struct Row {
    float a00, a01, a02, a10, a11, a12;
    bool identity;
};

__device__ __forceinline__ float uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ Row load_row(const float* p) {
    Row r;
    r.a00 = uniform(p[DVD_GEOM_A00]); r.a01 = uniform(p[DVD_GEOM_A01]); r.a02 = uniform(p[DVD_GEOM_A02]);
    r.a10 = uniform(p[DVD_GEOM_A10]); r.a11 = uniform(p[DVD_GEOM_A11]); r.a12 = uniform(p[DVD_GEOM_A12]);
    r.identity = r.a00 == 1.f && r.a01 == 0.f && r.a02 == 0.f && r.a10 == 0.f && r.a11 == 1.f && r.a12 == 0.f;
    return r;
}

// The source position of output pixel (x, y) and its bilinear cell: false when the pixel takes no part (the position is not
// finite or outside (-1, W) x (-1, H)); only a position that passed that test is converted to an integer.  x0 in [-1, W - 1],
// y0 in [-1, H - 1].  The one expression both directions use.
__device__ __forceinline__ bool locate(const Row& r, int x, int y, int H, int W, int& x0, int& y0, float& wx1, float& wy1) {
    const float sx = fmaf(r.a01, (float)y, fmaf(r.a00, (float)x, r.a02));
    const float sy = fmaf(r.a11, (float)y, fmaf(r.a10, (float)x, r.a12));
    if (!(sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H)) return false;
    const float fx = floorf(sx), fy = floorf(sy);
    x0 = (int)fx;
    y0 = (int)fy;
    wx1 = sx - fx;
    wy1 = sy - fy;
    return true;
}

// the pixels of a frame this thread owns: q = first, first + stride, ... below H * W
#define FOR_OWN_PIXELS(q, HW) for (int q = blockIdx.y * kThreads + threadIdx.x; q < (HW); q += gridDim.y * kThreads)

__global__ __launch_bounds__(kThreads) void geom_forward_kernel(const float* x, float* y, const float* mats, int frames_per_clip,
                                                                int H, int W) {
    const int n = blockIdx.x, HW = H * W;
    const Row r = load_row(mats + (size_t)(n / frames_per_clip) * DVD_GEOM_COLS);
    const float* xf = x + (size_t)n * 3 * HW;
    float* yf = y + (size_t)n * 3 * HW;
    if (r.identity) {
        FOR_OWN_PIXELS(q, HW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) yf[c * HW + q] = xf[c * HW + q];
        }
        return;
    }
    FOR_OWN_PIXELS(q, HW) {
        const int py = q / W, px = q - py * W;
        float o[3] = {0.f, 0.f, 0.f};
        int x0, y0;
        float wx1, wy1;
        if (locate(r, px, py, H, W, x0, y0, wx1, wy1)) {
            // x0 + 1 <= W and y0 + 1 <= H: a neighbour is read only where its column and its line are inside the frame
            const bool l = x0 >= 0, rgt = x0 + 1 < W, t = y0 >= 0, b = y0 + 1 < H;
            const int i00 = y0 * W + x0;
            if (wx1 == 0.f && wy1 == 0.f) {
                if (l && t) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = xf[c * HW + i00];
                }
            } else {
                const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
                const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* f = xf + c * HW;
                    const float v00 = t && l ? f[i00] : 0.f, v01 = t && rgt ? f[i00 + 1] : 0.f;
                    const float v10 = b && l ? f[i00 + W] : 0.f, v11 = b && rgt ? f[i00 + W + 1] : 0.f;
                    o[c] = fmaf(w11, v11, fmaf(w10, v10, fmaf(w01, v01, w00 * v00)));
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) yf[c * HW + q] = o[c];
    }
}

// clamp a window bound to [0, side - 1] as an int; v is finite here
__device__ __forceinline__ int bound(double v, int side) { return (int)fmin(fmax(v, 0.0), (double)(side - 1)); }

__global__ __launch_bounds__(kThreads) void geom_backward_kernel(const float* g, float* dx, const float* mats, int frames_per_clip,
                                                                 int H, int W) {
    const int n = blockIdx.x, HW = H * W;
    const Row r = load_row(mats + (size_t)(n / frames_per_clip) * DVD_GEOM_COLS);
    const float* gf = g + (size_t)n * 3 * HW;
    float* df = dx + (size_t)n * 3 * HW;
    if (r.identity) {
        FOR_OWN_PIXELS(q, HW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) df[c * HW + q] = gf[c * HW + q];
        }
        return;
    }
    // the row's inverse in fp64 (the products of two floats are exact there) and the half sides of the pre-image's bounding box
    const double a00 = r.a00, a01 = r.a01, a10 = r.a10, a11 = r.a11;
    const double det = a00 * a11 - a01 * a10;
    const double i00 = a11 / det, i01 = -a01 / det, i10 = -a10 / det, i11 = a00 / det;
    const double ux = 1.0 + 0x1p-20 * (fabs(a00) * W + fabs(a01) * H + fabs((double)r.a02) + 1.0);
    const double uy = 1.0 + 0x1p-20 * (fabs(a10) * W + fabs(a11) * H + fabs((double)r.a12) + 1.0);
    const double ex = fabs(i00) * ux + fabs(i01) * uy, ey = fabs(i10) * ux + fabs(i11) * uy;
    const bool whole = !(fabs(ex) < 1e300 && fabs(ey) < 1e300);            // false for a NaN too
    FOR_OWN_PIXELS(q, HW) {
        const int qy = q / W, qx = q - qy * W;
        int xlo = 0, xhi = W - 1, ylo = 0, yhi = H - 1;
        if (!whole) {
            const double tx = (double)qx - (double)r.a02, ty = (double)qy - (double)r.a12;
            const double cx = i00 * tx + i01 * ty, cy = i10 * tx + i11 * ty;
            const double lx = ceil(cx - ex), hx = floor(cx + ex), ly = ceil(cy - ey), hy = floor(cy + ey);
            if (fabs(cx) < 1e300 && fabs(cy) < 1e300) {
                if (hx < 0.0 || lx > (double)(W - 1) || hy < 0.0 || ly > (double)(H - 1)) {
                    xhi = -1;              // the pre-image misses the frame: nothing to visit
                } else {
                    xlo = bound(lx, W); xhi = bound(hx, W); ylo = bound(ly, H); yhi = bound(hy, H);
                }
            }
        }
        float acc[3] = {0.f, 0.f, 0.f};
        for (int py = ylo; py <= yhi; ++py) {
            for (int px = xlo; px <= xhi; ++px) {
                int x0, y0;
                float wx1, wy1;
                if (!locate(r, px, py, H, W, x0, y0, wx1, wy1)) continue;
                const int jx = qx - x0, jy = qy - y0;
                if ((unsigned)jx > 1u || (unsigned)jy > 1u) continue;
                const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
                const float w = (jy ? wy1 : wy0) * (jx ? wx1 : wx0);
                const int i = py * W + px;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = fmaf(w, gf[c * HW + i], acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) df[c * HW + q] = acc[c];
    }
}

int refusal(const void* x, const void* y, const void* mats, long long n_frames, int frames_per_clip, int H, int W) {
    if (!x || !y || !mats || x == y || n_frames < 0 || frames_per_clip < 1) return DVD_E_ARG;
    if (H < 1 || H > DVD_GEOM_MAX_SIDE || W < 1 || W > DVD_GEOM_MAX_SIDE || n_frames > DVD_GEOM_MAX_FRAMES) return DVD_E_SHAPE;
    return DVD_OK;
}

// frames x chunks of a frame's pixels; a launch holds fewer than 2^32 threads, so many frames get fewer chunks each
dim3 grid_of(long long n_frames, int H, int W) {
    const long long want = ((long long)H * W + kThreads - 1) / kThreads, room = ((1ll << 24) - 1) / n_frames;
    long long gy = want < room ? want : room;
    gy = gy < 1 ? 1 : gy > 65535 ? 65535 : gy;
    return dim3((unsigned)n_frames, (unsigned)gy, 1);
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvd_geom_abi_version(void) { return DVD_GEOM_ABI_VERSION; }

extern "C" const char* dvd_geom_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG: return "null pointer, output aliasing the input, negative frame count or frames_per_clip < 1";
    case DVD_E_SHAPE: return "unsupported shape: H or W outside [1, 4096] or more than 16777215 frames";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" int dvd_geom_clip_forward(const float* x, float* y, const float* mats, long long n_frames, int frames_per_clip, int H,
                                     int W, void* stream) {
    const int bad = refusal(x, y, mats, n_frames, frames_per_clip, H, W);
    if (bad != DVD_OK || n_frames == 0) return bad;
    geom_forward_kernel<<<grid_of(n_frames, H, W), kThreads, 0, S_>>>(x, y, mats, frames_per_clip, H, W);
    return launch_status();
}

extern "C" int dvd_geom_clip_backward(const float* g, float* dx, const float* mats, long long n_frames, int frames_per_clip, int H,
                                      int W, void* stream) {
    const int bad = refusal(g, dx, mats, n_frames, frames_per_clip, H, W);
    if (bad != DVD_OK || n_frames == 0) return bad;
    geom_backward_kernel<<<grid_of(n_frames, H, W), kThreads, 0, S_>>>(g, dx, mats, frames_per_clip, H, W);
    return launch_status();
}
