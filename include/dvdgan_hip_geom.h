/*
 * dvdgan_hip_geom.h -- C ABI of libdvdgan_hip_geom.so: clip-consistent geometric augmentation of what the discriminators see
 * (the geometric group of Karras et al. 2020, "ADA": mirror, quarter turns, scaling, rotation -- any affine map), a bilinear warp
 * with zero fill, forward and backward.  A library of its own beside libdvdgan_hip.so, libdvdgan_hip_adv.so,
 * libdvdgan_hip_eval.so, libdvdgan_hip_prdc.so and libdvdgan_hip_aug.so (whose sets of entry points are fixed): same conventions --
 * plain C, device pointers + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, return value
 * 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide state.  Every argument is
 * checked before anything touches the device.
 *
 * Frames are fp32 [n_frames][3][H][W], contiguous.  Frame n belongs to clip n / frames_per_clip and every frame of a clip is
 * warped by the same row of `mats`, fp32 [clips][DVD_GEOM_COLS] on the device: a00, a01, a02, a10, a11, a12.  A row maps the
 * index (x, y) of an OUTPUT pixel (x the column, y the line) to a source position in pixel units, in exactly these operations:
 *   sx = fmaf(a01, (float)y, fmaf(a00, (float)x, a02))
 *   sy = fmaf(a11, (float)y, fmaf(a10, (float)x, a12))
 * The pixel takes part only when sx lies in (-1, W) and sy in (-1, H) -- a test a NaN and an infinity fail -- and only then is
 * anything converted to an integer:
 *   x0 = (int)floorf(sx), wx1 = sx - floorf(sx), wx0 = 1 - wx1        (y0, wy1, wy0 likewise; x0 in [-1, W - 1])
 *   w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1
 * Forward, per channel c, with v(j, i) = x[c][j][i] inside the frame and 0 outside (the fill is zero):
 *   y[c][y][x] = fmaf(w11, v(y0 + 1, x0 + 1), fmaf(w10, v(y0 + 1, x0), fmaf(w01, v(y0, x0 + 1), w00 * v(y0, x0))))
 * and y[c][y][x] = v(y0, x0) itself when wx1 == 0 and wy1 == 0 (integer positions: mirrors and quarter turns move bits);
 * a pixel that takes no part is 0.  One set of weights serves the three channels.
 * Backward: the transpose.  dx[c][qy][qx] is owned by one thread, which visits the output pixels (x, y) of a window line by line
 * (y ascending, within a line x ascending), recomputes sx, sy, x0, y0 and the weights of each by the expressions above, and where
 * qx - x0 and qy - y0 are both 0 or 1 adds the matching weight's term:  acc = fmaf(w, g[c][y][x], acc), acc starting at 0.  The
 * weights of the transpose are therefore the forward's to the bit, the order of the sum is fixed, and there is no atomic.
 * The window is the bounding box of the pre-image of (qx, qy) + [-1 - s, 1 + s]^2 under the row, computed in fp64 from the row's
 * inverse (s = 2^-20 (|a00| W + |a01| H + |a02| + 1) for sx, likewise for sy: sixteen times the rounding error of sx) and clipped
 * to the frame; a row whose inverse is not finite (a singular one, a NaN) makes it the whole frame, which is slow and correct.
 * The window decides only which output pixels are LOOKED AT: each of them passes the test above before anything is indexed, so
 * no table can make either kernel read or write outside its tensors.
 * The identity row 1, 0, 0, 0, 1, 0 is skipped, not computed: its frames are copied bit for bit, in both directions.
 *
 * One thread per pixel and all three channels; DVD_GEOM_THREADS threads per workgroup; a result is a function of its frame and
 * its row alone: two launches give the same bits, and a frame gives the same bits alone and inside a batch.
 */
#ifndef DVDGAN_HIP_GEOM_H
#define DVDGAN_HIP_GEOM_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVD_GEOM_ABI_VERSION 1
#define DVD_GEOM_COLS 6               /* floats of a row */
#define DVD_GEOM_A00 0
#define DVD_GEOM_A01 1
#define DVD_GEOM_A02 2
#define DVD_GEOM_A10 3
#define DVD_GEOM_A11 4
#define DVD_GEOM_A12 5
#define DVD_GEOM_MAX_SIDE 4096        /* largest H and W */
#define DVD_GEOM_THREADS 256          /* threads of a workgroup */
#define DVD_GEOM_MAX_FRAMES 16777215  /* frames of one call */

/* DVD_GEOM_ABI_VERSION of the build */
int dvd_geom_abi_version(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvd_geom_strerror(int code);

/* y <- the warp of x.  x, y [n_frames][3][H][W] fp32; mats [ceil(n_frames / frames_per_clip)][DVD_GEOM_COLS] fp32.
 * DVD_E_ARG: null x / y / mats, x == y (the kernel gathers: in place is wrong), n_frames < 0, frames_per_clip < 1.
 * DVD_E_SHAPE: H or W outside [1, DVD_GEOM_MAX_SIDE], n_frames above DVD_GEOM_MAX_FRAMES.  n_frames == 0 succeeds and launches nothing. */
int dvd_geom_clip_forward(const float* x, float* y, const float* mats, long long n_frames, int frames_per_clip, int H, int W,
                          void* stream);

/* dx <- the transpose of the warp applied to g (same shapes, same mats, same refusals with g / dx for x / y). */
int dvd_geom_clip_backward(const float* g, float* dx, const float* mats, long long n_frames, int frames_per_clip, int H, int W,
                           void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
