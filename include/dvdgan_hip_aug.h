/*
 * dvdgan_hip_aug.h -- C ABI of libdvdgan_hip_aug.so: clip-consistent differentiable augmentation of what the discriminators see
 * (Zhao et al. 2020, "DiffAugment": colour, translation, cutout), forward and backward.  A library of its own beside
 * libdvdgan_hip.so, libdvdgan_hip_adv.so, libdvdgan_hip_eval.so and libdvdgan_hip_prdc.so (whose sets of entry points are fixed):
 * same conventions -- plain C, device pointers + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never
 * synchronises, return value 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide
 * state.  Every argument is checked before anything touches the device.
 *
 * Frames are fp32 [n_frames][3][H][W], contiguous.  Frame n belongs to clip n / frames_per_clip and every frame of a clip is
 * transformed by the same row of `params`, fp32 [clips][DVD_AUG_COLS] on the device: b, s, c, dx, dy, cy0, cx0, ch, cw (the last
 * six hold integers; they are clamped to +-DVD_AUG_MAX_SIDE before use, a NaN counts as the lower end).  Per frame, in this order:
 *   brightness   y0 = x + b
 *   saturation   m1[h][w] = (y0[0] + y0[1] + y0[2]) * (1/3),  y1 = (y0 - m1) * s + m1
 *   contrast     m2 = (float)(S / (3 H W) + (double)b), S the fp64 sum of the frame's x;  y2 = (y1 - m2) * c + m2
 *   translation  y3[c][h][w] = y2[c][h - dy][w - dx] where that source lies inside the frame, else 0
 *   cutout       y4 = 0 for cy0 <= h < cy0 + ch and cx0 <= w < cx0 + cw (the rectangle may stick out of the frame), else y3
 * A stage whose parameter is the identity (b == 0, s == 1, c == 1, dx == dy == 0, ch == 0 or cw == 0) is skipped, not computed:
 * a clip with the row 0, 1, 1, 0, 0, 0, 0, 0, 0 comes out bit-equal to its input.
 * The backward pass is the transpose (the map is affine in x).  With g the incoming gradient:
 *   g2[c][q] = g[c][q + d] where q + d lies inside the frame and outside the cutout, else 0
 *   dy1 = c * g2 + (1 - c) * (float)(sum(g2) / (3 H W))        (the sum per frame, in fp64)
 *   dx  = s * dy1 + (1 - s) * ((dy1[0] + dy1[1] + dy1[2]) * (1/3))
 *
 * One workgroup of DVD_AUG_THREADS threads per frame.  The fp64 sum runs only when c != 1: thread t adds the elements of the
 * four-element groups t, t + 256, ... of the frame in index order, the waves add their lanes in a fixed shuffle tree and the four
 * wave sums are added in order -- the same order whether the loads are 16 bytes wide or not, so the result of a frame is a
 * function of that frame and its row alone: no atomics, two launches give the same bits, and a frame gives the same bits alone
 * and inside a batch.  16-byte loads and stores are used where W % 4 == 0 and both bases are 16-byte aligned.
 */
#ifndef DVDGAN_HIP_AUG_H
#define DVDGAN_HIP_AUG_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVD_AUG_ABI_VERSION 1
#define DVD_AUG_COLS 9               /* floats of a parameter row */
#define DVD_AUG_B 0
#define DVD_AUG_S 1
#define DVD_AUG_C 2
#define DVD_AUG_DX 3
#define DVD_AUG_DY 4
#define DVD_AUG_CY0 5
#define DVD_AUG_CX0 6
#define DVD_AUG_CH 7
#define DVD_AUG_CW 8
#define DVD_AUG_MAX_SIDE 4096        /* largest H and W */
#define DVD_AUG_THREADS 256          /* threads of the workgroup that owns a frame */
#define DVD_AUG_MAX_FRAMES 16777215  /* frames of one call: a launch holds fewer than 2^32 threads */

/* DVD_AUG_ABI_VERSION of the build */
int dvd_aug_abi_version(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvd_aug_strerror(int code);

/* y <- the transform of x.  x, y [n_frames][3][H][W] fp32; params [ceil(n_frames / frames_per_clip)][DVD_AUG_COLS] fp32.
 * DVD_E_ARG: null x / y / params, x == y (the kernel gathers: in place is wrong), n_frames < 0, frames_per_clip < 1.
 * DVD_E_SHAPE: H or W outside [1, DVD_AUG_MAX_SIDE], n_frames above DVD_AUG_MAX_FRAMES.  n_frames == 0 succeeds and launches nothing. */
int dvd_aug_clip_forward(const float* x, float* y, const float* params, long long n_frames, int frames_per_clip, int H, int W,
                         void* stream);

/* dx <- the transpose of the transform applied to g (same shapes, same params, same refusals with g / dx for x / y). */
int dvd_aug_clip_backward(const float* g, float* dx, const float* params, long long n_frames, int frames_per_clip, int H, int W,
                          void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
