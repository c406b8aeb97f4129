/*
 * dvdgan_hip_prdc.h -- C ABI of libdvdgan_hip_prdc.so: the k-nearest-neighbour manifold statistics of sample features (improved
 * precision / recall, Kynkaanniemi et al. 2019; density / coverage, Naeem et al. 2020).  The feature extractor is the caller's.
 * A library of its own beside libdvdgan_hip.so, libdvdgan_hip_adv.so and libdvdgan_hip_eval.so (whose sets of entry points are
 * fixed): same conventions -- plain C, device pointers + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never
 * synchronises, return value 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide
 * state.  Every argument is checked before anything touches the device.
 *
 * The distance.  With a pivot c (fp32 [d], NULL = zeros) let y = fl32(x - c).  For two rows a, b
 *   d2(a, b) = max(0, |y_a|^2 + |y_b|^2 - 2 dot(y_a, y_b))
 * where the norms are fp64 sums, in k order, of the squares of the fp32 y; dot runs on v_mfma_f32_32x32x2_f32 with fp32
 * accumulators and k in order; the combination and every comparison are fp64.  (Centring matters: the rounding error of dot is
 * proportional to |y_a||y_b|, which a pivot near the data's mean keeps at the size of the spread instead of the offset.)
 * A comparison of two distances, or of a distance with a radius, is therefore decided up to the rounding of dot:
 * 2 (d + 2) 2^-24 |y_a|.|y_b| to first order.  The n x m matrix of distances is never stored.
 *
 * Deterministic: every output element is written by one thread, every sum has a fixed order, the k-th smallest of a multiset
 * does not depend on the order in which its members are visited, and how the work is split over workgroups is a fixed function
 * of the shapes (no atomics): two runs on the same inputs give the same bits.
 */
#ifndef DVDGAN_HIP_PRDC_H
#define DVDGAN_HIP_PRDC_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVD_PRDC_MAX_D 4096          /* widest feature vector */
#define DVD_PRDC_MAX_K 16            /* largest neighbour rank dvd_prdc_knn_radii serves */
#define DVD_PRDC_TILE 64             /* rows of a strip / of a tile of the other set */
#define DVD_PRDC_MAX_ROWS 16777216   /* rows of one set (2^24) */

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvd_prdc_strerror(int code);

/* pivot[j] <- fl32(mean_k X[k][j]), fp64 sums in row order (four interleaved row groups added in order): the definition, and the
 * bits, of dvd_eval_moments_update(first = 1).  X [n][d] fp32 with row stride ldx >= d (elements).
 * DVD_E_ARG: null pointer, n < 1, ldx < d.  DVD_E_SHAPE: d outside [1, DVD_PRDC_MAX_D], n * ldx above 2^40. */
int dvd_prdc_column_mean(const float* X, long long n, int d, long long ldx, float* pivot, void* stream);

/* r2[i] (fp64 [n]) <- the k-th smallest d2(X_i, X_j) over j != i.  j != i is by position: duplicate rows legitimately give
 * small or zero radii.  X [n][d] fp32, row stride ldx >= d; pivot fp32 [d] or NULL; ws: dvd_prdc_knn_ws_doubles(n, k) doubles,
 * 8-byte aligned (< 0 = the refusal).  Three launches: the rows' norms; per 64-row strip and chunk of the other rows' tiles the k
 * smallest distances of every row (a sorted list in registers); the merge of the chunks' lists per row.
 * DVD_E_ARG: null X / ws / r2, n < 1, k < 1, k >= n, ldx < d, ws or r2 not 8-byte aligned.  DVD_E_SHAPE: k > DVD_PRDC_MAX_K,
 * d outside [1, DVD_PRDC_MAX_D], n > DVD_PRDC_MAX_ROWS, n * ldx above 2^40. */
long long dvd_prdc_knn_ws_doubles(long long n, int k);
int dvd_prdc_knn_radii(const float* X, long long n, int d, long long ldx, const float* pivot, int k, double* ws, double* r2,
                       void* stream);

/* For every query row q < nq:  count[q] (int32) <- #{i < nr : d2(Q_q, R_i) <= r2[i]},  dmin[q] (fp64) <- min_i d2(Q_q, R_i).
 * Q [nq][d], R [nr][d] fp32 with row strides ldq, ldr >= d; pivot fp32 [d] or NULL; r2 fp64 [nr].  r2 and count may both be NULL
 * (only dmin is wanted); one of them NULL without the other is refused.  ws: dvd_prdc_ball_ws_doubles(nq, nr) doubles, 8-byte
 * aligned (< 0 = the refusal).
 * DVD_E_ARG: null Q / R / ws / dmin, r2 without count or count without r2, nq or nr < 1, ldq or ldr < d, ws / dmin / r2 not
 * 8-byte aligned.  DVD_E_SHAPE: d outside [1, DVD_PRDC_MAX_D], nq or nr > DVD_PRDC_MAX_ROWS, nq * ldq or nr * ldr above 2^40. */
long long dvd_prdc_ball_ws_doubles(long long nq, long long nr);
int dvd_prdc_ball_count(const float* Q, long long nq, long long ldq, const float* R, long long nr, long long ldr, int d,
                        const float* pivot, const double* r2, double* ws, int* count, double* dmin, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
