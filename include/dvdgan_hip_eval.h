/*
 * dvdgan_hip_eval.h -- C ABI of libdvdgan_hip_eval.so: distribution distances of sample features (the statistic of FID / FVD /
 * KID; the feature extractor is the caller's).  A library of its own beside libdvdgan_hip.so (dvdgan_hip.h, whose set of entry
 * points is fixed) and libdvdgan_hip_adv.so: same conventions -- plain C, device pointers + sizes, asynchronous on `stream` (a
 * hipStream_t passed as void*), never synchronises, return value 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH
 * (-3) of dvdgan_hip.h.  No process-wide state.  Every argument is checked before anything touches the device.
 *
 * Deterministic: every output element is written by one thread and every sum has a fixed order (no atomics), so two runs on the
 * same inputs give the same bits.
 */
#ifndef DVDGAN_HIP_EVAL_H
#define DVDGAN_HIP_EVAL_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVD_EVAL_MAX_D 4096     /* widest feature vector dvd_eval_moments_update / dvd_eval_kid serve */
#define DVD_EVAL_TILE 64        /* side of a tile of the second-moment state and of a kernel-sum tile */
#define DVD_EVAL_MAX_SUBSETS 65535

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvd_eval_strerror(int code);

/* Pooled discriminator feature.  x: channels-last activation [R][P][C] (dtype DVD_F32 / DVD_BF16, contiguous), the tensor the
 * discriminators hand to their projection head: R frames, P = h * w positions, C channels.
 * out [R / g][C] fp32:  out[q][c] = (sum over the g rows r = q g .. q g + g - 1, in order, and over p in order, of relu(x[r][p][c])) / g,
 * fp32 accumulation: the head's pooled feature averaged over the g frames of a clip (g = 1: per frame).  One pass over x, 16-byte
 * loads when C is a multiple of the elements per 16 bytes and x is 16-byte aligned (scalar loads otherwise, same sums).
 * DVD_E_ARG: null pointer, unknown dtype, R / P / C / g < 1, R % g != 0.  DVD_E_SHAPE: R * P * C above 2^40. */
int dvd_eval_pool_features(int dtype, const void* x, long long R, int P, int C, int g, float* out, void* stream);

/* Running first and second moments of feature rows about a pivot.
 * State: pivot[d] fp32 and dvd_eval_moments_state_doubles(d) doubles =  S1[d] | the tiles (I, J >= I) of the upper triangle of S2,
 * row by row, DVD_EVAL_TILE x DVD_EVAL_TILE doubles each (row-major, entries past d are zero): tile (I, J) is number
 * I nb - I (I - 1) / 2 + (J - I) with nb = ceil(d / DVD_EVAL_TILE).  (-1 for d outside [1, DVD_EVAL_MAX_D].)
 * X [n][d] fp32 with row stride ldx >= d (elements).  first != 0: pivot <- fl(column mean of X) (fp64 sums in row order), and the
 * state is overwritten; first == 0: pivot is read and the state is added to.  With y = fl(x - pivot):
 *   S1[j] += sum_k y[k][j] (fp64),   S2[i][j] += fl32(sum_k y[k][i] y[k][j])
 * -- the products and the sum over the n rows of this call run on v_mfma_f32_32x32x2_f32 with fp32 accumulators, in row order; the
 * tile is then added once into the fp64 state.  One workgroup owns a tile; rows past n and columns past d contribute zero.
 * The count of rows lives with the caller.  mean = pivot + S1 / N, cov = (S2 - S1 S1^T / N) / (N - 1).
 * DVD_E_ARG: null pointer, n < 1, ldx < d, state not 8-byte aligned.  DVD_E_SHAPE: d outside [1, DVD_EVAL_MAX_D], n * ldx above 2^40. */
long long dvd_eval_moments_state_doubles(int d);
int dvd_eval_moments_update(const float* X, long long n, int d, long long ldx, float* pivot, double* state, int first,
                            void* stream);

/* Kernel distance: for every subset b < n_sub, with x_i = X[ix[b][i]], y_j = Y[iy[b][j]] (i, j < s) and k(a, b) = (a.b / d + 1)^3,
 *   out[b] = 1/(s(s-1)) sum_{i != j} k(x_i, x_j) + 1/(s(s-1)) sum_{i != j} k(y_i, y_j) - 2/s^2 sum_{i,j} k(x_i, y_j)      (fp64)
 * -- the unbiased MMD^2 of the polynomial kernel (Binkowski et al. 2018).  i != j is by position in the subset.  The dot products
 * run on v_mfma_f32_32x32x2_f32 over the gathered rows (fp32 accumulators, k in order); a.b / d + 1, the cube and the tile sums are
 * fp64.  Tile sums go into one slot each of ws (dvd_eval_kid_ws_doubles(n_sub, s) doubles, 8-byte aligned; < 0 = the refusal);
 * a second launch adds a subset's slots in a fixed order.  terms (may be NULL) [n_sub][3]: the three sums before their weights.
 * X [n][d], Y [m][d] fp32, row strides ldx, ldy >= d.  The index tables [n_sub][s] int32 are given twice, in host memory (every
 * entry is range-checked there before any launch) and in device memory (the same values).
 * DVD_E_ARG: null pointer other than terms, n / m / n_sub < 1, s < 2, ldx or ldy < d, an index outside [0, n) / [0, m), ws or
 * out not 8-byte aligned.  DVD_E_SHAPE: d outside [1, DVD_EVAL_MAX_D], n_sub > DVD_EVAL_MAX_SUBSETS, s > 65536, n * ldx or
 * m * ldy above 2^40. */
long long dvd_eval_kid_ws_doubles(int n_sub, int s);
int dvd_eval_kid(const float* X, long long n, long long ldx, const float* Y, long long m, long long ldy, int d,
                 const int* ix_host, const int* iy_host, const int* ix_dev, const int* iy_dev, int n_sub, int s, double* ws,
                 double* out, double* terms, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
