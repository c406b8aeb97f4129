/*
 * dvdx_cr.h -- C ABI of libdvdx_cr.so: the pair loss of balanced consistency regularization (bCR of Zhao et al. 2020, "Improved
 * Consistency Regularization for GANs") -- a discriminator's logits of transformed clips against its logits of the same clips
 * untransformed -- with both gradients and a row of statistics, one launch.  A library of the EXTENSION family
 * (dvd_gan_amd/xsrc/<key>/, include/dvdx_<key>.h, libdvdx_<key>.so; dvd_gan_amd/lib.py MORE_EXTENSIONS): plain C, device pointers
 * + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, return value 0 = ok, < 0 = DVD_E_ARG
 * (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide state.  Every argument is checked before anything
 * touches the device (the checks need no device).
 *
 * The expressions, exactly (contraction is off; fl32 = one rounding to fp32):
 *   gap_i     = fl32(aug_i - clean_i)
 *   S         = sum_i (double)gap_i * (double)gap_i                  (each product is exact in fp64)
 *   loss      = fl32(((double)weight * S) / (double)n)
 *   scale     = fl32(fl32(2 * weight) / (float)n)                    (2 * weight is exact short of overflow, n <= 2^20 is exact)
 *   d_aug_i   = fl32(scale * gap_i)
 *   d_clean_i = d_aug_i with the sign bit flipped
 * so a gradient carries three roundings (gap, scale, product) and the loss the gaps' roundings and one more.  An identical pair
 * has gap +0 and gradients +0 / -0.  Non-finite logits are not refused: they reach the loss and their own pair's gradients.
 *
 * Order of the sum: one workgroup of DVDX_CR_THREADS threads; thread t adds the pairs t, t + DVDX_CR_THREADS, ... in index
 * order, the 64 lanes of a wave are summed by a butterfly of xor shuffles (offsets 32 .. 1), the four waves' sums are added in
 * wave order.  No atomics: two launches on the same logits give the same bits.
 *
 * The statistics row (DVDX_CR_NSTAT floats, overwritten; NULL: not wanted):
 *   [DVDX_CR_STAT_PENALTY] loss      [DVDX_CR_STAT_MSQ] fl32(S / n)      [DVDX_CR_STAT_MAXABS] max_i |gap_i| (a NaN gap is passed over)
 *   [DVDX_CR_STAT_NONZERO] pairs with gap_i != 0 (a NaN gap counts)      [DVDX_CR_STAT_N] n
 */
#ifndef DVDX_CR_H
#define DVDX_CR_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVDX_CR_ABI_VERSION 1
#define DVDX_CR_MAX_N 1048576         /* most pairs of a call (2^20: counts and n are exact in fp32) */
#define DVDX_CR_THREADS 256           /* threads of the one workgroup */
#define DVDX_CR_NSTAT 5               /* floats of a statistics row */
#define DVDX_CR_STAT_PENALTY 0
#define DVDX_CR_STAT_MSQ 1
#define DVDX_CR_STAT_MAXABS 2
#define DVDX_CR_STAT_NONZERO 3
#define DVDX_CR_STAT_N 4

/* DVDX_CR_ABI_VERSION of the build */
int dvdx_cr_abi_version(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvdx_cr_strerror(int code);

/* loss[0] <- weight * mean((aug - clean)^2), d_aug / d_clean [n] <- its gradients, stats (or NULL) <- the row above.  aug, clean
 * [n] fp32 logits.  Nothing else is written.
 * DVD_E_ARG: a null aug / clean / loss / d_aug / d_clean, n < 1, a negative or non-finite weight (a NaN too).
 * DVD_E_SHAPE: n above DVDX_CR_MAX_N. */
int dvdx_cr_pair(const float* aug, const float* clean, long long n, float weight, float* loss, float* d_aug, float* d_clean,
                 float* stats, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
