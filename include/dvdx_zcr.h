/*
 * dvdx_zcr.h -- C ABI of libdvdx_zcr.so: the clip distance of latent consistency regularization (zCR of Zhao et al. 2020,
 * "Improved Consistency Regularization for GANs") -- the generator's clips G(z) against its clips G(z + dz) of the perturbed
 * latents, term = -weight * mean((a - b)^2) over whole clips -- and its gradient.  A library of the EXTENSION family
 * (dvd_gan_amd/xsrc/<key>/, include/dvdx_<key>.h, libdvdx_<key>.so; dvd_gan_amd/lib.py ZCR_EXTENSIONS): plain C, device pointers
 * + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, return value 0 = ok, < 0 = DVD_E_ARG
 * (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide state.  Every argument is checked before anything
 * touches the device (the checks need no device).
 *
 * a and b are fp32 [pairs, n], row p of a against row p of b; N = pairs * n as a 64-bit count.  Two streaming launches over tens
 * of millions of floats each: 16-byte loads and stores where the pointers allow them, a grid sized to the chip, 64-bit indices.
 *
 * The forward, exactly (contraction is off; fl32 = one rounding to fp32, fl64 = one rounding to fp64):
 *   gap_pi   = fl32(a_pi - b_pi)
 *   S_p      = sum_i (double)gap_pi * (double)gap_pi                  (each product is exact in fp64; the order is below)
 *   total    = sum_p S_p                                              (the order is below)
 *   term     = fl32(-(fl64(fl64((double)weight * total) / fl64((double)pairs * (double)n))))
 * so the term carries the gaps' roundings, the fp64 sums' and one fp32 rounding.  Identical rows give gaps +0 and the term -0.
 * Non-finite values are not refused: they reach the term.
 *
 * Order of the sums.  A row is cut into C = dvdx_zcr_chunks(pairs, n) chunks of L = 4 * ceil(ceil(n / C) / 4) elements (the last
 * one shorter, possibly empty); chunk c of row p is work unit p * C + c and has ONE owner, a workgroup of DVDX_ZCR_THREADS
 * threads.  When both chunk pointers are 16-byte aligned, thread t adds the elements of the 4-element groups t, t +
 * DVDX_ZCR_THREADS, ... of the chunk in index order (a last group of fewer than 4 elements included); otherwise (the rows of a
 * second half that is only 4-byte aligned, or an n that is no multiple of 4) it adds the elements t, t + DVDX_ZCR_THREADS, ...
 * The 64 lanes of a wave are summed by a butterfly of xor shuffles (offsets 32 .. 1), the four waves' sums are added in wave
 * order, and the chunk's sum and its largest |gap| go to ws[2 * unit], ws[2 * unit + 1].  The finishing launch is one workgroup:
 * thread t owns the rows t, t + DVDX_ZCR_THREADS, ...; S_p is its chunks' sums added in chunk order; the thread adds its rows'
 * S_p in row order; lanes and waves are combined as above.  No atomics: two launches on the same pointers give the same bits.
 *
 * The statistics row (DVDX_ZCR_NSTAT floats, overwritten; NULL: not wanted):
 *   [DVDX_ZCR_STAT_TERM] term                        [DVDX_ZCR_STAT_MSQ] fl32(total / fl64((double)pairs * (double)n))
 *   [DVDX_ZCR_STAT_MIN_PAIR] min_p fl32(S_p / n)     [DVDX_ZCR_STAT_MAX_PAIR] max_p fl32(S_p / n)     (a NaN row is passed over)
 *   [DVDX_ZCR_STAT_MAXABS] max |gap_pi| (a NaN gap is passed over)                  [DVDX_ZCR_STAT_PAIRS] pairs
 *
 * The gradient of term * upstream, exactly:
 *   scale    = fl32(fl64(fl64(2 * (double)weight) / fl64((double)pairs * (double)n)))      (on the host: one value per call)
 *   g        = fl32(upstream[0] * scale)                                                    (on the device: no host read)
 *   db_i     = fl32(g * gap_i),  gap_i as above
 *   da_i     = db_i with the sign bit flipped
 * one pass, every element written once; nothing of full size is kept between the two calls.
 */
#ifndef DVDX_ZCR_H
#define DVDX_ZCR_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVDX_ZCR_ABI_VERSION 1
#define DVDX_ZCR_MAX_PAIRS 65536      /* most rows of a call (the finishing launch walks them in one workgroup) */
#define DVDX_ZCR_MAX_N 1099511627776  /* most elements of a row (2^40: pairs * n stays far inside 64 bits) */
#define DVDX_ZCR_THREADS 256          /* threads of a workgroup */
#define DVDX_ZCR_MAX_BLOCKS 2048      /* most workgroups of a launch: 8 for each of the 256 compute units */
#define DVDX_ZCR_MIN_CHUNK 4096       /* a row is not cut into chunks shorter than this */
#define DVDX_ZCR_NSTAT 6              /* floats of a statistics row */
#define DVDX_ZCR_STAT_TERM 0
#define DVDX_ZCR_STAT_MSQ 1
#define DVDX_ZCR_STAT_MIN_PAIR 2
#define DVDX_ZCR_STAT_MAX_PAIR 3
#define DVDX_ZCR_STAT_MAXABS 4
#define DVDX_ZCR_STAT_PAIRS 5

/* DVDX_ZCR_ABI_VERSION of the build */
int dvdx_zcr_abi_version(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvdx_zcr_strerror(int code);

/* C, the chunks a row of n elements is cut into: min(ceil(n / DVDX_ZCR_MIN_CHUNK), max(1, DVDX_ZCR_MAX_BLOCKS / pairs)); 0 for
 * arguments dvdx_zcr_dist refuses. */
long long dvdx_zcr_chunks(long long pairs, long long n);

/* doubles of the workspace dvdx_zcr_dist needs: 2 * pairs * C; 0 for arguments it refuses. */
long long dvdx_zcr_ws_doubles(long long pairs, long long n);

/* term[0] <- -weight * mean((a - b)^2), stats (or NULL) <- the row above, ws [ws_doubles] <- the chunks' partial results.
 * Nothing else is written.
 * DVD_E_ARG: a null a / b / ws / term, pairs < 1, n < 1, a negative or non-finite weight (a NaN too), ws_doubles below
 * dvdx_zcr_ws_doubles(pairs, n).       DVD_E_SHAPE: pairs above DVDX_ZCR_MAX_PAIRS, n above DVDX_ZCR_MAX_N. */
int dvdx_zcr_dist(const float* a, const float* b, long long pairs, long long n, float weight, double* ws, long long ws_doubles,
                  float* term, float* stats, void* stream);

/* da, db [pairs, n] <- the gradients above of upstream[0] * term; upstream is a DEVICE pointer to one fp32 value.  da and db are
 * typically the two halves of one [2 * pairs, n] buffer.  Nothing else is written.
 * DVD_E_ARG: a null a / b / upstream / da / db, pairs < 1, n < 1, a negative or non-finite weight.
 * DVD_E_SHAPE: pairs above DVDX_ZCR_MAX_PAIRS, n above DVDX_ZCR_MAX_N. */
int dvdx_zcr_dist_grad(const float* a, const float* b, long long pairs, long long n, float weight, const float* upstream,
                       float* da, float* db, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
