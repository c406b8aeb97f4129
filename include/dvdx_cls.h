/*
 * dvdx_cls.h -- C ABI of libdvdx_cls.so: the sums behind the Inception Score (Salimans et al. 2016) and the class-fidelity
 * metrics of a classifier's logits on generated samples -- softmax column sums, sum p log p, top-1 / top-5 hits against the
 * conditioning labels, their log likelihood and a confusion matrix -- per split, streamed over calls.  A library of the EXTENSION
 * family (dvd_gan_amd/xsrc/<key>/, include/dvdx_<key>.h, libdvdx_<key>.so; dvd_gan_amd/lib.py CLS_EXTENSIONS): plain C, device
 * pointers + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never synchronises, return value 0 = ok, < 0 =
 * DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide state.  Every argument is checked before
 * anything touches the device (the checks need no device).
 *
 * One call takes logits [rows, classes], row-major, in fp32, bf16 or fp16, optionally labels [rows] (int32), and the place of
 * these rows in the whole sample set: the global index row0 of the first one, the set's size n_total and the number of splits S.
 * Global row i belongs to split (i * S) / n_total (64-bit integers): split s holds the rows ceil(s * n_total / S) ..
 * ceil((s + 1) * n_total / S) - 1, contiguous and as equal as they can be.
 *
 * Per row, in fp64 on the stored values l_c (a half type is widened exactly; contraction is off):
 *   m       = max_c l_c
 *   logZ    = log(sum_c exp(l_c - m))
 *   logp_c  = (l_c - m) - logZ                      p_c = exp(logp_c)      (never the log of a rounded p: no 0 * log 0)
 *   argmax  = the lowest c with l_c == m
 * and with labels, for a label y in [0, classes):
 *   rank    = #{c : l_c > l_y} + #{c < y : l_c == l_y}       top-k: rank < k
 * A row with any non-finite logit is BAD: it is counted and enters no other sum, with or without a label.  A good row whose label
 * lies outside [0, classes) is counted as such, enters the sums that need no label and none of those that do.
 *
 * The state is fp64 [S][classes + DVDX_CLS_NSTAT], owned by the caller, zeroed by the caller before the first call and ADDED to
 * by every call, so successive calls stream a sample set of any size.  Row s: the column sums sum_i p_ic of the split's good rows
 * in columns 0 .. classes - 1, then at classes + DVDX_CLS_STAT_*:
 *   N          good rows                               A          sum_i sum_c p_ic * logp_ic
 *   BAD        bad rows
 *   LABELLED   good rows with a label in range         LOGLIK     sum_i logp_{i, y_i}
 *   TOP1       rows of rank 0                          TOP5       rows of rank < 5
 *   BAD_LABEL  good rows with a label out of range     (the last five stay untouched when labels is NULL)
 * The counts are exact integers in fp64.  confusion (or NULL) is int64 [classes][classes], added to as well: [y][argmax] += 1 for
 * every good row with a label y in range.
 *
 * Order of the sums.  Launch 1 gives every row one wave of 64 lanes: lane t adds the classes t, t + 64, ... in index order, the
 * lanes are summed by a butterfly of xor shuffles (offsets 32 .. 1).  Launch 2 gives every (split, column) of the state one owner:
 * wave q of its workgroup (q = 0 .. 3) adds the rows lo + q, lo + q + 4, ... of this call that lie in the split in row order, the
 * four sums are added in wave order and the total is added to the state.  Launch 3 (with a confusion matrix) gives every matrix
 * element one owner thread, which walks this call's rows in order.  No atomics: two runs over the same rows in the same calls give
 * the same bits; another cut into calls adds the same terms in another order.
 *
 * The workspace holds launch 1's per-row results: dvdx_cls_ws_bytes(rows, classes) bytes, 8-byte aligned, free once the call's
 * launches have run.
 */
#ifndef DVDX_CLS_H
#define DVDX_CLS_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVDX_CLS_ABI_VERSION 1
#define DVDX_CLS_F32 0
#define DVDX_CLS_BF16 1
#define DVDX_CLS_F16 2
#define DVDX_CLS_MAX_CLASSES 4096     /* most columns of the logits (Kinetics-600 and ImageNet-1000 fit) */
#define DVDX_CLS_MAX_ROWS 1048576     /* most rows of one call (2^20) */
#define DVDX_CLS_MAX_SPLITS 1024      /* most splits */
#define DVDX_CLS_MAX_TOTAL 1099511627776  /* most rows of the whole set (2^40: row * splits stays far inside 64 bits) */
#define DVDX_CLS_ROW_BYTES 40         /* workspace bytes per row: four doubles and two ints */
#define DVDX_CLS_NSTAT 8              /* doubles of a state row behind its column sums */
#define DVDX_CLS_STAT_N 0
#define DVDX_CLS_STAT_A 1
#define DVDX_CLS_STAT_BAD 2
#define DVDX_CLS_STAT_LABELLED 3
#define DVDX_CLS_STAT_LOGLIK 4
#define DVDX_CLS_STAT_TOP1 5
#define DVDX_CLS_STAT_TOP5 6
#define DVDX_CLS_STAT_BAD_LABEL 7

/* DVDX_CLS_ABI_VERSION of the build */
int dvdx_cls_abi_version(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvdx_cls_strerror(int code);

/* bytes of the workspace dvdx_cls_update needs for logits [rows, classes]: rows * DVDX_CLS_ROW_BYTES; 0 for counts it refuses. */
long long dvdx_cls_ws_bytes(long long rows, int classes);

/* state [splits][classes + DVDX_CLS_NSTAT] += the sums above of logits [rows, classes] (dtype: DVDX_CLS_F32 / _BF16 / _F16),
 * the global rows row0 .. row0 + rows - 1 of n_total; labels: int32 [rows] or NULL; confusion: int64 [classes][classes] or NULL
 * (it needs labels).  ws [ws_bytes] is overwritten.  Nothing else is written.
 * DVD_E_ARG: a null logits / state / ws, a confusion matrix without labels, ws not 8-byte aligned, an unknown dtype, rows,
 * classes, n_total or splits < 1, row0 < 0, splits > n_total, row0 + rows > n_total, ws_bytes below dvdx_cls_ws_bytes(rows,
 * classes).      DVD_E_SHAPE: classes above DVDX_CLS_MAX_CLASSES, rows above DVDX_CLS_MAX_ROWS, splits above DVDX_CLS_MAX_SPLITS,
 * n_total above DVDX_CLS_MAX_TOTAL. */
int dvdx_cls_update(int dtype, const void* logits, const int* labels, long long rows, int classes, long long row0,
                    long long n_total, int splits, double* state, long long* confusion, void* ws, long long ws_bytes, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
