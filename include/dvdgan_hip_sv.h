/*
 * dvdgan_hip_sv.h -- C ABI of libdvdgan_hip_sv.so: the top singular values of every weight matrix of a network (the diagnostic of
 * Brock et al. 2019, "BigGAN", section 4 and figure 3) by block power (subspace) iteration with a Rayleigh-Ritz finish, all
 * matrices of a table in a fixed number of launches.  A library of its own beside libdvdgan_hip.so, libdvdgan_hip_adv.so,
 * libdvdgan_hip_eval.so, libdvdgan_hip_prdc.so, libdvdgan_hip_aug.so and libdvdgan_hip_geom.so (whose sets of entry points are
 * fixed): same conventions -- plain C, device pointers + sizes, asynchronous on `stream` (a hipStream_t passed as void*), never
 * synchronises, return value 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) / DVD_E_LAUNCH (-3) of dvdgan_hip.h.  No process-wide
 * state.  Every argument is checked before anything touches the device.  Nothing an item points to with a const pointer is written.
 *
 * An item is one matrix W, row-major fp32 [h][w], h >= 1, w >= 1, aligned to 4 bytes only (a slice of a flat buffer).  All
 * arithmetic is fp64 (an fp32 value converts exactly).  With block width b (1 <= k <= b <= DVD_SV_MAX_BLOCK) the stored width is
 * bp = 8 for b <= 8 and 16 above; an item uses r = min(b, h, w) columns and the columns from r on are exact zeros throughout.
 * The persistent state of an item is  V [w][bp], Y [h][bp], R [bp][bp]  (doubles, at state_off of the state buffer, in this
 * order); its workspace is  P [h][bp], aux [h][2]  (at ws_off of the workspace).
 *
 * One iteration on V (orthonormal columns):
 *   1. Y = W V           a wave owns rows; lane l sums the 4-column chunks l, l + 64, ... of a row in ascending order, then the
 *                        w mod 4 last columns (lane l the l-th), and the 64 lane sums are added by a butterfly (xor 32, 16, .. 1)
 *   2. Y <- orth(Y)      below
 *   3. Z = W^T Y         a workgroup owns 64 columns; wave q of its 4 sums rows q, q + 4, ... in ascending order and the four
 *                        partial sums are added in the order 0, 1, 2, 3.  Z is written over V
 *   4. V, R <- orth(Z)   Z = V R, R upper triangular
 * orth(A), A [n][bp], is classical Gram-Schmidt with a second pass, one workgroup of 1024 threads per item, column by column:
 * twice { c_i = q_i . a_j for i < j;  a_j -= sum_i c_i q_i;  R[i][j] += c_i }, then nrm = |a_j|.  If nrm <= 2^-40 * (the largest
 * column norm of A before any projection) -- an all-zero A included -- the column becomes exact zeros and R[j][j] = 0, else
 * a_j /= nrm and R[j][j] = nrm.  Thread t sums rows t, t + 1024, ... in ascending order; a wave adds by the butterfly above and the
 * sixteen wave sums are added in the order 0, 1, .. 15.  No Gram matrix is factorised: nearly dependent columns (a decaying spectrum)
 * and rank-deficient W are the normal case.
 *
 * The finish (dvd_sv_ritz): one more product P = W V with two extras per row, aux[i][0] = sum_j W[i][j] v[j] (the item's spectral
 * norm vector as an unorthogonalised column; 0 without one) and aux[i][1] = sum_j W[i][j]^2.  Then one wave per item takes the SVD
 * of R by one-sided Jacobi (Hestenes) on its columns, cyclic over the pairs (p, q), p < q, in row-major order: with
 * al = |m_p|^2, be = |m_q|^2, ga = m_p . m_q the pair is rotated when |ga| > 2^-50 sqrt(al be):  ze = (be - al) / (2 ga),
 * t = sign(ze) / (|ze| + sqrt(1 + ze^2)),  c = 1 / sqrt(1 + t^2),  s = c t,  m_p' = c m_p - s m_q,  m_q' = s m_p + c m_q (the
 * same rotation is accumulated in J, which starts as the identity); sweeps repeat until one rotates nothing, DVD_SV_MAX_SWEEPS
 * at most.  sg_c = |m_c|, sorted descending (ties: lower column first).  For the i-th largest, column c:
 *   u_i = Y J[:, c],  v_i = V m_c / sg_c (0 when sg_c = 0),  so that  W^T u_i = sg_i v_i  holds by construction, and
 *   res_i = | P m_c / sg_c - sg_i Y J[:, c] | = | W v_i - sg_i u_i |.
 * Output row of an item, doubles [2 k + 2]:  sv[k] (descending; 0 beyond r),  res[k],  fro2 = sum aux[.][1],
 * sn_sigma = sum_i u[i] aux[i][0]  when the item has u and v, else NaN.
 * A report of T iterations reads every W 2 T + 1 times.  Every output element has one owner, no sum uses an atomic, and an item's
 * numbers are a function of its W, h, w, bp and start block alone: not of the table it stands in, its place there or W's address.
 */
#ifndef DVDGAN_HIP_SV_H
#define DVDGAN_HIP_SV_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

#define DVD_SV_ABI_VERSION 1
#define DVD_SV_MAX_BLOCK 16           /* largest block width b */
#define DVD_SV_MAX_SWEEPS 60          /* Jacobi sweeps of the finish, at most */
#define DVD_SV_MAX_ITEMS 65535        /* matrices of one table */
#define DVD_SV_MAX_ITERS 4096         /* iterations of one dvd_sv_iterate call */

typedef struct dvd_sv_item {
    const float* W;             /* [h][w] fp32, read only */
    const float* u;             /* [h] fp32 or NULL, read only */
    const float* v;             /* [w] fp32 or NULL (both or neither), read only */
    long long state_off;        /* doubles: the item's V, Y, R in the state buffer        (dvd_sv_prepare) */
    long long ws_off;           /* doubles: the item's P, aux in the workspace            (dvd_sv_prepare) */
    int h, w;
    int slot;                   /* the item's place in an output row, 0 <= slot < n, each taken once */
    int blk_wv, blk_wtv;        /* first workgroup of the item in the W V and W^T Y launches  (dvd_sv_prepare) */
    int pad_;
} dvd_sv_item;

/* DVD_SV_ABI_VERSION of the build */
int dvd_sv_abi_version(void);

/* sizeof(dvd_sv_item) of the build */
int dvd_sv_item_size(void);

/* "ok" / what DVD_E_ARG, DVD_E_SHAPE, DVD_E_LAUNCH mean in this library */
const char* dvd_sv_strerror(int code);

/* Host only: fills state_off, ws_off, blk_wv, blk_wtv of items[0..n) for block width `block` and reports the doubles of the state
 * buffer and of the workspace.  The caller then uploads the table once and passes both copies to the calls below.
 * DVD_E_ARG: null items / out-parameters, n outside [1, DVD_SV_MAX_ITEMS], block outside [1, DVD_SV_MAX_BLOCK], an item with a
 * null W, with one of u, v but not the other, or with a slot outside [0, n) or taken twice.
 * DVD_E_SHAPE: h < 1, w < 1, or a launch of more than 2^31 - 1 workgroups. */
int dvd_sv_prepare(dvd_sv_item* items, int n, int block, long long* state_doubles, long long* ws_doubles);

/* state <- start (a device buffer of state_doubles doubles in the state's layout: each item's start block in its V, zeros
 * elsewhere), then every V orthonormalised by orth.  Refusals: those of dvd_sv_prepare for `host` (the prepared table;
 * DVD_E_ARG as well when its planner columns are not what dvd_sv_prepare writes), null items / start / state, start == state. */
int dvd_sv_init(const dvd_sv_item* items, const dvd_sv_item* host, int n, int block, const double* start, double* state,
                void* stream);

/* `iters` iterations from the blocks the state holds, 4 launches each.  DVD_E_ARG also: iters outside [0, DVD_SV_MAX_ITERS]
 * (0 succeeds and launches nothing), null state. */
int dvd_sv_iterate(const dvd_sv_item* items, const dvd_sv_item* host, int n, int block, int iters, double* state, void* stream);

/* The finish, 2 launches: out[row][slot][2 k + 2] of a ring out[n_rows][n][2 k + 2].  The state is not changed.  DVD_E_ARG also:
 * k outside [1, block], null state / ws / out, row outside [0, n_rows).  Before the first iteration R is zero: sv = 0. */
int dvd_sv_ritz(const dvd_sv_item* items, const dvd_sv_item* host, int n, int block, int k, const double* state, double* ws,
                double* out, long long row, long long n_rows, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
