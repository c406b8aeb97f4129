// libdvdgan_hip_prdc.so (include/dvdgan_hip_prdc.h): k-nearest-neighbour radii and ball counts of sample features, the
// statistics behind precision / recall / density / coverage.
//
//   mean     pivot[j] = fl(mean_k X[k][j]): eval_pivot_kernel's sums (csrc/eval/distmetrics.hip), so the same bits.
//   norm     one thread per row: the fp64 sum, in k order, of the squares of y = fl32(x - pivot).
//   pair     all distances between a strip of 64 "owner" rows (the rows whose radius / count is sought) and a chunk of the other
//            set's 64-row tiles, never stored.  Four waves, one 32 x 32 block of v_mfma_f32_32x32x2_f32 each; both operands are
//            K-contiguous rows staged as [64 rows][32 k] slabs at pitch 33 like eval_kid_kernel's.  The next slab's loads -- the
//            next tile's first slab included: one loop runs over all slabs of all tiles -- are in flight while the current one is
//            multiplied; the pivot is subtracted when a slab is stored to LDS, NOT where it is loaded (a subtraction there makes
//            the wave wait for its loads before it multiplies; the first version did that, among other things, and was 3.6 x
//            slower on the whole call: profiles/prdc_numbers.md).  The owners sit on the MFMA's N
//            side: a lane owns ONE owner row (lane & 31 of its wave's half) and finds 16 candidate distances of it in its own
//            accumulator registers, so the selection needs no cross-lane work: d2 = max(0, (|a|^2 + |b|^2) - 2 acc) in fp64, then
//              radii: a sorted list of the KCAP smallest in registers (compare-exchange insertion, fully unrolled: every index is
//                     a compile-time constant, nothing goes to scratch), KCAP in {4, 8, 16} >= k; the candidate at the owner's
//                     own position and rows past n are left out;
//              ball:  a running count of d2 <= r2[candidate] and a running minimum.
//            The four partial results per owner (two waves x two lane halves) are merged through LDS by one thread per owner and
//            written to the slot of this chunk.
//   merge    one thread per row: the chunks' slots in slot order -> the k-th smallest of the S k candidates / the sum of the
//            counts and the minimum.  The k-th smallest of a multiset does not depend on the visiting order.
// The other set is split into S chunks of tpc tiles: S = min(tiles, ceil(2048 / strips) rounded up to a multiple of 8),
// re-balanced so that no chunk is empty -- a fixed function of the two row counts, so small sets still fill the chip and results
// depend on nothing else.  Workgroup b of the 1-D grid is (strip b / S, chunk b % S).
//
// Budgets (hipcc -O3, gfx950; build/prdc.res must show no scratch for any kernel):
//   prdc_pair_kernel   LDS 16.5 KB slabs (which become the merge area of 64 x 4 x KCAP doubles once the last slab has been multiplied;
//                      32 KB at KCAP = 16, where the merge area is the larger) + 0.5 .. 2 KB candidate norms / radii / counts;
//                      16 accumulator (AGPRs) + 17 staging registers + 2 KCAP for the list: 80 / 80 / 108 VGPRs for KCAP 4 / 8 / 16
//                      and 82 for the ball count as built, five (four) workgroups per CU
// Every output element has one owner and every sum a fixed order: no atomics.  All loads of X are scalar dwords with bounds
// checks (row strides are only 4-byte aligned); every store is bounds-checked against the padded slot sizes the ws query counts.
#include <algorithm>
#include "../common.h"
#include "../../../include/dvdgan_hip_prdc.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_T = DVD_PRDC_TILE;
constexpr int PR_KC = 32, PR_LD = PR_KC + 1;        // k per slab, LDS row pitch
constexpr long long PR_MAX_ELEMS = 1ll << 40;
#ifndef DVD_PRDC_TARGET_WGS                         // workgroups the split aims at: eight per CU of a 256-CU part (512, 1024 and
#define DVD_PRDC_TARGET_WGS 2048                    //  4096 were measured: profiles/prdc_numbers.md)
#endif
constexpr long long PR_TARGET_WGS = DVD_PRDC_TARGET_WGS;
static_assert(PR_T == 64, "the kernels below are written for 64-row strips and tiles");

// ----------------------------------------------------------------------------- mean, norms
__global__ __launch_bounds__(PR_THREADS) void prdc_mean_kernel(const float* __restrict__ X, long long n, int d, long long ldx,
                                                               float* __restrict__ pivot) {
    __shared__ double red[4 * PR_T];
    const int col = threadIdx.x & 63, kr = threadIdx.x >> 6;
    const int gj = blockIdx.x * PR_T + col;
    double s = 0.0;
    if (gj < d) {
        // eight loads in flight, added in row order: the order (and the bits) of the plain loop
        long long k = kr;
        for (; k + 28 < n; k += 32) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = X[(k + 4 * e) * ldx + gj];
#pragma unroll
            for (int e = 0; e < 8; ++e) s += (double)v[e];
        }
        for (; k < n; k += 4) s += (double)X[k * ldx + gj];
    }
    red[kr * PR_T + col] = s;
    __syncthreads();
    if (kr == 0 && gj < d)
        pivot[gj] = (float)((((red[col] + red[PR_T + col]) + red[2 * PR_T + col]) + red[3 * PR_T + col]) / (double)n);
}

// one wave per workgroup: its 64 rows' current cache lines fit the CU's L1, and a set of 10 000 rows still spreads over 157 CUs
constexpr int PR_NORM_THREADS = 64;
__global__ __launch_bounds__(PR_NORM_THREADS) void prdc_norm_kernel(const float* __restrict__ X, int n, int d, long long ldx,
                                                                    const float* __restrict__ pivot, double* __restrict__ norm) {
    const int i = blockIdx.x * PR_NORM_THREADS + threadIdx.x;
    if (i >= n) return;
    const float* p = X + (long long)i * ldx;
    double s = 0.0;
    int k = 0;
    for (; k + 8 <= d; k += 8) {                                     // eight loads in flight, added in k order
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[k + e];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float y = v[e] - (pivot ? pivot[k + e] : 0.f);
            s += (double)y * (double)y;
        }
    }
    for (; k < d; ++k) {
        const float y = p[k] - (pivot ? pivot[k] : 0.f);
        s += (double)y * (double)y;
    }
    norm[i] = s;
}

// ----------------------------------------------------------------------------- the sorted list
template <int K> __device__ __forceinline__ void list_insert(double (&l)[K], double v) {
    if (v < l[K - 1]) {
        l[K - 1] = v;
#pragma unroll
        for (int i = K - 1; i > 0; --i) {
            const double a = l[i - 1], b = l[i];
            const bool sw = b < a;
            l[i - 1] = sw ? b : a;
            l[i] = sw ? a : b;
        }
    }
}

// ----------------------------------------------------------------------------- pair
// RADII: own == cand (one set); part [S][strips * 64][k] doubles.  Ball (RADII = false, KCAP unused): pcnt / pmin [S][strips * 64].
template <bool RADII, int KCAP>
__global__ __launch_bounds__(PR_THREADS) void prdc_pair_kernel(const float* __restrict__ Own, long long ldo, int n_own,
                                                               const float* __restrict__ Cand, long long ldc, int n_cand, int d,
                                                               const float* __restrict__ pivot, const double* __restrict__ norm_own,
                                                               const double* __restrict__ norm_cand, const double* __restrict__ r2,
                                                               int tpc, int nct, int S, int k, double* __restrict__ part,
                                                               double* __restrict__ pcnt, double* __restrict__ pmin) {
    // the two slabs; once the last slab has been multiplied the same memory is the merge area
    constexpr int SLAB = PR_T * PR_LD, MERGE = RADII ? PR_T * 4 * KCAP : PR_T * 4;
    __shared__ double sBuf[SLAB > MERGE ? SLAB : MERGE];
    __shared__ double sN[PR_T], sR[RADII ? 1 : PR_T];
    __shared__ int sC[RADII ? 1 : PR_T * 4];
    float* sA = reinterpret_cast<float*>(sBuf);
    float* sB = sA + SLAB;
    double* sM = sBuf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    // chunk is the fast index: with S a multiple of 8 the workgroups of one XCD (dispatched round-robin) share chunks AND strips
    const int strip = blockIdx.x / S, chunk = blockIdx.x - strip * S, strips = gridDim.x / S;
    const int t0 = chunk * tpc, t1 = min(t0 + tpc, nct);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    const int kk = tid & 31, r0 = tid >> 5;                          // staging: 8 rows x 32 k per pass, 8 passes
    const int own_l = wn * 32 + (lane & 31), gj = strip * PR_T + own_l;       // the owner row of this lane
    const double no = gj < n_own ? norm_own[gj] : 0.0;
    const int sub = wm * 2 + (lane >> 5);                            // which of the owner's four partial results this lane keeps

    double list[KCAP];
#pragma unroll
    for (int i = 0; i < KCAP; ++i) list[i] = inf;
    int cnt = 0;
    double dmin = inf;

    const float* As = sA + (wm * 32 + (lane & 31)) * PR_LD + (lane >> 5);
    const float* Bs = sB + (wn * 32 + (lane & 31)) * PR_LD + (lane >> 5);
    float ra[8], rb[8], cl = 0.f;                                    // the slab in flight (raw values) and its pivot entry
    double nreg = 0.0, rreg = 0.0;                                   // ... and, with a tile's first slab, a candidate's norm and radius

    // one loop over all slabs of all tiles of the chunk: the first slab of the next tile is in flight while the last one of the
    // current tile is multiplied.  (lct, lks): tile and slab being loaded, (ct, ks): being multiplied.
    const int nslab = (d + PR_KC - 1) / PR_KC, total = (t1 - t0) * nslab;
    int ct = t0, ks = 0, lct = t0, lks = 0;
    const int own0 = strip * PR_T + r0;
    auto gload = [&](int lct, int lks) {
        const int kx = lks * PR_KC + kk, cand0 = lct * PR_T + r0;
        const bool kin = kx < d;
        cl = 0.f;
        if (pivot && kin) cl = pivot[kx];
        const float* pa = Cand + (long long)cand0 * ldc + kx;
        const float* pb = Own + (long long)own0 * ldo + kx;
        // The pivot is subtracted when the slab is stored to LDS, not here: nothing waits for these loads before the slab in LDS
        // has been multiplied.  Rows past the set and columns past d are not loaded and are staged as exact zeros.
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ra[j] = 0.f;
            rb[j] = 0.f;
            if (kin && cand0 + 8 * j < n_cand) ra[j] = pa[(long long)(8 * j) * ldc];
            if (kin && own0 + 8 * j < n_own) rb[j] = pb[(long long)(8 * j) * ldo];
        }
        if (lks == 0 && tid < PR_T) {
            const int gi = lct * PR_T + tid;
            nreg = gi < n_cand ? norm_cand[gi] : 0.0;
            if (!RADII) rreg = (r2 && gi < n_cand) ? r2[gi] : 0.0;
        }
    };
    f32x16 acc;
    // a wave whose 32 owners all lie past the set has nothing to compute (it still stages and keeps the barriers)
    const bool own_in = strip * PR_T + wn * 32 < n_own;

    if (total > 0) gload(lct, lks);
    for (int it = 0; it < total; ++it) {
        __syncthreads();                                             // the previous slab, and the previous tile's sN / sR, have been read
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sA[(r0 + 8 * j) * PR_LD + kk] = ct * PR_T + r0 + 8 * j < n_cand ? ra[j] - cl : 0.f;
            sB[(r0 + 8 * j) * PR_LD + kk] = own0 + 8 * j < n_own ? rb[j] - cl : 0.f;
        }
        if (ks == 0) {
            if (tid < PR_T) {
                sN[tid] = nreg;
                if (!RADII) sR[tid] = rreg;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        __syncthreads();
        if (it + 1 < total) {
            if (++lks == nslab) { lks = 0; ++lct; }
            gload(lct, lks);
        }
        const bool active = own_in && ct * PR_T + wm * 32 < n_cand;
        if (active) {
#pragma unroll
            for (int kq = 0; kq < PR_KC; kq += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kq], Bs[kq], acc, 0, 0, 0);
        }
        if (++ks < nslab) continue;
        if (active) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int li = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int gi = ct * PR_T + li;
                const double v = fmax(0.0, (sN[li] + no) - 2.0 * (double)acc[r]);
                if (RADII) {
                    if (gi < n_cand && gi != gj) list_insert<KCAP>(list, v);
                } else if (gi < n_cand) {
                    dmin = fmin(dmin, v);
                    if (r2) cnt += v <= sR[li] ? 1 : 0;
                }
            }
        }
        ks = 0;
        ++ct;
    }
    __syncthreads();                                                 // the slabs are done with: their memory becomes the merge area

    // the four partial results of an owner -> one, by one thread per owner, into the slot of this chunk
    const long long npad = (long long)strips * PR_T;
    if (RADII) {
#pragma unroll
        for (int i = 0; i < KCAP; ++i) sM[(own_l * 4 + sub) * KCAP + i] = list[i];
        __syncthreads();
        if (tid < PR_T) {
            double m[KCAP];
#pragma unroll
            for (int i = 0; i < KCAP; ++i) m[i] = inf;
            for (int e = 0; e < 4 * KCAP; ++e) list_insert<KCAP>(m, sM[tid * 4 * KCAP + e]);
            double* dst = part + ((long long)chunk * npad + strip * PR_T + tid) * k;
#pragma unroll
            for (int i = 0; i < KCAP; ++i)
                if (i < k) dst[i] = m[i];
        }
    } else {
        sM[own_l * 4 + sub] = dmin;
        sC[own_l * 4 + sub] = cnt;
        __syncthreads();
        if (tid < PR_T) {
            const long long at = (long long)chunk * npad + strip * PR_T + tid;
            pmin[at] = fmin(fmin(sM[tid * 4], sM[tid * 4 + 1]), fmin(sM[tid * 4 + 2], sM[tid * 4 + 3]));
            pcnt[at] = (double)(((sC[tid * 4] + sC[tid * 4 + 1]) + sC[tid * 4 + 2]) + sC[tid * 4 + 3]);
        }
    }
}

// ----------------------------------------------------------------------------- merge
template <int KCAP>
__global__ __launch_bounds__(PR_THREADS) void prdc_knn_merge_kernel(const double* __restrict__ part, int n, long long npad, int S,
                                                                    int k, double* __restrict__ r2) {
    const int i = blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= n) return;
    double m[KCAP];
#pragma unroll
    for (int j = 0; j < KCAP; ++j) m[j] = __longlong_as_double(0x7ff0000000000000ll);
    for (int s = 0; s < S; ++s) {
        const double* p = part + ((long long)s * npad + i) * k;
        for (int j = 0; j < k; ++j) list_insert<KCAP>(m, p[j]);
    }
    double out = m[0];
#pragma unroll
    for (int j = 1; j < KCAP; ++j)
        if (j == k - 1) out = m[j];
    r2[i] = out;
}

__global__ __launch_bounds__(PR_THREADS) void prdc_ball_merge_kernel(const double* __restrict__ pcnt, const double* __restrict__ pmin,
                                                                     int nq, long long npad, int S, int* __restrict__ count,
                                                                     double* __restrict__ dmin) {
    const int q = blockIdx.x * PR_THREADS + threadIdx.x;
    if (q >= nq) return;
    long long c = 0;
    double m = __longlong_as_double(0x7ff0000000000000ll);
    for (int s = 0; s < S; ++s) {
        c += (long long)pcnt[(long long)s * npad + q];
        m = fmin(m, pmin[(long long)s * npad + q]);
    }
    if (count) count[q] = (int)c;
    dmin[q] = m;
}

inline bool strided_ok(long long rows, long long ld) { return ld <= PR_MAX_ELEMS / rows; }
inline long long tiles(long long rows) { return (rows + PR_T - 1) / PR_T; }

// how the candidate set's tiles are split into chunks: a fixed function of the two row counts
inline void split(long long n_own, long long n_cand, int& S, int& tpc) {
    const long long strips = tiles(n_own), nct = tiles(n_cand);
    const long long want = std::min(nct, ((PR_TARGET_WGS + strips - 1) / strips + 7) / 8 * 8);
    tpc = (int)((nct + want - 1) / want);
    S = (int)((nct + tpc - 1) / tpc);
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" const char* dvd_prdc_strerror(int code) {
    switch (code) {
        case DVD_OK: return "ok";
        case DVD_E_ARG: return "bad argument (null pointer / non-positive size / stride below the row length / neighbour rank below 1 or "
                               "not below the row count / radii without counts or counts without radii / misaligned workspace)";
        case DVD_E_SHAPE: return "unsupported shape (feature width outside [1, 4096], neighbour rank above 16, too many rows or elements)";
        case DVD_E_LAUNCH: return "kernel launch failed";
        default: return "unknown error";
    }
}

extern "C" int dvd_prdc_column_mean(const float* X, long long n, int d, long long ldx, float* pivot, void* stream) {
    if (!X || !pivot || n < 1) return DVD_E_ARG;
    if (d < 1 || d > DVD_PRDC_MAX_D) return DVD_E_SHAPE;
    if (ldx < d || ((uintptr_t)X & 3) || ((uintptr_t)pivot & 3)) return DVD_E_ARG;
    if (!strided_ok(n, ldx)) return DVD_E_SHAPE;
    prdc_mean_kernel<<<(unsigned)tiles(d), PR_THREADS, 0, S_>>>(X, n, d, ldx, pivot);
    return launch_status();
}

extern "C" long long dvd_prdc_knn_ws_doubles(long long n, int k) {
    if (n < 1 || k < 1 || k >= n) return DVD_E_ARG;
    if (k > DVD_PRDC_MAX_K || n > DVD_PRDC_MAX_ROWS) return DVD_E_SHAPE;
    int S, tpc;
    split(n, n, S, tpc);
    return n + (long long)S * tiles(n) * PR_T * k;
}

extern "C" int dvd_prdc_knn_radii(const float* X, long long n, int d, long long ldx, const float* pivot, int k, double* ws,
                                  double* r2, void* stream) {
    if (!X || !ws || !r2 || n < 1 || k < 1 || k >= n) return DVD_E_ARG;
    if (k > DVD_PRDC_MAX_K || d < 1 || d > DVD_PRDC_MAX_D || n > DVD_PRDC_MAX_ROWS) return DVD_E_SHAPE;
    if (ldx < d || ((uintptr_t)ws & 7) || ((uintptr_t)r2 & 7) || ((uintptr_t)X & 3) || ((uintptr_t)pivot & 3)) return DVD_E_ARG;
    if (!strided_ok(n, ldx)) return DVD_E_SHAPE;
    int S, tpc;
    split(n, n, S, tpc);
    const int ni = (int)n, nt = (int)tiles(n);
    const long long npad = (long long)nt * PR_T;
    double* norm = ws;
    double* part = ws + n;
    const unsigned rows_grid = (unsigned)((n + PR_THREADS - 1) / PR_THREADS);
    prdc_norm_kernel<<<(unsigned)nt, PR_NORM_THREADS, 0, S_>>>(X, ni, d, ldx, pivot, norm);
    const unsigned grid = (unsigned)nt * (unsigned)S;
#define PAIR_(KC)                                                                                                             \
    do {                                                                                                                      \
        prdc_pair_kernel<true, KC><<<grid, PR_THREADS, 0, S_>>>(X, ldx, ni, X, ldx, ni, d, pivot, norm, norm, nullptr, tpc, nt, \
                                                                S, k, part, nullptr, nullptr);                              \
        prdc_knn_merge_kernel<KC><<<rows_grid, PR_THREADS, 0, S_>>>(part, ni, npad, S, k, r2);                                \
    } while (0)
    if (k <= 4) PAIR_(4);
    else if (k <= 8) PAIR_(8);
    else PAIR_(16);
#undef PAIR_
    return launch_status();
}

extern "C" long long dvd_prdc_ball_ws_doubles(long long nq, long long nr) {
    if (nq < 1 || nr < 1) return DVD_E_ARG;
    if (nq > DVD_PRDC_MAX_ROWS || nr > DVD_PRDC_MAX_ROWS) return DVD_E_SHAPE;
    int S, tpc;
    split(nq, nr, S, tpc);
    return nq + nr + 2ll * S * tiles(nq) * PR_T;
}

extern "C" int dvd_prdc_ball_count(const float* Q, long long nq, long long ldq, const float* R, long long nr, long long ldr, int d,
                                   const float* pivot, const double* r2, double* ws, int* count, double* dmin, void* stream) {
    if (!Q || !R || !ws || !dmin || nq < 1 || nr < 1 || (r2 == nullptr) != (count == nullptr)) return DVD_E_ARG;
    if (d < 1 || d > DVD_PRDC_MAX_D || nq > DVD_PRDC_MAX_ROWS || nr > DVD_PRDC_MAX_ROWS) return DVD_E_SHAPE;
    if (ldq < d || ldr < d || ((uintptr_t)ws & 7) || ((uintptr_t)dmin & 7) || ((uintptr_t)r2 & 7) || ((uintptr_t)count & 3)) return DVD_E_ARG;
    if (((uintptr_t)Q & 3) || ((uintptr_t)R & 3) || ((uintptr_t)pivot & 3)) return DVD_E_ARG;
    if (!strided_ok(nq, ldq) || !strided_ok(nr, ldr)) return DVD_E_SHAPE;
    int S, tpc;
    split(nq, nr, S, tpc);
    const int nqi = (int)nq, nri = (int)nr, nt = (int)tiles(nq), nct = (int)tiles(nr);
    const long long npad = (long long)nt * PR_T;
    double* norm_q = ws;
    double* norm_r = ws + nq;
    double* pcnt = norm_r + nr;
    double* pmin = pcnt + (long long)S * npad;
    prdc_norm_kernel<<<(unsigned)nt, PR_NORM_THREADS, 0, S_>>>(Q, nqi, d, ldq, pivot, norm_q);
    prdc_norm_kernel<<<(unsigned)nct, PR_NORM_THREADS, 0, S_>>>(R, nri, d, ldr, pivot, norm_r);
    prdc_pair_kernel<false, 1><<<(unsigned)nt * (unsigned)S, PR_THREADS, 0, S_>>>(Q, ldq, nqi, R, ldr, nri, d, pivot, norm_q, norm_r, r2,
                                                                                  tpc, nct, S, 0, nullptr, pcnt, pmin);
    prdc_ball_merge_kernel<<<(unsigned)((nq + PR_THREADS - 1) / PR_THREADS), PR_THREADS, 0, S_>>>(pcnt, pmin, nqi, npad, S, count, dmin);
    return launch_status();
}
