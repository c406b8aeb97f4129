// dvdx_cls_update (include/dvdx_cls.h), built into libdvdx_cls.so: the sums behind the Inception Score and the class-fidelity
// metrics of a classifier's logits.  Three launches: a wave per row (max, log-sum-exp, sum p log p, argmax, rank -> workspace), an
// owner per (split, column) of the fp64 state that adds the call's rows in a fixed order, and an owner per element of the
// confusion matrix.  Everything is fp64 with libm exp / log: 50 000 x 101 logits are 20 MB, accuracy is what this path is for.
// No atomics, no LDS beyond one 2 KiB exchange, 64-bit row indices.
#include "../../csrc/common.h"
#include "../../../include/dvdx_cls.h"

// the header states every expression operation by operation
#pragma clang fp contract(off)

namespace {

typedef _Float16 f16_t;   // raw storage of fp16 logits (bf16_t is an unsigned short)

constexpr int kRowWaves = 4;    // launch 1: rows (waves) of a workgroup
constexpr int kPhases = 4;      // launch 2: waves of a workgroup, each on every fourth row
constexpr int kCols = 64;       // launch 2: columns of a workgroup
constexpr int kRec = 4;         // doubles of a row record: m, logZ, sum_c p log p, logp of the label
constexpr int kGood = 1, kBad = 2, kLabelled = 4, kTop1 = 8, kTop5 = 16, kBadLabel = 32;   // flags of a row

template <typename T> __device__ __forceinline__ float ldl(const T* p);
template <> __device__ __forceinline__ float ldl<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldl<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }
template <> __device__ __forceinline__ float ldl<f16_t>(const f16_t* p) { return (float)*p; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// row i of the call -> rec[kRec * i ..] and info[2 * i] = argmax, info[2 * i + 1] = flags; one wave per row
template <typename T>
__global__ __launch_bounds__(64 * kRowWaves) void cls_row_kernel(const T* __restrict__ logits, const int* __restrict__ labels,
                                                                 long long rows, int C, double* __restrict__ rec,
                                                                 int* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * kRowWaves + (threadIdx.x >> 6);
    if (i >= rows) return;                                  // the whole wave: nothing below waits for another wave
    const T* row = logits + i * C;
    const int y = labels ? labels[i] : -1;
    const bool in_range = labels && y >= 0 && y < C;
    const float ly = in_range ? ldl(row + y) : 0.f;
    // pass 1 on the stored values: maximum, its lowest index, non-finite values, the label's rank
    float best = -__builtin_inff();
    int arg = 0x7fffffff, bad = 0, rank = 0;
    for (int c = lane; c < C; c += 64) {
        const float v = ldl(row + c);
        bad |= finite_f(v) ? 0 : 1;
        if (v > best) {
            best = v;
            arg = c;
        }
        if (in_range) rank += (v > ly || (v == ly && c < y)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ov > best || (ov == best && oa < arg)) {
            best = ov;
            arg = oa;
        }
    }
    bad = wave_sum_i(bad);
    rank = wave_sum_i(rank);
    if (bad) {
        if (lane == 0) {
            rec[kRec * i] = rec[kRec * i + 1] = rec[kRec * i + 2] = rec[kRec * i + 3] = 0.0;
            info[2 * i] = -1;
            info[2 * i + 1] = kBad;
        }
        return;
    }
    const double m = (double)best;
    // pass 2: log-sum-exp
    double z = 0.0;
    for (int c = lane; c < C; c += 64) z += exp((double)ldl(row + c) - m);
    const double logz = log(wave_sum_d(z));
    // pass 3: sum_c p log p with p = exp(logp)
    double a = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double lp = ((double)ldl(row + c) - m) - logz;
        a += exp(lp) * lp;
    }
    a = wave_sum_d(a);
    if (lane == 0) {
        int flags = kGood;
        if (in_range) flags |= kLabelled | (rank == 0 ? kTop1 : 0) | (rank < 5 ? kTop5 : 0);
        else if (labels) flags |= kBadLabel;
        rec[kRec * i] = m;
        rec[kRec * i + 1] = logz;
        rec[kRec * i + 2] = a;
        rec[kRec * i + 3] = in_range ? ((double)ly - m) - logz : 0.0;
        info[2 * i] = arg;
        info[2 * i + 1] = flags;
    }
}

__device__ __forceinline__ long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// workgroup (bx, by): the columns 64 * bx .. of the state row of split s_first + by; adjacent lanes on adjacent classes
template <typename T>
__global__ __launch_bounds__(kCols * kPhases) void cls_split_kernel(const T* __restrict__ logits, const double* __restrict__ rec,
                                                                    const int* __restrict__ info, long long rows, int C,
                                                                    long long row0, long long n_total, int S, int s_first,
                                                                    double* __restrict__ state) {
    __shared__ double sh[kPhases][kCols];
    const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int col = blockIdx.x * kCols + tx, width = C + DVDX_CLS_NSTAT;
    const long long s = s_first + (int)blockIdx.y;
    long long lo = ceil_div(s * n_total, S) - row0, hi = ceil_div((s + 1) * n_total, S) - row0;
    lo = lo < 0 ? 0 : lo;
    hi = hi > rows ? rows : hi;
    double acc = 0.0;
    if (col < C) {
        for (long long i = lo + q; i < hi; i += kPhases)
            if (info[2 * i + 1] & kGood) acc += exp(((double)ldl(logits + i * C + col) - rec[kRec * i]) - rec[kRec * i + 1]);
    } else if (col < width) {
        const int k = col - C;
        const int flag = k == DVDX_CLS_STAT_N || k == DVDX_CLS_STAT_A ? kGood
                         : k == DVDX_CLS_STAT_BAD                     ? kBad
                         : k == DVDX_CLS_STAT_TOP1                    ? kTop1
                         : k == DVDX_CLS_STAT_TOP5                    ? kTop5
                         : k == DVDX_CLS_STAT_BAD_LABEL               ? kBadLabel
                                                                      : kLabelled;
        const int field = k == DVDX_CLS_STAT_A ? 2 : k == DVDX_CLS_STAT_LOGLIK ? 3 : -1;     // a sum of a record's field, or a count
        for (long long i = lo + q; i < hi; i += kPhases)
            if (info[2 * i + 1] & flag) acc += field < 0 ? 1.0 : rec[kRec * i + field];
    }
    sh[q][tx] = acc;
    __syncthreads();
    if (q == 0 && col < width) {
        double total = sh[0][tx];
#pragma unroll
        for (int k = 1; k < kPhases; ++k) total += sh[k][tx];
        state[s * width + col] += total;
    }
}

// workgroup y: row y of the matrix, thread t its columns t, t + 64, ...
__global__ __launch_bounds__(64) void cls_confusion_kernel(const int* __restrict__ labels, const int* __restrict__ info, long long rows,
                                                           int C, long long* __restrict__ confusion) {
    const int y = blockIdx.x, t = threadIdx.x;
    long long* out = confusion + (long long)y * C;
    for (long long i = 0; i < rows; ++i) {
        if (labels[i] != y || !(info[2 * i + 1] & kLabelled)) continue;
        const int a = info[2 * i];
        if ((a & 63) == t) out[a] += 1;
    }
}

template <typename T>
void launch(const void* logits, const int* labels, long long rows, int C, long long row0, long long n_total, int S, double* state,
            long long* confusion, void* ws, hipStream_t stream) {
    double* rec = (double*)ws;
    int* info = (int*)(rec + kRec * rows);
    const T* l = (const T*)logits;
    cls_row_kernel<T><<<cdiv(rows, kRowWaves), 64 * kRowWaves, 0, stream>>>(l, labels, rows, C, rec, info);
    const int s_first = (int)((row0 * S) / n_total), s_last = (int)(((row0 + rows - 1) * S) / n_total);
    const dim3 grid(cdiv(C + DVDX_CLS_NSTAT, kCols), (unsigned)(s_last - s_first + 1));
    cls_split_kernel<T><<<grid, kCols * kPhases, 0, stream>>>(l, rec, info, rows, C, row0, n_total, S, s_first, state);
    if (confusion) cls_confusion_kernel<<<(unsigned)C, 64, 0, stream>>>(labels, info, rows, C, confusion);
}

bool counts_ok(long long rows, int classes) {
    return rows >= 1 && classes >= 1 && rows <= DVDX_CLS_MAX_ROWS && classes <= DVDX_CLS_MAX_CLASSES;
}

}  // namespace

static_assert(DVDX_CLS_ROW_BYTES == kRec * sizeof(double) + 2 * sizeof(int), "the workspace record");

extern "C" int dvdx_cls_abi_version(void) { return DVDX_CLS_ABI_VERSION; }

extern "C" const char* dvdx_cls_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG:
        return "null logits, state or workspace pointer, a confusion matrix without labels, a workspace that is misaligned or "
               "smaller than dvdx_cls_ws_bytes, an unknown dtype, a count below one, more splits than rows, or rows past n_total";
    case DVD_E_SHAPE: return "unsupported shape: more than 4096 classes, 2^20 rows a call, 1024 splits or 2^40 rows in all";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" long long dvdx_cls_ws_bytes(long long rows, int classes) {
    return counts_ok(rows, classes) ? rows * DVDX_CLS_ROW_BYTES : 0;
}

extern "C" int dvdx_cls_update(int dtype, const void* logits, const int* labels, long long rows, int classes, long long row0,
                               long long n_total, int splits, double* state, long long* confusion, void* ws, long long ws_bytes,
                               void* stream) {
    if (!logits || !state || !ws || (confusion && !labels) || ((uintptr_t)ws & 7)) return DVD_E_ARG;
    if (dtype != DVDX_CLS_F32 && dtype != DVDX_CLS_BF16 && dtype != DVDX_CLS_F16) return DVD_E_ARG;
    if (rows < 1 || classes < 1 || n_total < 1 || splits < 1 || row0 < 0) return DVD_E_ARG;
    if (!counts_ok(rows, classes) || splits > DVDX_CLS_MAX_SPLITS || n_total > DVDX_CLS_MAX_TOTAL) return DVD_E_SHAPE;
    if (splits > n_total || row0 > n_total - rows) return DVD_E_ARG;
    if (ws_bytes < rows * DVDX_CLS_ROW_BYTES) return DVD_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == DVDX_CLS_F32) launch<float>(logits, labels, rows, classes, row0, n_total, splits, state, confusion, ws, st);
    else if (dtype == DVDX_CLS_BF16) launch<bf16_t>(logits, labels, rows, classes, row0, n_total, splits, state, confusion, ws, st);
    else launch<f16_t>(logits, labels, rows, classes, row0, n_total, splits, state, confusion, ws, st);
    return launch_status();
}
