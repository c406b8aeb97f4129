// libdvdgan_hip_sv.so (include/dvdgan_hip_sv.h): block power iteration with a Rayleigh-Ritz finish over a table of fp32 matrices, in
// fp64.  Four kernels, each launched once for the whole table (an item's workgroups are found by bisecting the planner columns):
//   sv_wv_kernel    Y = W V      waves own rows, lanes stride along w in 16-byte chunks (a chunk is 4-byte aligned only: the
//                                compiler picks the widest load that alignment allows), V comes from L2
//   sv_wtv_kernel   Z = W^T Y    a workgroup owns 64 columns and walks the rows, coalesced along w
//   sv_orth_kernel  Gram-Schmidt with a second pass, one workgroup of 1024 threads per item; a thread reads only rows it wrote itself
//   sv_ritz_kernel  Jacobi SVD of R, residuals, fro2 and sn_sigma: one wave per item
// The memory-bound passes carry 8 or 16 fp64 FMAs per 4 bytes of W; all sums have the fixed orders the header states.
#include "../common.h"
#include "../../../include/dvdgan_hip_sv.h"

namespace {

constexpr int kThreads = 256, kWaves = 4, kStrip = 64;
constexpr int kOrthThreads = 1024, kOrthWaves = 16;      // one workgroup per item: its speed is the loads it keeps in flight

struct __attribute__((packed, aligned(4))) F4 { float a, b, c, d; };      // 16 bytes of a row at any float offset

__host__ __device__ constexpr int rows_per_wave(int bp) { return 32 / bp; }        // 4 (bp 8) or 2 (bp 16)

__device__ __forceinline__ int find_item(const dvd_sv_item* it, int n, int blk, int which) {
    int lo = 0, hi = n - 1;                      // the last item whose first workgroup is <= blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int first = which == 0 ? it[mid].blk_wv : it[mid].blk_wtv;
        if (first <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ double* state_V(const dvd_sv_item& it, double* state, int bp) { return state + it.state_off; }
__device__ __forceinline__ double* state_Y(const dvd_sv_item& it, double* state, int bp) {
    return state + it.state_off + (long long)it.w * bp;
}
__device__ __forceinline__ double* state_R(const dvd_sv_item& it, double* state, int bp) {
    return state + it.state_off + ((long long)it.w + it.h) * bp;
}

// ---------------------------------------------------------------------------------------------------------------- Y = W V
// EXTRA: the finish's product, into the workspace, with the two extra sums per row
template <int BP, bool EXTRA>
__global__ __launch_bounds__(kThreads) void sv_wv_kernel(const dvd_sv_item* items, int n, double* state, double* ws) {
    constexpr int ROWS = rows_per_wave(BP);
    const int k = find_item(items, n, blockIdx.x, 0);
    const dvd_sv_item it = items[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = ((blockIdx.x - it.blk_wv) * kWaves + wave) * ROWS;
    if (row0 >= it.h) return;
    const int w = it.w, n4 = w >> 2;
    const double* V = state_V(it, state, BP);
    const float* wr[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) wr[r] = it.W + (size_t)min(row0 + r, it.h - 1) * w;      // a row past the end re-reads the last
    double acc[ROWS][BP], ax[ROWS], sq[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        ax[r] = 0.0; sq[r] = 0.0;
#pragma unroll
        for (int c = 0; c < BP; ++c) acc[r][c] = 0.0;
    }
    for (int ch = lane; ch < n4; ch += 64) {
        float x[ROWS][4];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const F4 f = *reinterpret_cast<const F4*>(wr[r] + 4 * ch);
            x[r][0] = f.a; x[r][1] = f.b; x[r][2] = f.c; x[r][3] = f.d;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double* vj = V + (size_t)(4 * ch + j) * BP;
            double vv[BP];
#pragma unroll
            for (int c = 0; c < BP; ++c) vv[c] = vj[c];
            const double vs = EXTRA && it.v ? (double)it.v[4 * ch + j] : 0.0;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const double xv = (double)x[r][j];
#pragma unroll
                for (int c = 0; c < BP; ++c) acc[r][c] += xv * vv[c];
                if (EXTRA) { ax[r] += xv * vs; sq[r] += xv * xv; }
            }
        }
    }
    const int col = 4 * n4 + lane;
    if (col < w) {                              // the w mod 4 last columns: lanes 0..2
        const double* vj = V + (size_t)col * BP;
        const double vs = EXTRA && it.v ? (double)it.v[col] : 0.0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double xv = (double)wr[r][col];
#pragma unroll
            for (int c = 0; c < BP; ++c) acc[r][c] += xv * vj[c];
            if (EXTRA) { ax[r] += xv * vs; sq[r] += xv * xv; }
        }
    }
    double* out = EXTRA ? ws + it.ws_off : state_Y(it, state, BP);
    double* aux = ws + it.ws_off + (long long)it.h * BP;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
#pragma unroll
        for (int c = 0; c < BP; ++c) acc[r][c] = wave_sum_d(acc[r][c]);
        if (EXTRA) { ax[r] = wave_sum_d(ax[r]); sq[r] = wave_sum_d(sq[r]); }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int row = row0 + r;
            if (row < it.h) {
#pragma unroll
                for (int c = 0; c < BP; ++c) out[(size_t)row * BP + c] = acc[r][c];
                if (EXTRA) { aux[2 * (size_t)row] = ax[r]; aux[2 * (size_t)row + 1] = sq[r]; }
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- Z = W^T Y
template <int BP>
__global__ __launch_bounds__(kThreads) void sv_wtv_kernel(const dvd_sv_item* items, int n, double* state) {
    __shared__ double part[kWaves - 1][kStrip][BP + 1];
    const int k = find_item(items, n, blockIdx.x, 1);
    const dvd_sv_item it = items[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (blockIdx.x - it.blk_wtv) * kStrip + lane;
    const bool live = col < it.w;
    const float* wc = it.W + (live ? col : it.w - 1);
    const double* Y = state_Y(it, state, BP);
    double acc[BP];
#pragma unroll
    for (int c = 0; c < BP; ++c) acc[c] = 0.0;
#pragma unroll 4
    for (int row = wave; row < it.h; row += kWaves) {
        const double xv = (double)wc[(size_t)row * it.w];
        const double* yr = Y + (size_t)row * BP;
#pragma unroll
        for (int c = 0; c < BP; ++c) acc[c] += xv * yr[c];
    }
    if (wave > 0) {
#pragma unroll
        for (int c = 0; c < BP; ++c) part[wave - 1][lane][c] = acc[c];
    }
    __syncthreads();
    if (wave == 0 && live) {
        double* Z = state_V(it, state, BP) + (size_t)col * BP;
#pragma unroll
        for (int c = 0; c < BP; ++c) Z[c] = ((acc[c] + part[0][lane][c]) + part[1][lane][c]) + part[2][lane][c];
    }
}

// ------------------------------------------------------------------------------------------------------------------- orth
// sums of BP values over the workgroup, in `tot` (LDS) afterwards: butterfly per wave, then waves 0, 1, .. 15
template <int BP>
__device__ __forceinline__ void wg_sums(double (&s)[BP], double (*part)[BP], double* tot) {
#pragma unroll
    for (int c = 0; c < BP; ++c) s[c] = wave_sum_d(s[c]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                            // the readers of the previous totals are done
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < BP; ++c) part[wave][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < BP) {
        double t = part[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kOrthWaves; ++q) t += part[q][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
}

// which = 0: the item's Y [h][BP];  1: its V [w][BP], R written
template <int BP>
__global__ __launch_bounds__(kOrthThreads) void sv_orth_kernel(const dvd_sv_item* items, double* state, int which) {
    __shared__ double part[kOrthWaves][BP], tot[BP], Rs[BP][BP];
    const dvd_sv_item it = items[blockIdx.x];
    double* A = which ? state_V(it, state, BP) : state_Y(it, state, BP);
    const int rows = which ? it.w : it.h, tid = threadIdx.x;
    for (int i = tid; i < BP * BP; i += kOrthThreads) (&Rs[0][0])[i] = 0.0;
    double s[BP];
#pragma unroll
    for (int c = 0; c < BP; ++c) s[c] = 0.0;
    for (int row = tid; row < rows; row += kOrthThreads) {
#pragma unroll
        for (int c = 0; c < BP; ++c) { const double a = A[(size_t)row * BP + c]; s[c] += a * a; }
    }
    wg_sums<BP>(s, part, tot);
    double big = 0.0;
#pragma unroll
    for (int c = 0; c < BP; ++c) big = fmax(big, tot[c]);
    const double limit = 0x1p-40 * sqrt(big);
    for (int j = 0; j < BP; ++j) {
        double nrm2 = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int c = 0; c < BP; ++c) s[c] = 0.0;
            for (int row = tid; row < rows; row += kOrthThreads) {
                const double* a = A + (size_t)row * BP;
                const double aj = a[j];
#pragma unroll
                for (int c = 0; c < BP; ++c) s[c] += a[c] * aj;
            }
            wg_sums<BP>(s, part, tot);
            double cf[BP];
#pragma unroll
            for (int c = 0; c < BP; ++c) cf[c] = c < j ? tot[c] : 0.0;
            if (tid < j) Rs[tid][j] += tot[tid];
            nrm2 = 0.0;
            for (int row = tid; row < rows; row += kOrthThreads) {
                double* a = A + (size_t)row * BP;
                double p = 0.0;
#pragma unroll
                for (int c = 0; c < BP; ++c) p += cf[c] * a[c];
                const double v = a[j] - p;
                a[j] = v;
                nrm2 += v * v;
            }
        }
#pragma unroll
        for (int c = 1; c < BP; ++c) s[c] = 0.0;
        s[0] = nrm2;
        wg_sums<BP>(s, part, tot);
        const double nrm = sqrt(tot[0]);
        const bool drop = !(nrm > limit);
        const double inv = drop ? 0.0 : 1.0 / nrm;
        if (tid == 0) Rs[j][j] = drop ? 0.0 : nrm;
        for (int row = tid; row < rows; row += kOrthThreads) {
            double* a = A + (size_t)row * BP + j;
            *a = drop ? 0.0 : *a * inv;
        }
    }
    __syncthreads();
    if (which) {
        double* R = state_R(it, state, BP);
        for (int i = tid; i < BP * BP; i += kOrthThreads) R[i] = (&Rs[0][0])[i];
    }
}

// ------------------------------------------------------------------------------------------------------------- the finish
template <int BP>
__global__ __launch_bounds__(64) void sv_ritz_kernel(const dvd_sv_item* items, int n, const double* state, const double* ws, double* out,
                                                      int kout) {
    __shared__ double M[BP][BP + 1], J[BP][BP + 1], sg[BP], cv[BP][BP], cu[BP][BP], sgs[BP], fin[BP + 2], red[64 / BP][BP + 2];
    __shared__ int perm[BP];
    const dvd_sv_item it = items[blockIdx.x];
    const int tid = threadIdx.x;
    const double* V0 = state + it.state_off;
    const double* Y = V0 + (long long)it.w * BP;
    const double* R = Y + (long long)it.h * BP;
    for (int i = tid; i < BP * BP; i += 64) {
        M[i / BP][i % BP] = R[i];
        J[i / BP][i % BP] = (i / BP == i % BP) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sweep = 0; sweep < DVD_SV_MAX_SWEEPS; ++sweep) {
        bool any = false;
        for (int p = 0; p < BP - 1; ++p) {
            for (int q = p + 1; q < BP; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int t = 0; t < BP; ++t) {
                    const double mp = M[t][p], mq = M[t][q];
                    al += mp * mp; be += mq * mq; ga += mp * mq;
                }
                const bool rot = fabs(ga) > 0x1p-50 * sqrt(al * be);          // the same bits in every lane
                __syncthreads();
                if (rot) {
                    any = true;
                    const double ze = (be - al) / (2.0 * ga);
                    const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                    if (tid < BP) {
                        const double mp = M[tid][p], mq = M[tid][q], jp = J[tid][p], jq = J[tid][q];
                        M[tid][p] = c * mp - s * mq; M[tid][q] = s * mp + c * mq;
                        J[tid][p] = c * jp - s * jq; J[tid][q] = s * jp + c * jq;
                    }
                }
                __syncthreads();
            }
        }
        if (!any) break;
    }
    if (tid < BP) {
        double a = 0.0;
#pragma unroll
        for (int t = 0; t < BP; ++t) a += M[t][tid] * M[t][tid];
        sg[tid] = sqrt(a);
    }
    if (tid < BP) perm[tid] = tid;              // a NaN among the values leaves ranks untaken: every entry stays a column
    __syncthreads();
    if (tid < BP) {
        int rank = 0;
        for (int c = 0; c < BP; ++c) rank += (sg[c] > sg[tid] || (sg[c] == sg[tid] && c < tid)) ? 1 : 0;
        perm[rank] = tid;
    }
    __syncthreads();
    for (int i = tid; i < BP * BP; i += 64) {
        const int t = i / BP, r = i % BP, c = perm[r];
        cv[t][r] = sg[c] > 0.0 ? M[t][c] / sg[c] : 0.0;
        cu[t][r] = J[t][c];
        if (t == 0) sgs[r] = sg[c];
    }
    __syncthreads();
    // residuals, fro2, sn_sigma: thread (g, i) = (tid / BP, tid % BP) takes value i on rows g, g + G, ... in ascending order; the G
    // partial sums of a value are added in the order 0 .. G - 1
    constexpr int G = 64 / BP;
    const double* P = ws + it.ws_off;
    const double* aux = P + (long long)it.h * BP;
    const int g = tid / BP, i = tid % BP;
    double cvi[BP], cui[BP];
#pragma unroll
    for (int c = 0; c < BP; ++c) { cvi[c] = cv[c][i]; cui[c] = cu[c][i]; }
    const double sgi = sgs[i];
    double rs = 0.0, fro = 0.0, sn = 0.0;
    for (int row = g; row < it.h; row += G) {
        const double* p = P + (size_t)row * BP;
        const double* y = Y + (size_t)row * BP;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int c = 0; c < BP; ++c) { a += p[c] * cvi[c]; b += y[c] * cui[c]; }
        const double d = a - sgi * b;
        rs += d * d;
        if (i == 0) {
            fro += aux[2 * (size_t)row + 1];
            if (it.u) sn += (double)it.u[row] * aux[2 * (size_t)row];
        }
    }
    red[g][i] = rs;
    if (i == 0) { red[g][BP] = fro; red[g][BP + 1] = sn; }
    __syncthreads();
    if (tid < BP + 2) {
        double t = 0.0;
        for (int q = 0; q < G; ++q) t += red[q][tid];
        fin[tid] = tid < BP ? sqrt(t) : t;
    }
    __syncthreads();
    if (tid == 0 && !(it.u && it.v)) fin[BP + 1] = __builtin_nan("");
    __syncthreads();
    double* o = out + (size_t)it.slot * (2 * kout + 2);
    if (tid < kout) { o[tid] = sgs[tid]; o[kout + tid] = fin[tid]; }
    if (tid == 0) { o[2 * kout] = fin[BP]; o[2 * kout + 1] = fin[BP + 1]; }
}

// ------------------------------------------------------------------------------------------------------------------- host
int stored_width(int block) { return block <= 8 ? 8 : 16; }

struct Plan { long long state, ws, g_wv, g_wtv; };

// what dvd_sv_prepare checks and computes; `fill` writes the planner columns, otherwise they are compared
int plan(dvd_sv_item* fill, const dvd_sv_item* items, int n, int block, Plan* out) {
    if (!items || n < 1 || n > DVD_SV_MAX_ITEMS || block < 1 || block > DVD_SV_MAX_BLOCK) return DVD_E_ARG;
    const int bp = stored_width(block), rows = kWaves * rows_per_wave(bp);
    Plan p = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const dvd_sv_item& it = items[i];
        if (!it.W || (it.u == nullptr) != (it.v == nullptr) || it.slot < 0 || it.slot >= n) return DVD_E_ARG;
        if (it.h < 1 || it.w < 1) return DVD_E_SHAPE;
    }
    {
        unsigned char seen[DVD_SV_MAX_ITEMS] = {0};
        for (int i = 0; i < n; ++i) {
            if (seen[items[i].slot]) return DVD_E_ARG;
            seen[items[i].slot] = 1;
        }
    }
    for (int i = 0; i < n; ++i) {
        const dvd_sv_item& it = items[i];
        if (fill) {
            fill[i].state_off = p.state; fill[i].ws_off = p.ws; fill[i].blk_wv = (int)p.g_wv; fill[i].blk_wtv = (int)p.g_wtv;
            fill[i].pad_ = 0;
        } else if (it.state_off != p.state || it.ws_off != p.ws || it.blk_wv != p.g_wv || it.blk_wtv != p.g_wtv) {
            return DVD_E_ARG;
        }
        p.state += ((long long)it.w + it.h + bp) * bp;
        p.ws += (long long)it.h * (bp + 2);
        p.g_wv += (it.h + rows - 1) / rows;
        p.g_wtv += (it.w + kStrip - 1) / kStrip;
        if (p.g_wv > 0x7fffffffll || p.g_wtv > 0x7fffffffll) return DVD_E_SHAPE;
    }
    *out = p;
    return DVD_OK;
}

template <int BP>
int run_orth(const dvd_sv_item* items, int n, double* state, int which, hipStream_t s) {
    sv_orth_kernel<BP><<<n, kOrthThreads, 0, s>>>(items, state, which);
    return launch_status();
}

template <int BP>
int run_iterate(const dvd_sv_item* items, int n, const Plan& p, int iters, double* state, hipStream_t s) {
    for (int t = 0; t < iters; ++t) {
        sv_wv_kernel<BP, false><<<(unsigned)p.g_wv, kThreads, 0, s>>>(items, n, state, nullptr);
        sv_orth_kernel<BP><<<n, kOrthThreads, 0, s>>>(items, state, 0);
        sv_wtv_kernel<BP><<<(unsigned)p.g_wtv, kThreads, 0, s>>>(items, n, state);
        sv_orth_kernel<BP><<<n, kOrthThreads, 0, s>>>(items, state, 1);
        if (launch_status() != DVD_OK) return DVD_E_LAUNCH;
    }
    return DVD_OK;
}

template <int BP>
int run_ritz(const dvd_sv_item* items, int n, const Plan& p, int k, const double* state, double* ws, double* out, hipStream_t s) {
    sv_wv_kernel<BP, true><<<(unsigned)p.g_wv, kThreads, 0, s>>>(items, n, const_cast<double*>(state), ws);
    sv_ritz_kernel<BP><<<n, 64, 0, s>>>(items, n, state, ws, out, k);
    return launch_status();
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvd_sv_abi_version(void) { return DVD_SV_ABI_VERSION; }

extern "C" int dvd_sv_item_size(void) { return (int)sizeof(dvd_sv_item); }

extern "C" const char* dvd_sv_strerror(int code) {
    switch (code) {
    case DVD_OK: return "ok";
    case DVD_E_ARG:
        return "null pointer, n outside [1, 65535], block outside [1, 16], k outside [1, block], iters outside [0, 4096], row outside "
               "the ring, an item with a null W, half a u / v pair or a bad slot, or a table dvd_sv_prepare did not fill";
    case DVD_E_SHAPE: return "unsupported shape: h < 1, w < 1 or more than 2147483647 workgroups in a launch";
    case DVD_E_LAUNCH: return "kernel launch failed";
    default: return "unknown error";
    }
}

extern "C" int dvd_sv_prepare(dvd_sv_item* items, int n, int block, long long* state_doubles, long long* ws_doubles) {
    if (!state_doubles || !ws_doubles) return DVD_E_ARG;
    Plan p;
    const int bad = plan(items, items, n, block, &p);
    if (bad != DVD_OK) return bad;
    *state_doubles = p.state;
    *ws_doubles = p.ws;
    return DVD_OK;
}

extern "C" int dvd_sv_init(const dvd_sv_item* items, const dvd_sv_item* host, int n, int block, const double* start, double* state,
                           void* stream) {
    Plan p;
    const int bad = plan(nullptr, host, n, block, &p);
    if (bad != DVD_OK) return bad;
    if (!items || !start || !state || start == state) return DVD_E_ARG;
    if (hipMemcpyAsync(state, start, (size_t)p.state * sizeof(double), hipMemcpyDeviceToDevice, S_) != hipSuccess) return DVD_E_LAUNCH;
    return stored_width(block) == 8 ? run_orth<8>(items, n, state, 1, S_) : run_orth<16>(items, n, state, 1, S_);
}

extern "C" int dvd_sv_iterate(const dvd_sv_item* items, const dvd_sv_item* host, int n, int block, int iters, double* state,
                              void* stream) {
    Plan p;
    const int bad = plan(nullptr, host, n, block, &p);
    if (bad != DVD_OK) return bad;
    if (!items || !state || iters < 0 || iters > DVD_SV_MAX_ITERS) return DVD_E_ARG;
    return stored_width(block) == 8 ? run_iterate<8>(items, n, p, iters, state, S_) : run_iterate<16>(items, n, p, iters, state, S_);
}

extern "C" int dvd_sv_ritz(const dvd_sv_item* items, const dvd_sv_item* host, int n, int block, int k, const double* state, double* ws,
                           double* out, long long row, long long n_rows, void* stream) {
    Plan p;
    const int bad = plan(nullptr, host, n, block, &p);
    if (bad != DVD_OK) return bad;
    if (!items || !state || !ws || !out || k < 1 || k > block || n_rows < 1 || row < 0 || row >= n_rows) return DVD_E_ARG;
    double* o = out + (size_t)row * n * (2 * k + 2);
    return stored_width(block) == 8 ? run_ritz<8>(items, n, p, k, state, ws, o, S_) : run_ritz<16>(items, n, p, k, state, ws, o, S_);
}
