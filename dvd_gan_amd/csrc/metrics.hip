// Prediction metrics: per-frame MSE and SSIM (Wang et al. 2004) of predicted frames against held-out real ones, one pass.
//
// One workgroup owns a whole frame: it walks the C planes, and each plane from top to bottom in steps of S rows.  Per step:
//   stage   S new rows of both operands -> LDS (denorm / 8-bit quantisation on load, (p - t)^2 summed here: every pixel is loaded
//           exactly once), stored CENTRED (x - 0.5): the second moments E[x^2] - mu^2 then cancel a quarter of what they cancel on
//           pixels near 1, and the variances do not move;
//   h-pass  the 11-tap Gaussian along the row over x, y, x^2, y^2, xy, four neighbouring windows per thread from four 16-byte
//           LDS reads per operand -> five moments per window, side by side, written into a RING of S + 10 rows;
//   v-pass  the 11 taps down the ring for the output rows that became complete (four rows per thread, one column per lane), the
//           SSIM expression, summed per thread in fp64.
// The ring holds the 10-row overlap between neighbouring strips, so nothing is filtered or read twice.  S comes from the row
// width (metrics_plan): 16 rows up to 130 pixels, then 12, 8 and from 199 pixels 4.  The per-frame sums are reduced in a fixed order (lanes by xor
// shuffles, then the four waves in order) and one thread writes mse[f] and ssim[f]: no atomics, nothing depends on how many
// frames the launch has or on which CU a frame lands.
#include <atomic>
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int MET_TAPS = 11, MET_RB = 4, MET_THREADS = 256;
constexpr int MET_LDS_MAX = 80 * 1024;         // two workgroups per CU at the widest rows
constexpr float MET_C1 = 0.01f * 0.01f, MET_C2 = 0.03f * 0.03f, MET_CENTRE = 0.5f;

struct GaussWin { float w[MET_TAPS / 2 + 1]; };       // the window is symmetric: taps 0 .. 5, tap t > 5 is tap 10 - t

struct MetK {
    const float* p; const float* t;
    long long psb, pst, psc, tsb, tst, tsc, F;
    int T, C, H, W, flags, S, vec;
    float* mse; float* ssim;
    GaussWin g;
};

// LDS floats of one workgroup: 8 doubles of reduction scratch, 2 x [S][Pin] staged rows, the ring [S + 10][Wq][5]
static inline int met_wq(int W) { return (W - (MET_TAPS - 1) + 3) & ~3; }      // windows per row, in whole float4
static inline int met_pin(int W) { return met_wq(W) + 12; }                    // staged row: the last float4 of windows reads 16 pixels
static inline long long met_lds_bytes(int W, int S) {
    return 64 + 4ll * (2ll * S * met_pin(W) + 5ll * (S + MET_TAPS - 1) * met_wq(W));
}
static inline int metrics_plan(int H, int W) {
    // S >= 4 always (S = 4 fits at the widest row, H >= 11): the ring has at least 14 rows, which the v-pass relies on
    static const int cand[] = {16, 12, 8, 4};
    for (int s : cand)
        if (met_lds_bytes(W, s) <= MET_LDS_MAX) return s < H ? s : H;
    return 0;
}

__device__ __forceinline__ float met_prep(float v, int flags) {
    if (flags & DVD_METRICS_SIGNED) v = fminf(fmaxf((v + 1.f) * 0.5f, 0.f), 1.f);
    if (flags & DVD_METRICS_QUANTIZE) v = rintf(255.f * v) / 255.f;
    return v;
}

__global__ __launch_bounds__(MET_THREADS) void frame_metrics_kernel(const MetK k) {
    extern __shared__ double met_lds[];
    const int W = k.W, H = k.H, S = k.S, Wout = W - (MET_TAPS - 1), Hout = H - (MET_TAPS - 1);
    const int Wq = (Wout + 3) & ~3, nq = Wq >> 2, Pin = Wq + 12, pq = Pin >> 2, R = S + MET_TAPS - 1;
    double* red = met_lds;
    float* inx = reinterpret_cast<float*>(met_lds + 8);
    float* iny = inx + S * Pin;
    float* maps = iny + S * Pin;
    const int rowf = 5 * Wq;                       // ring row: [window][x, y, xx, yy, xy], the five moments of a window side by side
    const int tid = threadIdx.x;

    for (long long f = blockIdx.x; f < k.F; f += gridDim.x) {
        const long long b = f / k.T, tt = f % k.T;
        double acc_mse = 0.0, acc_ssim = 0.0;
        for (int c = 0; c < k.C; ++c) {
            const float* px = k.p + b * k.psb + tt * k.pst + c * k.psc;
            const float* py = k.t + b * k.tsb + tt * k.tst + c * k.tsc;
            int o_done = 0;
            for (int r0 = 0; r0 < H; r0 += S) {
                const int nrows = min(S, H - r0);
                // ---- stage
                if (k.vec) {
                    for (int i = tid; i < nrows * pq; i += MET_THREADS) {
                        const int r = i / pq, col = (i - r * pq) * 4;
                        f32x4 a = {0.f, 0.f, 0.f, 0.f}, bb = a;
                        if (col < W) {                                   // W % 4 == 0 here: whole vectors or none
                            const long long off = (long long)(r0 + r) * W + col;
                            a = *reinterpret_cast<const f32x4*>(px + off);
                            bb = *reinterpret_cast<const f32x4*>(py + off);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float xv = met_prep(a[e], k.flags), yv = met_prep(bb[e], k.flags), d = xv - yv;
                                acc_mse += (double)d * (double)d;
                                a[e] = xv - MET_CENTRE;
                                bb[e] = yv - MET_CENTRE;
                            }
                        }
                        *reinterpret_cast<f32x4*>(inx + r * Pin + col) = a;
                        *reinterpret_cast<f32x4*>(iny + r * Pin + col) = bb;
                    }
                } else {
                    for (int i = tid; i < nrows * Pin; i += MET_THREADS) {
                        const int r = i / Pin, col = i - r * Pin;
                        float a = 0.f, bb = 0.f;
                        if (col < W) {
                            const long long off = (long long)(r0 + r) * W + col;
                            const float xv = met_prep(px[off], k.flags), yv = met_prep(py[off], k.flags), d = xv - yv;
                            acc_mse += (double)d * (double)d;
                            a = xv - MET_CENTRE;
                            bb = yv - MET_CENTRE;
                        }
                        inx[i] = a;
                        iny[i] = bb;
                    }
                }
                __syncthreads();
                // ---- horizontal taps: windows 4 q .. 4 q + 3 of staged row r -> ring row (r0 + r) % R
                for (int i = tid; i < nrows * nq; i += MET_THREADS) {
                    const int r = i / nq, q = i - r * nq;
                    float xs[16], ys[16];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(inx + r * Pin + 4 * (q + v));
                        const f32x4 bb = *reinterpret_cast<const f32x4*>(iny + r * Pin + 4 * (q + v));
#pragma unroll
                        for (int e = 0; e < 4; ++e) { xs[4 * v + e] = a[e]; ys[4 * v + e] = bb[e]; }
                    }
                    f32x2 m01[4], m23[4];                        // per window: (E x, E y), (E xx, E yy), E xy
                    float m4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { m01[j] = f32x2{0.f, 0.f}; m23[j] = m01[j]; m4[j] = 0.f; }
#pragma unroll
                    for (int e = 0; e < MET_TAPS + 3; ++e) {
                        const f32x2 p01 = {xs[e], ys[e]}, p23 = p01 * p01;
                        const float p4 = xs[e] * ys[e];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int tap = e - j;
                            if (tap >= 0 && tap < MET_TAPS) {
                                const float w = k.g.w[tap <= MET_TAPS / 2 ? tap : MET_TAPS - 1 - tap];
                                m01[j] += w * p01; m23[j] += w * p23; m4[j] += w * p4;
                            }
                        }
                    }
                    float flat[20];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        flat[5 * j] = m01[j][0]; flat[5 * j + 1] = m01[j][1]; flat[5 * j + 2] = m23[j][0]; flat[5 * j + 3] = m23[j][1];
                        flat[5 * j + 4] = m4[j];
                    }
                    float* dst = maps + ((r0 + r) % R) * rowf + 20 * q;
#pragma unroll
                    for (int v = 0; v < 5; ++v)                          // 20 floats in a row: the five moments of window 0, of window 1, ...
                        *reinterpret_cast<f32x4*>(dst + 4 * v) = f32x4{flat[4 * v], flat[4 * v + 1], flat[4 * v + 2], flat[4 * v + 3]};
                }
                __syncthreads();
                // ---- vertical taps + the SSIM expression for output rows [o_done, hi - 10): their 11 input rows are in the ring
                const int o_end = r0 + nrows - (MET_TAPS - 1);
                if (o_end > o_done) {
                    const int nblk = (o_end - o_done + MET_RB - 1) / MET_RB;
                    for (int i = tid; i < nblk * Wout; i += MET_THREADS) {
                        const int blk = i / Wout, ox = i - blk * Wout;
                        const int o0 = o_done + blk * MET_RB;
                        const unsigned slot0 = o0 % R;
                        const float* col = maps + 5 * ox;
                        f32x2 a01[MET_RB], a23[MET_RB];
                        float a4[MET_RB];
#pragma unroll
                        for (int j = 0; j < MET_RB; ++j) { a01[j] = f32x2{0.f, 0.f}; a23[j] = a01[j]; a4[j] = 0.f; }
                        const float* src = col + slot0 * rowf;
                        const float* wrap = col + R * rowf;
#pragma unroll
                        for (int e = 0; e < MET_TAPS + MET_RB - 1; ++e) {
                            const f32x2 v01 = {src[0], src[1]}, v23 = {src[2], src[3]};
                            const float v4 = src[4];
                            src += rowf;
                            if (src == wrap) src = col;                          // 14 rows read, R >= 14 (metrics_plan): at most one wrap per block
#pragma unroll
                            for (int j = 0; j < MET_RB; ++j) {
                                const int tap = e - j;
                                if (tap >= 0 && tap < MET_TAPS) {
                                    const float w = k.g.w[tap <= MET_TAPS / 2 ? tap : MET_TAPS - 1 - tap];
                                    a01[j] += w * v01; a23[j] += w * v23; a4[j] += w * v4;
                                }
                            }
                        }
#pragma unroll
                        for (int j = 0; j < MET_RB; ++j) {
                            // rows past o_end were filtered over ring rows that are not theirs: computed, not counted
                            const float mxc = a01[j][0], myc = a01[j][1];
                            const float sxx = a23[j][0] - mxc * mxc, syy = a23[j][1] - myc * myc, sxy = a4[j] - mxc * myc;
                            const float mx = mxc + MET_CENTRE, my = myc + MET_CENTRE;
                            const float num = (2.f * mx * my + MET_C1) * (2.f * sxy + MET_C2);
                            const float den = (mx * mx + my * my + MET_C1) * (sxx + syy + MET_C2);
                            const float s = num / den;
                            if (o0 + j < o_end) acc_ssim += (double)s;
                        }
                    }
                    o_done = o_end;
                }
                // (the next stage writes rows the h-pass has finished with; the barrier behind it orders the next h-pass, which
                //  overwrites ring rows, after this v-pass)
            }
        }
        // ---- fixed-order reduction over the workgroup
        acc_mse = wave_sum_d(acc_mse);
        acc_ssim = wave_sum_d(acc_ssim);
        if ((tid & 63) == 0) { red[tid >> 6] = acc_mse; red[4 + (tid >> 6)] = acc_ssim; }
        __syncthreads();
        if (tid == 0) {
            const double m = ((red[0] + red[1]) + red[2]) + red[3], s = ((red[4] + red[5]) + red[6]) + red[7];
            k.mse[f] = (float)(m / ((double)k.C * H * W));
            k.ssim[f] = (float)(s / ((double)k.C * Hout * Wout));
        }
        __syncthreads();
    }
}

const GaussWin& gauss_window() {        // sigma = 1.5, normalised to sum 1 in fp64, rounded once
    static const GaussWin g = [] {
        double w[MET_TAPS], sum = 0.0;
        for (int i = 0; i < MET_TAPS; ++i) {
            const double d = i - MET_TAPS / 2;
            sum += w[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
        }
        GaussWin out;
        for (int i = 0; i <= MET_TAPS / 2; ++i) out.w[i] = (float)(w[i] / sum);
        return out;
    }();
    return g;
}

}  // namespace

extern "C" long long dvd_frame_metrics_ws_bytes(long long B, int T, int C, int H, int W) {
    (void)B; (void)T; (void)C; (void)H; (void)W;
    return 0;                           // one workgroup owns a frame: no partial sums leave it
}

extern "C" int dvd_frame_metrics(const float* pred, long long p_sb, long long p_st, long long p_sc, const float* target,
                                 long long t_sb, long long t_st, long long t_sc, long long B, int T, int C, int H, int W,
                                 int flags, float* mse, float* ssim, void* ws, void* stream) {
    (void)ws;
    if (!pred || !target || !mse || !ssim) return DVD_E_ARG;
    if (H < DVD_METRICS_MIN_SIDE || W < DVD_METRICS_MIN_SIDE || H > DVD_METRICS_MAX_SIDE || W > DVD_METRICS_MAX_SIDE)
        return DVD_E_SHAPE;
    if (C < 1 || T < 1 || B < 1 || B > (1ll << 40) / T) return DVD_E_SHAPE;
    if (flags & ~(DVD_METRICS_SIGNED | DVD_METRICS_QUANTIZE)) return DVD_E_SHAPE;
    const int S = metrics_plan(H, W);
    if (S <= 0) return DVD_E_SHAPE;
    MetK k;
    k.p = pred; k.t = target;
    k.psb = p_sb; k.pst = p_st; k.psc = p_sc; k.tsb = t_sb; k.tst = t_st; k.tsc = t_sc;
    k.F = B * T; k.T = T; k.C = C; k.H = H; k.W = W; k.flags = flags; k.S = S;
    // 16-byte loads need every plane to start on a 16-byte boundary and rows of whole vectors; anything else goes scalar
    const unsigned long long bits = (uintptr_t)pred | (uintptr_t)target |
                                    4ull * (unsigned long long)(p_sb | p_st | p_sc | t_sb | t_st | t_sc | (long long)W);
    k.vec = (bits & 15) == 0;
    k.mse = mse; k.ssim = ssim;
    k.g = gauss_window();
    const size_t lds = (size_t)met_lds_bytes(W, S);
    if (lds > 48 * 1024) {              // raised once per device to the plan's ceiling, not on every launch
        static std::atomic<unsigned long long> raised{0};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return DVD_E_LAUNCH;
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_relaxed) & bit)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(frame_metrics_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, MET_LDS_MAX) != hipSuccess)
                return DVD_E_LAUNCH;
            raised.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    const unsigned grid = (unsigned)(k.F < 65536 ? k.F : 65536);
    frame_metrics_kernel<<<grid, MET_THREADS, lds, (hipStream_t)stream>>>(k);
    return launch_status();
}
