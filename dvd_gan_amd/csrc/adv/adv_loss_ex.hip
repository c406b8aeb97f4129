// dvd_adv_loss_ex (include/dvdgan_hip_adv.h), built into libdvdgan_hip_adv.so: Trainer.calc_loss (trainer.py:114-121) with top-k
// selection, the LeCam gradient, the anchor update and the logit statistics.  fp32, one workgroup: latency-sized.
#include "../common.h"
#include "../../../include/dvdgan_hip_adv.h"

namespace {

// adv_loss_kernel's term (misc.hip; block_sum of common.h is shared, so with everything off the bits are its) -- over the samples a top-k selection keeps, when
// there is one -- plus the LeCam gradient, the anchor update and the logit statistics, in the same single workgroup.
// Selection: one thread sums a sample's logits in index order; the scores go to LDS and every thread ranks its samples by
// counting (all lanes read the same score[c]: an LDS broadcast, no bank conflict).  O(samples^2 / 1024) compares per thread.
// The seven sums are per-thread strided sums followed by block_sum, no atomics; thread 0 writes every scalar result.
__global__ __launch_bounds__(1024) void adv_loss_ex_kernel(const float* out, long long n, int group, int hinge, int real,
                                                           int keep, float lecam, const float* a_other, const float* a_prev,
                                                           float* a_next, float decay, float* loss, float* dout, float gscale,
                                                           float* stats) {
    __shared__ float sh[32];
    __shared__ float score[DVD_ADV_MAX_SAMPLES];
    __shared__ unsigned char kept[DVD_ADV_MAX_SAMPLES];
    const float sgn = real ? -1.f : 1.f;
    const int B = keep > 0 ? (int)(n / group) : 0;            // <= DVD_ADV_MAX_SAMPLES (the host checked)
    float nkept = 0.f;
    if (keep > 0) {
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            float s = 0.f;
            for (int j = 0; j < group; ++j) s += out[(long long)b * group + j];
            score[b] = s / (float)group;
        }
        __syncthreads();
        // (one sample at a time per thread: ranking a thread's up to four samples in one pass over the scores was measured and
        //  is slower, 879 against 650 us at 4096 samples and 17.7 against 8.4 us at 64 -- the loop is bound by the compares)
        for (int b = threadIdx.x; b < B; b += blockDim.x) {
            const float sb = score[b];
            int ahead = 0;                                    // a NaN compares false: nothing is ahead of it, it is ahead of nothing
            for (int c = 0; c < B; ++c) {
                const float sc = score[c];
                ahead += (sc > sb || (sc == sb && c < b)) ? 1 : 0;
            }
            kept[b] = ahead < keep;
            nkept += ahead < keep ? 1.f : 0.f;
        }
        __syncthreads();
    }
    const float div = keep > 0 ? (float)((long long)keep * group) : (float)n;
    const float anchor = a_other ? *a_other : 0.f;
    const float pen_sgn = real ? 2.f : -2.f;
    const bool want_stats = stats != nullptr, want_mean = want_stats || a_next != nullptr;
    float a = 0.f, sx = 0.f, ssign = 0.f, act = 0.f, pen = 0.f, bad = 0.f;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const float x0 = out[i];
        const float x = sgn * x0;
        const bool k = keep > 0 ? kept[i / group] != 0 : true;
        float l = hinge ? fmaxf(1.f + x, 0.f) : x;
        if (k) a += l;
        float g = k ? ((hinge && !(1.f + x > 0.f)) ? 0.f : sgn) * gscale / div : 0.f;
        if (lecam > 0.f) {
            const float r = fmaxf(real ? x0 - anchor : anchor - x0, 0.f);
            pen += r * r;
            g += gscale * lecam * (pen_sgn * r / (float)n);
        }
        if (dout) dout[i] = g;
        sx += x0;
        ssign += (x0 > 0.f ? 1.f : 0.f) - (x0 < 0.f ? 1.f : 0.f);
        act += 1.f + x > 0.f ? 1.f : 0.f;
        bad += (__float_as_uint(x0) & 0x7f800000u) == 0x7f800000u ? 1.f : 0.f;      // exponent all ones: inf / NaN
    }
    a = block_sum(a, sh);
    if (want_mean) sx = block_sum(sx, sh);
    if (lecam > 0.f) pen = block_sum(pen, sh);
    if (want_stats) {
        ssign = block_sum(ssign, sh);
        act = block_sum(act, sh);
        bad = block_sum(bad, sh);
        if (keep > 0) nkept = block_sum(nkept, sh);
    }
    if (threadIdx.x != 0) return;
    const float adv = a / div, mean = sx / (float)n;
    *loss += adv;
    if (a_next) {
        float v = (1.f - decay) * mean;
        if (decay != 0.f) v += decay * *a_prev;
        *a_next = v;
    }
    if (want_stats) {
        stats[DVD_ADV_STAT_MEAN] = mean;
        stats[DVD_ADV_STAT_SIGN] = ssign / (float)n;
        stats[DVD_ADV_STAT_ACTIVE] = act / (float)n;
        stats[DVD_ADV_STAT_ADV] = adv;
        stats[DVD_ADV_STAT_LECAM] = pen / (float)n;
        stats[DVD_ADV_STAT_ANCHOR] = anchor;
        stats[DVD_ADV_STAT_KEPT] = keep > 0 ? nkept : (float)(n / group);
        stats[DVD_ADV_STAT_NONFINITE] = bad;
    }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int dvd_adv_loss_ex(const float* out, long long n, int group, int hinge, int real_flag, int keep, float lecam,
                               const float* anchor_other, const float* anchor_prev, float* anchor_next, float decay,
                               float* loss, float* dout, float grad_scale, float* stats, void* stream) {
    if (!out || !loss || n <= 0 || group <= 0 || n % group != 0 || keep < 0 || keep > n / group) return DVD_E_ARG;
    if (!(lecam >= 0.f) || (lecam > 0.f && !anchor_other)) return DVD_E_ARG;
    if (anchor_next && (!decay_ok(decay) || (decay != 0.f && !anchor_prev))) return DVD_E_ARG;
    if (keep > 0 && n / group > DVD_ADV_MAX_SAMPLES) return DVD_E_SHAPE;
    adv_loss_ex_kernel<<<1, 1024, 0, S_>>>(out, n, group, hinge, real_flag, keep, lecam, anchor_other, anchor_prev, anchor_next,
                                           decay, loss, dout, grad_scale, stats);
    return launch_status();
}
