/*
 * dvdgan_hip_adv.h -- C ABI of libdvdgan_hip_adv.so: the adversarial loss launch of the DVD-GAN training step with the
 * stabilisers that work on the discriminators' logits alone.  A library of its own beside libdvdgan_hip.so
 * (dvdgan_hip.h, whose set of entry points is fixed): same conventions -- plain C, device pointers + sizes, asynchronous on
 * `stream` (a hipStream_t passed as void*), never synchronises, return value 0 = ok, < 0 = DVD_E_ARG (-1) / DVD_E_SHAPE (-2) /
 * DVD_E_LAUNCH of dvdgan_hip.h.  No process-wide state.
 */
#ifndef DVDGAN_HIP_ADV_H
#define DVDGAN_HIP_ADV_H
#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations of this header are exported */
#pragma GCC visibility push(default)

/* Trainer.calc_loss (trainer.py:114-121) with the stabilisers that work on the logits alone (no reference counterpart;
 * functional.AdvLossEx).  One launch of one workgroup, no atomics: every sum is a strided
 * per-thread sum followed by the workgroup reduction, so the results are a function of the inputs alone.  x_i = out[i]; `out` is
 * sample-major: sample b owns x[b * group, (b + 1) * group).
 *
 * Selection (keep > 0; top-k generator updates).  The score of a sample is the fp32 mean of its `group` logits, summed in index
 * order.  Sample b is kept when fewer than `keep` samples c have score_c > score_b, or score_c == score_b with c < b: ties go to
 * the lower index, and a NaN score compares false everywhere, so it ranks first and is kept (it reaches the statistics and the
 * gradient guard).  The adversarial mean and its gradient then run over the kept logits only, divisor keep * group; dropped
 * logits get dout = 0.  At most DVD_ADV_MAX_SAMPLES samples (the scores live in LDS); without selection any n is served.
 *
 * Adversarial term: dvd_adv_loss's arithmetic, *loss += it.  With keep = 0, lecam = 0 the results are dvd_adv_loss's bit for bit.
 *
 * LeCam term (lecam > 0; Tseng et al. 2021, the relu'd form), a = *anchor_other, over all n logits:
 *   real_flag: P = mean relu(x_i - a)^2,  else: P = mean relu(a - x_i)^2;   dout[i] += grad_scale * lecam * dP/dx_i.
 * P is reported in stats only: *loss stays the adversarial term (like the orthogonal penalty, only the gradient enters).
 *
 * Anchor (anchor_next != NULL, whatever lecam is): *anchor_next = decay * *anchor_prev + (1 - decay) * mean_i x_i over all n
 * logits; decay in [0, 1), and decay == 0 does not read *anchor_prev.  The three anchor pointers name distinct floats.
 *
 * stats (may be NULL): DVD_ADV_NSTAT floats, overwritten, indexed by DVD_ADV_STAT_*.  MEAN, SIGN (mean of sign(x_i): the
 * overfitting indicator r_t on a real call), ACTIVE (fraction with 1 + sgn * x_i > 0, the hinge's active side) and NONFINITE (a
 * count) run over all n logits; ADV is the adversarial term, LECAM is P, ANCHOR is *anchor_other (0 when NULL), KEPT the number
 * of samples kept (n / group without selection).
 * DVD_E_ARG: n % group != 0, keep < 0, keep > n / group, lecam < 0, lecam > 0 without anchor_other, anchor_next with a decay
 * outside [0, 1) or with decay > 0 and no anchor_prev.  DVD_E_SHAPE: keep > 0 and n / group > DVD_ADV_MAX_SAMPLES. */
#define DVD_ADV_MAX_SAMPLES 4096
#define DVD_ADV_NSTAT 8
#define DVD_ADV_STAT_MEAN 0
#define DVD_ADV_STAT_SIGN 1
#define DVD_ADV_STAT_ACTIVE 2
#define DVD_ADV_STAT_ADV 3
#define DVD_ADV_STAT_LECAM 4
#define DVD_ADV_STAT_ANCHOR 5
#define DVD_ADV_STAT_KEPT 6
#define DVD_ADV_STAT_NONFINITE 7
int dvd_adv_loss_ex(const float* out, long long n, int group, int hinge, int real_flag, int keep, float lecam,
                    const float* anchor_other, const float* anchor_prev, float* anchor_next, float decay, float* loss,
                    float* dout, float grad_scale, float* stats, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
