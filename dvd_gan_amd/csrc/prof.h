// Optional per-launch HIP-event profiling of the convolution kernels (bench.py; see dvd_prof_enable in include/dvdgan_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <mutex>

// ProfRec::variant of a forward / backward-data launch (kind 0) = its slot in dvd_prof_report_variants (0: every launch); bench.py,
// tools/ and the tests read the numbers.  HALO: halo-staged kernels, weights through LDS or from L2; TAP: tap-by-tap kernel; FRAME:
// whole 4 x 4 / 8 x 8 frames on 256- / 128-row tiles; THIN: conv_thin.hip; GROUP: grouped launches of the HALO / FRAME kernels.
enum ConvVariant {
    CV_VAR_ALL = 0, CV_VAR_HALO_256x128 = 1, CV_VAR_HALO_128x128 = 2, CV_VAR_HALO_256x64 = 3, CV_VAR_TAP_128x128 = 4,
    CV_VAR_TAP_256x128 = 5, CV_VAR_TAP_256x256 = 6, CV_VAR_FRAME_256 = 7, CV_VAR_FRAME_128 = 8, CV_VAR_THIN = 9,
    CV_VAR_GROUP_HALO = 10, CV_VAR_GROUP_FRAME = 11,
};

namespace dvdprof {
struct ProfRec { hipEvent_t a, b; double flops; int kind; long long M; int C, Cout, taps, split, flags, variant; };
extern bool g_prof;
extern std::vector<ProfRec> g_recs;
extern std::mutex g_prof_mu;
struct ProfScope {
    ProfRec r; bool on; hipStream_t s;
    ProfScope(int kind, double flops, void* stream, long long M, int C, int Cout, int taps, int split, int flags)
        : on(g_prof), s((hipStream_t)stream) {
        if (!on) return;
        r.kind = kind; r.flops = flops; r.M = M; r.C = C; r.Cout = Cout; r.taps = taps; r.split = split; r.flags = flags;
        r.variant = 0;
        hipEventCreate(&r.a); hipEventCreate(&r.b);
        hipEventRecord(r.a, s);
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(r.b, s);
        std::lock_guard<std::mutex> l(g_prof_mu);
        g_recs.push_back(r);
    }
};
}  // namespace dvdprof
using dvdprof::ProfScope;
