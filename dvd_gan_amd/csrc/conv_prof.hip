// Optional per-launch profiling of the convolution kernels (prof.h): the record store and the dvd_prof_* entry points.  bench.py
// needs the average duration of the dominant kernel measured with HIP events on the launch stream.  When enabled, every conv launch is
// bracketed by an event pair; dvd_prof_report synchronises and sums them.  Off by default (no events, no global state touched).
#include "common.h"
#include "prof.h"
#include <cstdio>
#include <cstdlib>
namespace dvdprof {
bool g_prof = false;
std::vector<ProfRec> g_recs;
std::mutex g_prof_mu;
}  // namespace dvdprof
using namespace dvdprof;
extern "C" void dvd_prof_enable(int on) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    g_prof = on != 0;
}
// kind 0 = forward / backward-data (ConvVariant, prof.h), 1 = conv_wgrad: 1 = filter-row kernel, 2 = one-tap kernel, 3 = thin-end
// kernel (wgrad_thin.hip), 4 = filter-row kernel, one wave per SIMD.  Drains the records of `kind` and returns the number of
// launches; n / ms / flops (each [nvar] or NULL) receive the per-variant totals; index 0 = everything.
// If the environment variable DVD_PROF_CSV is set, every drained record is appended to that file.
extern "C" long long dvd_prof_report_variants(int kind, int nvar, long long* n, double* ms, double* flops) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    for (int v = 0; v < nvar; ++v) { if (n) n[v] = 0; if (ms) ms[v] = 0; if (flops) flops[v] = 0; }
    long long total = 0;
    std::vector<ProfRec> keep;
    const char* csv = getenv("DVD_PROF_CSV");
    FILE* f = csv ? fopen(csv, "a") : nullptr;
    for (auto& r : g_recs) {
        if (r.kind != kind) { keep.push_back(r); continue; }
        hipEventSynchronize(r.b);
        float t = 0; hipEventElapsedTime(&t, r.a, r.b);
        if (f) fprintf(f, "%d,%lld,%d,%d,%d,%d,%d,%.4f,%.0f,%d\n", r.kind, r.M, r.C, r.Cout, r.taps, r.split, r.flags, t, r.flops, r.variant);
        const int slots[2] = {0, r.variant};                    // slot 0 = all launches, plus the record's own slot
        for (int j = 0; j < (r.variant > 0 ? 2 : 1); ++j) {
            const int v = slots[j];
            if (v >= nvar) continue;
            if (n) ++n[v];
            if (ms) ms[v] += t;
            if (flops) flops[v] += r.flops;
        }
        ++total;
        hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    if (f) fclose(f);
    g_recs.swap(keep);
    return total;
}
extern "C" long long dvd_prof_report(int kind, double* total_ms, double* total_flops) {
    long long n = 0;
    return dvd_prof_report_variants(kind, 1, &n, total_ms, total_flops);
}
