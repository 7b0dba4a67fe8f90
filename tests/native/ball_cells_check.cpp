// ball_cells (livo_internal.h) against a literal restatement of the cell range
// the searches computed inline before it existed (grid_search's range_of):
// random (q, t, org, h, eps) and the edge cases.  Integer outputs must be equal.
//
// t = +inf and NaN: the callers test `t < INFINITY` before they call, and the
// helper rejects both as well (the radius is +inf / NaN, so no index passes
// the limit test); the check below asserts the helper's side.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "livo_internal.h"

using namespace livo;

static bool range_ref(const float org[3], float h, float eps, float qx, float qy, float qz, float t, int lo[3],
                      int hi[3]) {
    const double rad = sqrt((double)t + 1e-9) * (1.0 + 1e-5) + (double)eps;
    const double ih = 1.0 / (double)h;
    const double lim = (double)(kGridBias - 8);
    const double l0 = floor(((double)qx - rad - (double)org[0]) * ih), h0 = floor(((double)qx + rad - (double)org[0]) * ih);
    const double l1 = floor(((double)qy - rad - (double)org[1]) * ih), h1 = floor(((double)qy + rad - (double)org[1]) * ih);
    const double l2 = floor(((double)qz - rad - (double)org[2]) * ih), h2 = floor(((double)qz + rad - (double)org[2]) * ih);
    if (!(fmax(fmax(fabs(l0), fabs(h0)), fmax(fmax(fabs(l1), fabs(h1)), fmax(fabs(l2), fabs(h2)))) < lim)) return false;
    lo[0] = (int)l0; hi[0] = (int)h0;
    lo[1] = (int)l1; hi[1] = (int)h1;
    lo[2] = (int)l2; hi[2] = (int)h2;
    return true;
}

static long g_bad = 0, g_cases = 0, g_rejected = 0;

static void check(const float org[3], float h, float eps, float qx, float qy, float qz, float t, int expect = -1) {
    int lo[3], hi[3], rlo[3], rhi[3];
    const bool ok = ball_cells(org, h, eps, qx, qy, qz, t, lo, hi);
    const bool rok = range_ref(org, h, eps, qx, qy, qz, t, rlo, rhi);
    bool same = ok == rok;
    if (ok && rok)
        for (int a = 0; a < 3; a++) same = same && lo[a] == rlo[a] && hi[a] == rhi[a];
    if (expect >= 0) same = same && (int)ok == expect;
    g_cases++;
    g_rejected += !ok;
    if (!same) {
        g_bad++;
        if (g_bad <= 10) std::printf("mismatch: q=(%g %g %g) t=%g org=(%g %g %g) h=%g eps=%g\n", qx, qy, qz, t, org[0], org[1], org[2], h, eps);
    }
}

int main(int argc, char** argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 5000;
    std::mt19937_64 rng(9);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    for (long i = 0; i < n; i++) {
        const float org[3] = {100.f * U(rng), 100.f * U(rng), 20.f * U(rng)};
        const float h = 0.05f + 2.f * std::fabs(U(rng));
        const float eps = 1e-4f * std::fabs(U(rng));
        const float ext = (i % 7 == 0) ? 3e6f : 300.f;  // (every 7th: far enough to pass the index limit)
        const float t = (i % 5 == 0) ? 25.f * std::fabs(U(rng)) : 0.2f * std::fabs(U(rng));
        check(org, h, eps, org[0] + ext * U(rng), org[1] + ext * U(rng), org[2] + ext * U(rng), t);
    }
    const float o[3] = {-12.5f, 3.25f, 0.f};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    check(o, 0.5f, 1e-5f, 1.f, 2.f, 3.f, 0.f, 1);     // t = 0: the radius is the margins alone
    check(o, 0.5f, 0.f, 1.f, 2.f, 3.f, 0.f, 1);
    check(o, 0.5f, 1e-5f, 1.f, 2.f, 3.f, inf, 0);     // rejected by the helper (and by the callers before it)
    check(o, 0.5f, 1e-5f, 1.f, 2.f, 3.f, nan, 0);
    {   // a NaN query coordinate: rejected.  (The inline range_of let it through -- fmax drops a NaN --
        // into an undefined double -> int conversion; the other inline copies rejected it as the helper does.)
        int lo[3], hi[3];
        g_cases++;
        if (ball_cells(o, 0.5f, 1e-5f, nan, 2.f, 3.f, 0.1f, lo, hi)) g_bad++;
    }
    for (int c = -3; c <= 3; c++) {                   // queries exactly on a cell face
        check(o, 0.5f, 1e-5f, o[0] + 0.5f * (float)c, o[1] + 0.5f * (float)c, o[2] + 0.5f * (float)c, 0.04f, 1);
        check(o, 0.5f, 0.f, o[0] + 0.5f * (float)c, o[1], o[2] - 0.5f * (float)c, 0.f, 1);
    }
    // ranges touching the +- index limit kGridBias - 8 (h = 1, org = 0, integer-valued queries)
    const float z[3] = {0.f, 0.f, 0.f};
    const float L = (float)(kGridBias - 8);
    for (int d = -3; d <= 3; d++)
        for (float rad2 : {0.f, 0.25f, 1.f, 4.f}) {
            check(z, 1.f, 0.f, L + (float)d + 0.5f, 0.f, 0.f, rad2);
            check(z, 1.f, 0.f, 0.f, -L + (float)d + 0.5f, 0.f, rad2);
            check(z, 1.f, 0.f, 0.f, 0.f, L + (float)d, rad2);
        }
    check(z, 1.f, 0.f, L - 1.5f, 0.f, 0.f, 0.f, 1);  // last cell inside the limit
    check(z, 1.f, 0.f, L + 0.5f, 0.f, 0.f, 0.f, 0);  // first cell outside it
    std::printf("%ld cases (%ld rejected), %ld mismatches\n", g_cases, g_rejected, g_bad);
    return g_bad ? 1 : 0;
}
