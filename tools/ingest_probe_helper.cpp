// ingest_probe_helper.cpp — what a caller ran on the host before livo_frame_ingest_livox: a plain
// single-thread restatement of avia_handler (preprocess.cpp:315-349) and sync_packages' std::sort
// (laser_mapping.cpp:705).  Built by tools/ingest_probe.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "livo.h"

extern "C" int64_t avia_sort_host(const livo_livox_point* msg, int64_t n, int32_t n_scans, int32_t filter_num,
                                  double blind, livo_raw_point* out) {
    std::vector<livo_raw_point> pl;
    pl.reserve((size_t)n);
    unsigned effect_ind = 0;
    for (int64_t i = 1; i < n; i++) {
        const livo_livox_point &a = msg[i], &b = msg[i - 1];
        const double range = a.x * a.x + a.y * a.y;
        if (std::abs(a.x - b.x) < 1e-8 || std::abs(a.y - b.y) < 1e-8 || std::abs(a.z - b.z) < 1e-8 || range < blind ||
            range > 900 || a.line > n_scans || (a.tag & 0x30) != 0x10)
            continue;
        effect_ind++;
        if (effect_ind % filter_num == 0)
            pl.push_back({a.x, a.y, a.z, std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z), a.offset_time / float(1000000)});
    }
    std::sort(pl.begin(), pl.end(),
              [](const livo_raw_point& x, const livo_raw_point& y) { return x.curvature < y.curvature; });
    std::copy(pl.begin(), pl.end(), out);
    return (int64_t)pl.size();
}
