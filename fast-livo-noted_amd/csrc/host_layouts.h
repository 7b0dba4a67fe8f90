// host_layouts.h — the scratch layouts of livo_capi.cpp whose arrays hold plain
// integers and floats, each a function of a Carve (carve.h): run over a null
// base it sizes the buffer, run over the buffer it yields the pointers.  Every
// array starts on its own 256-byte boundary: no array is found from another by
// offset.  No HIP here: tests/native/carve_check.cpp runs them on the host.
#pragma once
#include <stdint.h>

#include "carve.h"

namespace livo {

// The sizing pass of one of the layouts below: its byte total for these arguments.
template <class L, class... A>
inline size_t carve_bytes(L (*layout)(Carve&, A...), A... a) {
    Carve k{nullptr};
    layout(k, a...);
    return k.total();
}

// The run builds' sort and scan arrays for n entries (build_cell_runs_into;
// ball: build_ball_runs_idx, which also carries each entry's grid position and
// gathers the anchor keys).  runid, plen and pstart reuse arrays that are dead
// by the time they are written (rho, srho: after the first sort; iota: after
// the sorts), except where the ball build still needs them.
struct RunBuild {
    uint32_t *rho, *iota, *srho, *e1, *e2, *heads, *starts;
    uint32_t* pt;                     // ball only
    unsigned long long *keys, *skeys;
    unsigned long long* key1;         // ball only
    unsigned long long* nruns;
    uint32_t *runid, *plen, *pstart;  // aliases (cell: runid is an array of its own)
};
inline RunBuild run_build_layout(Carve& k, size_t n, bool ball) {
    RunBuild L{};
    L.rho = k.take<uint32_t>(n);
    L.iota = k.take<uint32_t>(n);
    L.srho = k.take<uint32_t>(n);
    L.e1 = k.take<uint32_t>(n);
    L.e2 = k.take<uint32_t>(n);
    L.heads = k.take<uint32_t>(n);
    L.starts = k.take<uint32_t>(n + 1);
    L.keys = k.take<unsigned long long>(n);
    L.skeys = k.take<unsigned long long>(n);
    L.nruns = k.take<unsigned long long>(1);
    if (ball) {
        L.pt = k.take<uint32_t>(n);
        L.key1 = k.take<unsigned long long>(n);
        L.runid = L.rho;
        L.plen = k.take<uint32_t>(n + 1);
        L.pstart = L.srho;
    } else {
        L.runid = k.take<uint32_t>(n);
        L.plen = L.rho;
        L.pstart = L.iota;
    }
    return L;
}

// A scan build's Morton keys, their sorted copy, iota, the sorted values and
// `bound_words` bound words (6 per scan: scan_build_on 6, the batched upload
// 6 * kFeSegMax) for n points.
struct ScanBuild {
    uint32_t *keys, *skeys, *iota, *svals;
    unsigned* bounds;
};
inline ScanBuild scan_build_layout(Carve& k, size_t n, size_t bound_words) {
    ScanBuild L{};
    L.keys = k.take<uint32_t>(n);
    L.skeys = k.take<uint32_t>(n);
    L.iota = k.take<uint32_t>(n);
    L.svals = k.take<uint32_t>(n);
    L.bounds = k.take<unsigned>(bound_words);
    return L;
}

// The single-scan uploads' scratch: the build's arrays (6 bound words), then (src:
// livo_scan_upload, livo_scan_upload_async) the packed source points x, y, z.
struct ScanUpload {
    ScanBuild build;
    float* src;
};
inline ScanUpload scan_upload_layout(Carve& k, size_t n, bool src) {
    ScanUpload L{};
    L.build = scan_build_layout(k, n, 6);
    if (src) L.src = k.take<float>(n * 3);
    return L;
}

// livo_knn / livo_ivox_knn: n queries (x, y, z, 0) and their neighbour records.
template <class Rec>
struct KnnQuery {
    float* q;
    Rec* rec;
};
template <class Rec>
inline KnnQuery<Rec> knn_query_layout(Carve& k, size_t n) {
    KnnQuery<Rec> L{};
    L.q = k.take<float>(n * 4);
    L.rec = k.take<Rec>(n);
    return L;
}

// ensure_nn_records: the plane cache and plane states of a scan of n points.
struct PlaneTmp {
    float* plane;
    uint8_t* pstate;
};
inline PlaneTmp plane_tmp_layout(Carve& k, size_t n) {
    PlaneTmp L{};
    L.plane = k.take<float>(n * 4);
    L.pstate = k.take<uint8_t>(n);
    return L;
}

// livo_h_share's per-point outputs for n points and (ori) the laserCloudOri
// compaction: flags, their scan, the effective points and their normals.
struct HShareDbg {
    float *normvec, *world;
    uint8_t* sel;
    uint32_t *flags, *pos;  // ori only
    float *ori, *corr;      // ori only
};
inline HShareDbg hshare_dbg_layout(Carve& k, size_t n, bool ori) {
    HShareDbg L{};
    L.normvec = k.take<float>(n * 4);
    L.world = k.take<float>(n * 3);
    L.sel = k.take<uint8_t>(n);
    if (ori) {
        L.flags = k.take<uint32_t>(n);
        L.pos = k.take<uint32_t>(n);
        L.ori = k.take<float>(n * 3);
        L.corr = k.take<float>(n * 4);
    }
    return L;
}

// livo_map_incremental (iVox): the 2n candidate points in order (add, then
// no-need-down), their flags and scan, and the n categories.
struct MapIncr {
    float* ordered;
    uint32_t *flags, *pos;
    uint8_t* cat;
};
inline MapIncr map_incr_layout(Carve& k, size_t n) {
    MapIncr L{};
    L.ordered = k.take<float>(2 * n * 4);
    L.flags = k.take<uint32_t>(2 * n);
    L.pos = k.take<uint32_t>(2 * n);
    L.cat = k.take<uint8_t>(n);
    return L;
}

}  // namespace livo
