// upload_plan.h — the arithmetic of the scan uploads in livo_capi.cpp that needs
// no device: how a batch of scans splits into build passes (UploadPass), and
// the one list of a scan's device arrays with their element counts
// (scan_arrays), by which the scan buffers are allocated, freed and budgeted.
// No HIP here: tests/native/upload_plan_check.cpp runs it on the host (of
// livo_internal.h it uses constants and NNRec only; a host program declares the
// one HIP type that header names, uint4, before including this).
#pragma once
#include <stdint.h>

#include "livo_internal.h"

namespace livo {

// One build pass of livo_scan_upload_batch_async: scans [b0, b0 + m) of the
// batch, m <= kFeSegMax, packed back to back.
struct UploadPass {
    int32_t m;                // scans in the pass
    int64_t tot, max_n;       // their points in all, and the largest scan's
    int64_t off[kFeSegMax];   // first point of scan b0 + b in the packed pass
    int key_bits;             // of the pass's sort: 27 Morton bits + the scan index's
};
// The pass that starts at scan b0 of the n sizes N[].  LIVO_E_RANGE: more points
// than the batch sort's 32-bit positions hold.
inline int upload_pass(const int64_t* N, int32_t n, int32_t b0, UploadPass* P) {
    *P = UploadPass{};
    P->m = n - b0 < kFeSegMax ? n - b0 : kFeSegMax;
    for (int32_t b = 0; b < P->m; b++) {
        P->off[b] = P->tot;
        P->tot += N[b0 + b];
        if (N[b0 + b] > P->max_n) P->max_n = N[b0 + b];
    }
    P->key_bits = 27;
    while ((1 << (P->key_bits - 27)) < P->m) P->key_bits++;
    return P->tot > (int64_t)0xFFFFFFFF - kBlock ? LIVO_E_RANGE : LIVO_OK;
}

// Blocks of the per-point kernels over n points (at least one).
inline int64_t scan_blocks(int64_t n) {
    const int64_t b = (n + kBlock * kPtsPerThread - 1) / (kBlock * kPtsPerThread);
    return b < 1 ? 1 : b;
}
// Doubles of a scan's block partials: the larger of the IKFoM blocks' and the
// fused evaluation's.
inline size_t partial_doubles(int64_t N) {
    const int64_t a = scan_blocks(N) * kIkCols;
    const int64_t e = (N + kEvalBlock - 1) / kEvalBlock;
    const int64_t b = (e < 1 ? 1 : e) * kRedCols;
    return (size_t)(a > b ? a : b);
}

// A scan's device arrays, each an allocation of its own.
struct ScanArrays {
    float* pts = nullptr;        // n x 4
    NNRec* nn = nullptr;         // neighbour records (Nearest_Points cache)
    double* partial = nullptr;   // nblk x kIkCols (the A-path uses kRedCols of each)
    int32_t* d_perm = nullptr;   // stored (Morton) position -> caller's point index
    int32_t* d_iperm = nullptr;  // caller's point index -> stored position
    float* plane = nullptr;      // N x 4: planes of the cached neighbours (k_hshare)
    uint8_t* pstate = nullptr;   // N: plane state (0: not fitted since the neighbours changed)
    double* ikrows = nullptr;    // IKFoM few-point rows (nblk x kIkFewRows x 13)
    uint32_t* ikcnt = nullptr;   // per block
};
// f(array, elements) for each of them, sized for cap points: the only list.
template <class F>
inline void scan_arrays(ScanArrays& s, int64_t cap, F&& f) {
    const size_t n = (size_t)cap, blk = (size_t)scan_blocks(cap);
    f(s.pts, n * 4);
    f(s.nn, n);
    f(s.partial, partial_doubles(cap));
    f(s.d_perm, n);
    f(s.d_iperm, n);
    f(s.plane, n * 4);
    f(s.pstate, n);
    f(s.ikrows, blk * kIkFewRows * 13);
    f(s.ikcnt, blk);
}
// Their bytes in all (the spare pool's budget counts a released scan by this).
inline size_t scan_buf_bytes(int64_t cap) {
    ScanArrays s;
    size_t bytes = 0;
    scan_arrays(s, cap, [&](auto*& p, size_t count) { bytes += count * sizeof(*p); });
    return bytes;
}

}  // namespace livo
