// vis_kernels.hip — CDNA4 (gfx950) kernels of a frame's new visual map points:
// LidarSelector::addSparseMap, src/lidar_selection.cpp:140-193, with getpatch
// (:117-138) and AddPoint's voxel key (:195-208).
//
//   k_vis_score  one cloud point per thread, in the cloud's order: the world
//                point exactly as k_to_world stores it (world_point), then
//                vis_project and vis_score (cam_model.h): w2c, the frame test,
//                the grid index, shiTomasiScore over the 10 x 10 byte window
//                (aligned 4-byte loads, a row at a time).  A point of positive
//                score bids for its cell with one 64-bit atomicMax of
//                score bits << 32 | ~cloud index: positive floats order as
//                their bits, the complemented index lets the lowest one win
//                among equal scores, so the table is what the reference's
//                sequential `cur_value > map_value[index]` leaves, whatever
//                the order of execution.  The call's counters take one integer
//                add per block and counter (wave ballots first).
//   k_vis_flags  one cell per thread: 1 where the cell has a winner, and their
//                count.
//   k_vis_emit   behind an exclusive scan of the flags: one wave per occupied
//                cell recomputes its winner's world point and pixel (the same
//                functions, so the same bits), lane 0 stores the 64-B record,
//                and the 3 * ps^2 patch values go one per lane (coalesced).
// No position is decided by an atomic: two calls give the same bytes.
// The image (1.3 MB at 1280 x 1024) stays cache-resident.  Numerics as
// livo_kernels.hip: -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "livo_internal.h"

namespace livo {

static_assert(sizeof(livo_vis_point) == 64, "one 64-B record");
static_assert(kVisBlock % 64 == 0 && kVisBlock <= 1024, "whole waves");
constexpr int kVisWaves = kVisBlock / 64;

__device__ __forceinline__ void vis_world(const VisParams& P, int i, float& wx, float& wy, float& wz) {
    const int64_t k = P.iperm ? (int64_t)P.iperm[i] : (int64_t)i;
    const float* p = P.src + P.stride * k;
    world_point(P.W.rot, P.W.pos, P.W.R_LI, P.W.t_LI, p[0], p[1], p[2], wx, wy, wz);
}

__global__ __launch_bounds__(kVisBlock) void k_vis_score(VisParams P) {
    const int i = blockIdx.x * kVisBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int fate = kVisOutOfFrame;
    bool behind = false;
    if (i < P.n) {
        float wx, wy, wz;
        vis_world(P, i, wx, wy, wz);
        double pc[2];
        int index;
        fate = vis_project(P.cam, P.grid, wx, wy, wz, pc, behind, index);
        if (fate == kVisInFrame) {  // (0 <= index < length)
            const float score = vis_score(P.img, P.cam.w, P.cam.h, (int)pc[0], (int)pc[1]);
            if (score > 0.0f) {  // (false for a NaN: it never exceeds map_value)
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
                // the table only grows: a bid below what was already read cannot win
                if (key > P.table[index]) atomicMax(P.table + index, key);
            }
        }
    }
    __shared__ uint32_t cnt[kVisWaves][kVisCtrOut];
    const unsigned long long mi = __ballot(fate != kVisOutOfFrame), mb = __ballot(behind),
                             mo = __ballot(fate == kVisOverflow);
    if (lane == 0) {
        cnt[w][kVisCtrInFrame] = (uint32_t)__popcll(mi);
        cnt[w][kVisCtrBehind] = (uint32_t)__popcll(mb);
        cnt[w][kVisCtrOverflow] = (uint32_t)__popcll(mo);
    }
    __syncthreads();
    if (threadIdx.x < kVisCtrOut) {
        uint32_t v = 0;
        for (int ww = 0; ww < kVisWaves; ww++) v += cnt[ww][threadIdx.x];
        if (v) atomicAdd(P.ctr + threadIdx.x, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kVisBlock) void k_vis_flags(VisParams P) {
    const int c = blockIdx.x * kVisBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool occ = c < P.grid.length && P.table[c] != 0ull;
    if (c < P.grid.length) P.flag[c] = occ ? 1u : 0u;
    __shared__ uint32_t cnt[kVisWaves];
    const unsigned long long m = __ballot(occ);
    if (lane == 0) cnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t v = 0;
        for (int ww = 0; ww < kVisWaves; ww++) v += cnt[ww];
        if (v) atomicAdd(P.ctr + kVisCtrOut, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kVisBlock) void k_vis_emit(VisParams P) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * kVisWaves + (threadIdx.x >> 6);  // one wave per cell
    if (c >= P.grid.length) return;
    const unsigned long long key = P.table[c];
    if (key == 0ull) return;
    const int i = (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
    const uint32_t pos = P.slot[c];
    float wx, wy, wz;
    vis_world(P, i, wx, wy, wz);
    double pc[2];
    bool behind;
    int index;
    (void)vis_project(P.cam, P.grid, wx, wy, wz, pc, behind, index);
    if (lane == 0) {
        livo_vis_point r;
        r.x = wx;
        r.y = wy;
        r.z = wz;
        r.score = __uint_as_float((uint32_t)(key >> 32));
        r.u = pc[0];
        r.v = pc[1];
        r.src_index = i;
        r.cell = c;
        r.voxel[0] = vis_voxel_key(wx);
        r.voxel[1] = vis_voxel_key(wy);
        r.voxel[2] = vis_voxel_key(wz);
        P.out[pos] = r;
    }
    const int pst = P.grid.ps * P.grid.ps;
    float* dst = P.patches + (size_t)pos * 3 * pst;
    for (int e = lane; e < 3 * pst; e += 64) {
        const int level = e / pst;
        dst[e] = vis_getpatch(P.img, P.cam.w, pc, P.grid.ps, level, e - level * pst);
    }
}

static inline unsigned vis_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int launch_vis_score(const VisParams& p, void* stream) {
    if (p.n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_vis_score, dim3(vis_blocks(p.n, kVisBlock)), dim3(kVisBlock), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_vis_flags(const VisParams& p, void* stream) {
    if (p.grid.length <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_vis_flags, dim3(vis_blocks(p.grid.length, kVisBlock)), dim3(kVisBlock), 0,
                       (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_vis_emit(const VisParams& p, void* stream) {
    if (p.grid.length <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_vis_emit, dim3(vis_blocks(p.grid.length, kVisWaves)), dim3(kVisBlock), 0,
                       (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

}  // namespace livo
