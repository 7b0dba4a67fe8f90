// vis_kernels.hip — CDNA4 (gfx950) kernels of a frame's new visual map points:
// LidarSelector::addSparseMap, src/lidar_selection.cpp:140-193, with getpatch
// (:117-138) and AddPoint's voxel key (:195-208).
//
//   k_vis_score  one cloud point per thread, in the cloud's order: the world
//                point exactly as k_to_world stores it (cloud_world_point,
//                device_common.h), then vis_project and vis_score
//                (cam_model.h): w2c, the frame test,
//                the grid index, shiTomasiScore over the 10 x 10 byte window
//                (aligned 4-byte loads, a row at a time).  A point of positive
//                score bids for its cell with one 64-bit atomicMax of
//                score bits << 32 | ~cloud index: positive floats order as
//                their bits, the complemented index lets the lowest one win
//                among equal scores, so the table is what the reference's
//                sequential `cur_value > map_value[index]` leaves, whatever
//                the order of execution.  The call's counters take one integer
//                add per block and counter (block_tally).
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

__global__ __launch_bounds__(kVisBlock) void k_vis_score(VisParams P) {
    const int i = blockIdx.x * kVisBlock + threadIdx.x;
    int fate = kVisOutOfFrame;
    bool behind = false;
    if (i < (int)P.cloud.n) {
        float wx, wy, wz;
        cloud_world_point(P.cloud, P.W, i, wx, wy, wz);
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
    static_assert(kVisCtrInFrame == 0 && kVisCtrBehind == 1 && kVisCtrOverflow == 2 && kVisCtrOut == 3, "the order");
    const bool pred[kVisCtrOut] = {fate != kVisOutOfFrame, behind, fate == kVisOverflow};
    const uint32_t v = block_tally<kVisWaves>(pred);
    if (threadIdx.x < kVisCtrOut && v) atomicAdd(P.ctr + threadIdx.x, (unsigned long long)v);
}

__global__ __launch_bounds__(kVisBlock) void k_vis_flags(VisParams P) {
    const int c = blockIdx.x * kVisBlock + threadIdx.x;
    const bool occ = c < P.grid.length && P.table[c] != 0ull;
    if (c < P.grid.length) P.flag[c] = occ ? 1u : 0u;
    const bool pred[1] = {occ};
    const uint32_t v = block_tally<kVisWaves>(pred);
    if (threadIdx.x == 0 && v) atomicAdd(P.ctr + kVisCtrOut, (unsigned long long)v);
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
    cloud_world_point(P.cloud, P.W, i, wx, wy, wz);
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
    if (p.cloud.n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_vis_score, dim3(vis_blocks(p.cloud.n, kVisBlock)), dim3(kVisBlock), 0, (hipStream_t)stream, p);
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
