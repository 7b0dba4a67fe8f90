// rgb_kernels.hip — CDNA4 (gfx950) kernels of the coloured world cloud:
// LaserMapping::publish_frame_world_rgb, src/laser_mapping.cpp:1351-1381.
//
//   k_rgb_points   one cloud point per thread, in the cloud's order: the world
//                  point exactly as k_to_world stores it (cloud_world_point,
//                  device_common.h), then rgb_point (cam_model.h): camera
//                  frame, p_cam.z > 0, pinhole projection, isInFrame, getpixel.
//                  Stores the 16-B record and the keep flag, the block's kept
//                  count, and adds the block's drop / edge / kept counts
//                  (block_tally) to the call's counters (integer adds: the
//                  sums do not depend on their order).
//   k_rgb_scatter  behind an exclusive scan of the blocks' counts: a kept
//                  point's place is its block's offset + the kept points of
//                  the waves before its own + those of the lanes before it
//                  (64-bit ballot, popcount below the lane), so the output is
//                  in the cloud's order, as the reference's push_back inside a
//                  sequential for_each leaves it, and the same on every run.
// The image (3.9 MB at 1280 x 1024) stays cache-resident; both source orders
// are spatially coherent, so neighbouring lanes read neighbouring pixels.
// Numerics as livo_kernels.hip: -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "livo_internal.h"

namespace livo {

static_assert(sizeof(livo_rgb_point) == 16, "one 16-B store per record");
static_assert(kRgbBlock % 64 == 0 && kRgbBlock <= 1024, "whole waves");
constexpr int kRgbWaves = kRgbBlock / 64;

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

__global__ __launch_bounds__(kRgbBlock) void k_rgb_points(RgbParams P) {
    const int i = blockIdx.x * kRgbBlock + threadIdx.x;
    int fate = -1;  // (no point)
    bool edge = false;
    if (i < (int)P.cloud.n) {
        float wx, wy, wz;
        cloud_world_point(P.cloud, P.W, i, wx, wy, wz);
        uint32_t rgba;
        fate = rgb_point(P.cam, P.img, wx, wy, wz, rgba, edge);
        if (fate == kRgbKept)
            reinterpret_cast<float4*>(P.rec)[i] = make_float4(wx, wy, wz, __uint_as_float(rgba));
        P.keep[i] = fate == kRgbKept ? 1 : 0;
    }
    static_assert(kRgbCtrBehind == 0 && kRgbCtrOutOfFrame == 1 && kRgbCtrEdge == 2 && kRgbCtrKept == 3, "the order");
    const bool pred[kRgbCtrN] = {fate == kRgbBehind, fate == kRgbOutOfFrame, edge, fate == kRgbKept};
    const uint32_t v = block_tally<kRgbWaves>(pred);
    if (threadIdx.x < kRgbCtrN) {
        if (threadIdx.x == kRgbCtrKept) P.blk_cnt[blockIdx.x] = v;
        if (v) atomicAdd(P.ctr + threadIdx.x, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kRgbBlock) void k_rgb_scatter(RgbParams P) {
    const int i = blockIdx.x * kRgbBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool kept = i < (int)P.cloud.n && P.keep[i] != 0;
    __shared__ uint32_t wcnt[kRgbWaves];
    const unsigned long long mk = __ballot(kept);
    if (lane == 0) wcnt[w] = (uint32_t)__popcll(mk);
    __syncthreads();
    if (!kept) return;
    uint32_t pos = P.blk_off[blockIdx.x] + (uint32_t)lanes_below(mk);
    for (int ww = 0; ww < w; ww++) pos += wcnt[ww];
    if (P.out) reinterpret_cast<float4*>(P.out)[pos] = reinterpret_cast<const float4*>(P.rec)[i];
    if (P.src_index) P.src_index[pos] = i;
}

static inline unsigned rgb_blocks(int64_t n) { return (unsigned)((n + kRgbBlock - 1) / kRgbBlock); }

int launch_rgb_points(const RgbParams& p, void* stream) {
    if (p.cloud.n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_rgb_points, dim3(rgb_blocks(p.cloud.n)), dim3(kRgbBlock), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_rgb_scatter(const RgbParams& p, void* stream) {
    if (p.cloud.n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_rgb_scatter, dim3(rgb_blocks(p.cloud.n)), dim3(kRgbBlock), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

}  // namespace livo
