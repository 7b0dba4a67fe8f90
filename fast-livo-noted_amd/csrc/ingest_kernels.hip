// ingest_kernels.hip — CDNA4 (gfx950) kernels of the sensor handlers: the driver's
// message to the time-ordered frame (Preprocess::process with feature_enabled == false,
// preprocess.cpp:315-349, :424-453, :578-637, :650-680; the time sort of sync_packages,
// laser_mapping.cpp:705; the count of UndistortPcl's slice, IMU_Processing.cpp:225-230).
//
//   k_ingest_livox / k_ingest_cloud   one thread per message point.  A block's records
//       (20 B, or point_step B) come through LDS in one coalesced read of whole words; the
//       Avia block also stages the record in front of it, which its duplicate test reads.
//       Every point is decoded as its handler would emit it (dec) and flagged: the handler's
//       survivors (AVIA), or the survivors with i % point_filter_num == 0 (the others).  The
//       survivors are counted per block (one atomic a block).
//   k_ingest_emit   behind the exclusive scan of the flags: with E_i the inclusive count of
//       survivors, an Avia point is kept iff it survives and E_i % p == 0, at slot E_i / p - 1;
//       the others at slot E_i - 1.  Writes the 5-float point, its order-preserving time key
//       and the slot, and reduces the largest key (the frame's end time) per block.
//   k_ingest_gather  the stable sort's permutation applied to the points.
//   k_ingest_take_count  the upper bound of the take limit in the sorted keys, one thread.
//
// Numerics: -ffp-contract=off, correctly rounded sqrt and division; float expressions in
// the reference's order.
#include <hip/hip_runtime.h>
#include <math.h>

#include "livo_internal.h"

namespace livo {

static_assert(sizeof(livo_livox_point) == 20, "livox_ros_driver::CustomPoint");
constexpr int kLivoxW = 5;  // words a record

// float -> u32 whose unsigned order is the float's (-0.0 before +0.0; NaNs at both ends by sign)
__device__ __forceinline__ unsigned time_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float time_of_key(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// common::calc_range (common_lib.h:99-101)
__device__ __forceinline__ float calc_range(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

__device__ __forceinline__ void ingest_store(const IngestParams& P, int64_t i, float x, float y, float z,
                                             float intensity, float curvature, bool flag) {
    float* d = P.dec + 5 * i;
    d[0] = x;
    d[1] = y;
    d[2] = z;
    d[3] = intensity;
    d[4] = curvature;
    P.flags[i] = flag ? 1u : 0u;
}

// every thread of the block calls it: the block's survivors into ctr[kIngCtrPass]
__device__ __forceinline__ void ingest_count(const IngestParams& P, bool pass) {
    const int cnt = __syncthreads_count(pass ? 1 : 0);
    if (threadIdx.x == 0 && cnt > 0) atomicAdd(P.ctr + kIngCtrPass, (unsigned)cnt);
}

// avia_handler (:315-349)
__global__ __launch_bounds__(kIngestBlock) void k_ingest_livox(IngestParams P) {
    __shared__ uint32_t S[(kIngestBlock + 1) * kLivoxW];
    const int64_t base = (int64_t)blockIdx.x * kIngestBlock;
    const int64_t first = base > 0 ? base - 1 : 0;  // with the previous message point
    const int words = (int)(min(base + kIngestBlock, P.n) - first) * kLivoxW;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(P.msg) + first * kLivoxW;
    for (int w = threadIdx.x; w < words; w += kIngestBlock) S[w] = g[w];
    __syncthreads();
    const int64_t i = base + threadIdx.x;
    bool pass = false;
    if (i < P.n) {
        const uint32_t* r = S + (i - first) * kLivoxW;
        const float x = __uint_as_float(r[1]), y = __uint_as_float(r[2]), z = __uint_as_float(r[3]);
        if (i > 0) {  // (the loop starts at 1)
            const float px = __uint_as_float(r[1 - kLivoxW]), py = __uint_as_float(r[2 - kLivoxW]),
                        pz = __uint_as_float(r[3 - kLivoxW]);
            const unsigned tag = (r[4] >> 8) & 0xFFu, line = (r[4] >> 16) & 0xFFu;
            const double range = (double)(x * x + y * y);
            pass = !((double)fabsf(x - px) < 1e-8 || (double)fabsf(y - py) < 1e-8 || (double)fabsf(z - pz) < 1e-8 ||
                     range < P.blind || range > 900.0 || (int)line > P.n_scans || (tag & 0x30u) != 0x10u);
        }
        ingest_store(P, i, x, y, z, calc_range(x, y, z), (float)r[0] / 1000000.f, pass);
    }
    ingest_count(P, pass);
}

// a 32-bit field of a record staged in LDS, at any byte offset
__device__ __forceinline__ uint32_t lds_u32(const unsigned char* s, int at) {
    if ((at & 3) == 0) return *reinterpret_cast<const uint32_t*>(s + at);
    return (uint32_t)s[at] | ((uint32_t)s[at + 1] << 8) | ((uint32_t)s[at + 2] << 16) | ((uint32_t)s[at + 3] << 24);
}

// oust64_handler (:424-453), velodyne_handler with point times (:578-637), xt32_handler (:650-680)
__global__ __launch_bounds__(kIngestBlock) void k_ingest_cloud(IngestParams P) {
    extern __shared__ uint32_t Sd[];
    const int64_t base = (int64_t)blockIdx.x * kIngestBlock;
    const int ps = P.L.point_step;
    // base * ps is a multiple of 256: whole words from an aligned start (the message's buffer is
    // padded past its last record)
    const int words = ((int)min((int64_t)kIngestBlock, P.n - base) * ps + 3) >> 2;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(P.msg + base * ps);
    for (int w = threadIdx.x; w < words; w += kIngestBlock) Sd[w] = g[w];
    __syncthreads();
    const int64_t i = base + threadIdx.x;
    bool pass = false;
    if (i < P.n) {
        const unsigned char* s = reinterpret_cast<const unsigned char*>(Sd);
        const int at = threadIdx.x * ps;
        const float x = __uint_as_float(lds_u32(s, at + P.L.off_x)), y = __uint_as_float(lds_u32(s, at + P.L.off_y)),
                    z = __uint_as_float(lds_u32(s, at + P.L.off_z));
        const float r2 = x * x + y * y + z * z;
        float intensity, curvature;
        if (P.lidar_type == LIVO_LIDAR_OUST64) {
            pass = !((double)r2 < P.blind * P.blind);
            intensity = calc_range(x, y, z);
            curvature = (float)lds_u32(s, at + P.L.off_time) * 1.e-6f;
        } else if (P.lidar_type == LIVO_LIDAR_VELO16) {
            pass = (double)r2 > P.blind * P.blind;
            intensity = __uint_as_float(lds_u32(s, at + P.L.off_intensity));
            curvature = __uint_as_float(lds_u32(s, at + P.L.off_time)) * 1.e-3f;
        } else {
            pass = (double)r2 > P.blind;
            intensity = __uint_as_float(lds_u32(s, at + P.L.off_intensity));
            const unsigned long long tb = (unsigned long long)lds_u32(s, at + P.L.off_time) |
                                          ((unsigned long long)lds_u32(s, at + P.L.off_time + 4) << 32);
            curvature = (float)((__longlong_as_double((long long)tb) - P.time_head) * (double)1000.f);
        }
        ingest_store(P, i, x, y, z, intensity, curvature, pass && i % P.filter_num == 0);
    }
    ingest_count(P, pass);
}

__global__ __launch_bounds__(kIngestBlock) void k_ingest_emit(IngestParams P) {
    __shared__ unsigned red[kIngestBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kIngestBlock + threadIdx.x;
    unsigned key = 0u;
    if (i < P.n) {
        const uint32_t flag = P.flags[i], e = P.pos[i] + 1u;  // e: the inclusive count where flag is set
        if (i == P.n - 1) P.ctr[kIngCtrTotal] = P.pos[i] + flag;
        const bool avia = P.lidar_type == LIVO_LIDAR_AVIA;
        if (flag && (!avia || e % (uint32_t)P.filter_num == 0u)) {
            const int64_t slot = avia ? (int64_t)(e / (uint32_t)P.filter_num) - 1 : (int64_t)e - 1;
            const float* d = P.dec + 5 * i;
            const float v[5] = {d[0], d[1], d[2], d[3], d[4]};
            float* q = P.pts + 5 * slot;
#pragma unroll
            for (int k = 0; k < 5; k++) q[k] = v[k];
            key = time_key(v[4]);
            P.keys[slot] = key;
            P.iota[slot] = (uint32_t)slot;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = red[0];
#pragma unroll
        for (int w = 1; w < kIngestBlock / 64; w++) m = max(m, red[w]);
        if (m > 0u) atomicMax(P.ctr + kIngCtrMaxKey, m);
    }
}

__global__ __launch_bounds__(256) void k_ingest_gather(const float* __restrict__ pts, const uint32_t* __restrict__ perm,
                                                       int64_t n, float* __restrict__ frame) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float* p = pts + 5 * (int64_t)perm[k];
    const float v[5] = {p[0], p[1], p[2], p[3], p[4]};
#pragma unroll
    for (int c = 0; c < 5; c++) frame[5 * k + c] = v[c];
}

// while (it != end && it->curvature <= pcl_offset_time) (IMU_Processing.cpp:225): on times in
// ascending order the first point that fails, by bisection
__global__ void k_ingest_take_count(const uint32_t* __restrict__ skeys, int64_t from, int64_t n, double limit_ms,
                                    unsigned* __restrict__ count) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t lo = from, hi = n;  // [from, lo) taken, [hi, n) not
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((double)time_of_key(skeys[mid]) <= limit_ms)
            lo = mid + 1;
        else
            hi = mid;
    }
    *count = (unsigned)(lo - from);
}

static inline unsigned ingest_blocks(int64_t n) { return (unsigned)((n + kIngestBlock - 1) / kIngestBlock); }

int launch_ingest_decode(const IngestParams& P, void* stream) {
    if (P.n <= 0) return LIVO_OK;
    if (P.lidar_type == LIVO_LIDAR_AVIA) {
        hipLaunchKernelGGL(k_ingest_livox, dim3(ingest_blocks(P.n)), dim3(kIngestBlock), 0, (hipStream_t)stream, P);
    } else {
        if (P.L.point_step < 1 || P.L.point_step > kIngestMaxStep) return LIVO_E_INVALID;
        const size_t lds = (size_t)kIngestBlock * (size_t)P.L.point_step;
        hipLaunchKernelGGL(k_ingest_cloud, dim3(ingest_blocks(P.n)), dim3(kIngestBlock), lds, (hipStream_t)stream, P);
    }
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_ingest_emit(const IngestParams& P, void* stream) {
    if (P.n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_ingest_emit, dim3(ingest_blocks(P.n)), dim3(kIngestBlock), 0, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_ingest_gather(const float* pts, const uint32_t* perm, int64_t n, float* frame, void* stream) {
    if (n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_ingest_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, perm,
                       n, frame);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_ingest_take_count(const uint32_t* skeys, int64_t from, int64_t n, double limit_ms, unsigned* count,
                             void* stream) {
    hipLaunchKernelGGL(k_ingest_take_count, dim3(1), dim3(64), 0, (hipStream_t)stream, skeys, from, n, limit_ms, count);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

}  // namespace livo
