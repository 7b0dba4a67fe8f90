// device_common.h — device helpers shared by the kernel files.
#pragma once
#include <hip/hip_runtime.h>

#include "livo_internal.h"

namespace livo {

// ------------------------------------------------ neighbour records ----
// NNRec (livo_internal.h) as eight 16-B parts: the hot half's four
//   part 0 = sqdist[0..3]        part 1 = sqdist[4], idx[0..2]
//   part 2 = idx[3..4], key[0..1] part 3 = key[2..4], cf
// and the cold half's four (xyz[5][3], one pad word).  Writers pack a half
// and store its parts (straight to the record, or through an LDS stage);
// readers go through rec_load.
__device__ __forceinline__ float4 rec_i4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    return make_float4(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z), __uint_as_float(w));
}
__device__ __forceinline__ uint32_t rec_cf(int cnt, int flag) {
    return ((uint32_t)cnt << kRecCntShift) | ((uint32_t)flag & kRecFlagMask);
}
__device__ __forceinline__ void rec_pack_hot(float4 (&h)[4], const float (&d)[kNN], const int32_t (&idx)[kNN],
                                             const uint32_t (&key)[kNN], int cnt, int flag) {
    h[0] = make_float4(d[0], d[1], d[2], d[3]);
    h[1] = make_float4(d[4], __int_as_float(idx[0]), __int_as_float(idx[1]), __int_as_float(idx[2]));
    h[2] = rec_i4((uint32_t)idx[3], (uint32_t)idx[4], key[0], key[1]);
    h[3] = rec_i4(key[2], key[3], key[4], rec_cf(cnt, flag));
}
// nb: (x, y, z, -) of the five neighbours (0 pad)
__device__ __forceinline__ void rec_pack_cold(float4 (&c)[4], const float4 (&nb)[kNN]) {
    c[0] = make_float4(nb[0].x, nb[0].y, nb[0].z, nb[1].x);
    c[1] = make_float4(nb[1].y, nb[1].z, nb[2].x, nb[2].y);
    c[2] = make_float4(nb[2].z, nb[3].x, nb[3].y, nb[3].z);
    c[3] = make_float4(nb[4].x, nb[4].y, nb[4].z, 0.0f);
}
// A full record: both halves, kRecNoXyz cleared.  nb: (x, y, z, sqdist) with
// the (0, 0, 0, +inf) pads; idx: -1 pads.
__device__ __forceinline__ void rec_store_full(NNRec* __restrict__ out, const float4 (&nb)[kNN],
                                               const int32_t (&idx)[kNN], int cnt, int flag) {
    const float d[kNN] = {nb[0].w, nb[1].w, nb[2].w, nb[3].w, nb[4].w};
    const uint32_t key[kNN] = {0u, 0u, 0u, 0u, 0u};
    float4 h[4], c[4];
    rec_pack_hot(h, d, idx, key, cnt, flag & ~(int)kRecNoXyz);
    rec_pack_cold(c, nb);
    float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        o4[k] = h[k];
        o4[4 + k] = c[k];
    }
}
// Neighbour k of a full record written by lane k of a team (the iVox
// searches), and the rest of the record by one lane.
__device__ __forceinline__ void rec_store_neighbor(NNRec* __restrict__ out, int k, const float4 v) {
    out->xyz[k][0] = v.x;
    out->xyz[k][1] = v.y;
    out->xyz[k][2] = v.z;
    out->sqdist[k] = v.w;
}
__device__ __forceinline__ void rec_store_meta(NNRec* __restrict__ out, const int32_t (&idx)[kNN], int cnt, int flag) {
#pragma unroll
    for (int k = 0; k < kNN; k++) {
        out->idx[k] = idx[k];
        out->key[k] = 0u;
    }
    out->cf = rec_cf(cnt, flag & ~(int)kRecNoXyz);
}
__device__ __forceinline__ void rec_clear(NNRec* __restrict__ out) {
    float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
    for (int w = 0; w < 8; w++) o4[w] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void rec_load_cf(const NNRec* __restrict__ r, int& cnt, int& flag) {
    const uint32_t cf = r->cf;
    cnt = rec_cnt(cf);
    flag = rec_flag(cf);
}
__device__ __forceinline__ void rec_store_flag(NNRec* __restrict__ r, int cnt, int flag) { r->cf = rec_cf(cnt, flag); }
// The five neighbours (x, y, z, sqdist) as a full record holds them (pads:
// 0, 0, 0 and the stored distance, +inf from a search), the count and the
// flags.  A kRecNoXyz record's coordinates come from keypts (the cell grid's
// points, 4 floats each) through its keys: only k < cnt is gathered.
__device__ __forceinline__ void rec_load(const NNRec* __restrict__ r, const float4* __restrict__ keypts,
                                         float4 (&nb)[kNN], int& cnt, int& flag) {
    const float4* r4 = reinterpret_cast<const float4*>(r);
    const float4 h0 = r4[0], h1 = r4[1], h2 = r4[2], h3 = r4[3];
    const uint32_t cf = __float_as_uint(h3.w);
    cnt = rec_cnt(cf);
    flag = rec_flag(cf);
    const float d[kNN] = {h0.x, h0.y, h0.z, h0.w, h1.x};
    if (flag & (int)kRecNoXyz) {
        const uint32_t key[kNN] = {__float_as_uint(h2.z), __float_as_uint(h2.w), __float_as_uint(h3.x),
                                   __float_as_uint(h3.y), __float_as_uint(h3.z)};
#pragma unroll
        for (int k = 0; k < kNN; k++) {
            float4 v = make_float4(0.f, 0.f, 0.f, d[k]);
            if (k < cnt) {
                const float4 a = keypts[key[k]];
                v = make_float4(a.x, a.y, a.z, d[k]);
            }
            nb[k] = v;
        }
    } else {
        const float4 c0 = r4[4], c1 = r4[5], c2 = r4[6], c3 = r4[7];
        nb[0] = make_float4(c0.x, c0.y, c0.z, d[0]);
        nb[1] = make_float4(c0.w, c1.x, c1.y, d[1]);
        nb[2] = make_float4(c1.z, c1.w, c2.x, d[2]);
        nb[3] = make_float4(c2.y, c2.z, c2.w, d[3]);
        nb[4] = make_float4(c3.x, c3.y, c3.z, d[4]);
    }
}

__device__ __forceinline__ void world_point(const double* R, const double* pos, const double* RL, const double* tL,
                                            float bxf, float byf, float bzf, float& wx, float& wy, float& wz) {
    // pointBodyToWorld (laser_mapping.cpp:662-671): double math, float storage
    const double bx = bxf, by = byf, bz = bzf;
    const double ix = ((RL[0] * bx + RL[1] * by) + RL[2] * bz) + tL[0];
    const double iy = ((RL[3] * bx + RL[4] * by) + RL[5] * bz) + tL[1];
    const double iz = ((RL[6] * bx + RL[7] * by) + RL[8] * bz) + tL[2];
    wx = (float)(((R[0] * ix + R[1] * iy) + R[2] * iz) + pos[0]);
    wy = (float)(((R[3] * ix + R[4] * iy) + R[5] * iz) + pos[1]);
    wz = (float)(((R[6] * ix + R[7] * iy) + R[8] * iz) + pos[2]);
}
// The world point of cloud index i (the caller's point order), exactly as
// k_to_world stores it.  A world cloud's three floats are returned as stored
// (no identity transform: a -0.0f stays -0.0f).
__device__ __forceinline__ void cloud_world_point(const CloudSrc& S, const WorldParams& W, int i, float& wx, float& wy,
                                                  float& wz) {
    const int64_t k = S.iperm ? (int64_t)S.iperm[i] : (int64_t)i;
    const float* p = S.src + S.stride * k;
    if (S.world) {
        wx = p[0];
        wy = p[1];
        wz = p[2];
        return;
    }
    world_point(W.rot, W.pos, W.R_LI, W.t_LI, p[0], p[1], p[2], wx, wy, wz);
}

// The block's count of each of K per-thread predicates, returned on thread k
// for predicate k (0 on the other threads): a ballot and popcount per wave, an
// LDS row per wave, one __syncthreads.  Every thread of a block of kWaves
// whole waves calls it, once per kernel.  Integer counts: no order to keep.
template <int kWaves, int K>
__device__ __forceinline__ uint32_t block_tally(const bool (&pred)[K]) {
    __shared__ uint32_t cnt[kWaves][K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const unsigned long long m = __ballot(pred[k]);
        if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6][k] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t v = 0;
    if (threadIdx.x < K)
        for (int w = 0; w < kWaves; w++) v += cnt[w][threadIdx.x];
    return v;
}

// XCD-aware block order for a 1-D grid of nb blocks per scan: blocks are dealt
// round-robin over the 8 XCDs, so give each XCD one contiguous run of (scan,
// block) ids -- one region of Morton-ordered points -- and its L2 only the
// part of the map around that region (bijective for any grid size).
__device__ __forceinline__ void xcd_block(int nb, unsigned& job, unsigned& bx) {
    const unsigned nwg = gridDim.x, orig = blockIdx.x, xcd = orig % 8u, q = nwg / 8u, r = nwg % 8u;
    const unsigned wgid = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + orig / 8u;
    job = wgid / (unsigned)nb;
    bx = wgid % (unsigned)nb;
}

// XCD-interleaved block order in chunks of C consecutive blocks: XCD x takes
// chunks x, x + 8, x + 16, ... of the (scan, block) ids, so every XCD holds a
// share of every scan (a batch's scans cost different amounts in a search:
// with one contiguous range per XCD the most expensive scan's XCD is the
// straggler), while a chunk of C Morton-consecutive blocks keeps its map
// region in one L2.  The order is the same in every evaluation, so a block's
// plane cache is re-read on the XCD that wrote it.  C = 0: xcd_block.
__device__ __forceinline__ void xcd_chunk_block(int nb, int C, unsigned& job, unsigned& bx) {
    if (C <= 0) {
        xcd_block(nb, job, bx);
        return;
    }
    const unsigned c = (unsigned)C, orig = blockIdx.x, span = 8u * c;
    const unsigned full = gridDim.x / span * span;
    unsigned wgid = orig;
    if (orig < full) {
        const unsigned k = orig / 8u;
        wgid = ((k / c) * 8u + orig % 8u) * c + k % c;
    }
    job = wgid / (unsigned)nb;
    bx = wgid % (unsigned)nb;
}

// The slot of `key` in an open-addressing table of 2^log2 GridSlots (linear
// probing, load factor <= 1/4), or the empty slot that ends its probe sequence
// (key != `key`); every slot read counts one visit.
__device__ __forceinline__ GridSlot grid_find(const GridSlot* __restrict__ slots, int log2, unsigned long long key,
                                              unsigned& visits) {
    const uint64_t mask = (1ull << log2) - 1ull;
    uint64_t sl = grid_hash(key, log2);
    GridSlot g = slots[sl];
    visits++;
    while (g.key != key && g.key != kGridEmpty) {
        sl = (sl + 1) & mask;
        g = slots[sl];
        visits++;
    }
    return g;
}

// Centre of grid cell v along one axis, and the squared distance of a point to
// a cell centre: the cell runs' sort key (k_cr_rho) and the search's
// termination test (vrun_search) use exactly these operations, so both see
// the same bits.
__device__ __forceinline__ float cell_centre(float org, float h, int v) { return org + ((float)v + 0.5f) * h; }
__device__ __forceinline__ float centre_d2(float cx, float cy, float cz, float x, float y, float z) {
    const float t0 = x - cx, t1 = y - cy, t2 = z - cz;
    return (t0 * t0 + t1 * t1) + t2 * t2;
}
__device__ __forceinline__ float cr_rho2(const float org[3], float h, int v0, int v1, int v2, float x, float y,
                                         float z) {
    return centre_d2(cell_centre(org[0], h, v0), cell_centre(org[1], h, v1), cell_centre(org[2], h, v2), x, y, z);
}

}  // namespace livo
