// vmap_kernels.hip — CDNA4 (gfx950) kernels of the resident visual map and of
// LidarSelector::addFromSparseMap, src/lidar_selection.cpp:332-593.  The
// arithmetic of one item is vmap_model.h's (shared with the host check).
//
//   k_vm_cloud    one cloud point per thread: the world point exactly as
//                 k_to_world stores it, its floor voxel key inserted into the
//                 frame's hash set (one 64-bit CAS per probe; the set has at
//                 least two slots per cloud point, so a probe always ends),
//                 and 1 + its cloud index bid for its depth pixel with a
//                 32-bit atomicMax: the last index wins, as the reference's
//                 sequential loop leaves it.  The depth itself is recomputed
//                 from that index where it is read (the same functions, so
//                 the same bits): the image to clear is 4 bytes a pixel.
//   k_vm_map      one map point per thread: its stored key looked up, the
//                 projection, and one 64-bit atomicMin of distance bits << 32
//                 | ~id for its cell (vm_bid).
//   k_vm_cell     one cell per thread: the cell's point through the depth
//                 continuity test and the view choice; a cell that passes bids
//                 its index for its reference frame's warp (atomicMin).
//   k_vm_warp     one wave per cell that passed: the warp owner's matrix and
//                 level recomputed by the shared function, one warped and one
//                 current sample per lane, NCC and the error summed in index
//                 order by lane 0 from LDS, the keep flag, the cell's record
//                 and patch pyramid, and the warped patch into the map.
//   k_vm_scatter  behind an exclusive scan of the keep flags: one wave per
//                 survivor copies its record, position, level and patches.
//   k_vm_put      livo_vmap_add: one wave per staged observation.
//   k_vm_observe  livo_vio_observe (addObservation, :905-962): one wave per
//                 matched point; the add decision, the eviction at 20
//                 observations and the new observation, in the map.
//   k_vm_frame    livo_vio_detect: the stored frame of the updated state, from
//                 the update's slot on the device (one thread).
//   k_vm_fresh    livo_vio_detect: one wave per selected record: the new
//                 point, its observation and its patch pyramid.
//   k_vm_frame_refs  livo_vmap_release_frames: observations per frame slot,
//                 counted in LDS, one add per slot and block.
// No position is decided by an atomic: two calls give the same bytes.
// Numerics as livo_kernels.hip: -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "livo_internal.h"

namespace livo {

static_assert(sizeof(livo_vmatch_point) == 48, "one 48-B record");
static_assert(kVmBlock % 64 == 0 && kVmBlock <= 1024, "whole waves");
constexpr int kVmWaves = kVmBlock / 64;

__device__ __forceinline__ uint32_t vm_bid_id(unsigned long long b) {
    return 0xFFFFFFFFu - (uint32_t)(b & 0xFFFFFFFFull);
}

__global__ __launch_bounds__(kVmBlock) void k_vm_cloud(VmatchParams P) {
    const int i = blockIdx.x * kVmBlock + threadIdx.x;
    bool fresh = false;
    if (i < (int)P.cloud.n) {
        float wx, wy, wz, depth;
        cloud_world_point(P.cloud, P.W, i, wx, wy, wz);
        int64_t key[3], pix;
        const bool hit = vm_cloud_point(P.cam, P.grid.border, wx, wy, wz, key, pix, depth);
        unsigned long long k;
        if (vm_pack_key(key, k)) {
            const uint32_t mask = (1u << P.vset_log2) - 1u;
            uint32_t s = vm_hash(k, P.vset_log2);
            for (;;) {
                unsigned long long cur = P.vset[s];
                if (cur == kVmBidEmpty) cur = atomicCAS(P.vset + s, kVmBidEmpty, k);
                if (cur == kVmBidEmpty) {
                    fresh = true;
                    break;
                }
                if (cur == k) break;
                s = (s + 1u) & mask;
            }
        }
        if (hit) atomicMax(P.depth + pix, (uint32_t)i + 1u);  // (0 <= pix < w * h: inside the border)
    }
    const bool pred[1] = {fresh};
    const uint32_t v = block_tally<kVmWaves>(pred);
    if (threadIdx.x == 0 && v) atomicAdd(P.ctr + kVmCtrVoxels, (unsigned long long)v);
}

__device__ __forceinline__ bool vm_set_has(const VmatchParams& P, unsigned long long k) {
    const uint32_t mask = (1u << P.vset_log2) - 1u;
    uint32_t s = vm_hash(k, P.vset_log2);
    for (;;) {
        const unsigned long long cur = P.vset[s];
        if (cur == k) return true;
        if (cur == kVmBidEmpty) return false;
        s = (s + 1u) & mask;
    }
}

__global__ __launch_bounds__(kVmBlock) void k_vm_map(VmatchParams P) {
    const int i = blockIdx.x * kVmBlock + threadIdx.x;
    bool tested = false;
    int fate = kVmSkip;
    if (i < P.map.n_points) {
        const VmPoint pt = P.map.pt[i];
        unsigned long long k;
        tested = vm_pack_key(pt.voxel, k) && vm_set_has(P, k);
        if (tested) {
            double pf[3], pc[2];
            int index;
            float dist;
            fate = vm_map_point(P.cam, P.grid, P.fpos, pt.pos, pf, pc, index, dist);
            if (fate == kVmInFrame) atomicMin(P.bid + index, vm_bid(dist, (uint32_t)i));  // (0 <= index < length)
        }
    }
    static_assert(kVmCtrTested + 1 == kVmCtrInFrame && kVmCtrInFrame + 1 == kVmCtrOverflow, "the order");
    const bool pred[3] = {tested, fate != kVmSkip, fate == kVmOverflow};
    const uint32_t v = block_tally<kVmWaves>(pred);
    if (threadIdx.x < 3 && v) atomicAdd(P.ctr + kVmCtrTested + threadIdx.x, (unsigned long long)v);
}

__global__ __launch_bounds__(kVmBlock) void k_vm_cell(VmatchParams P) {
    const int c = blockIdx.x * kVmBlock + threadIdx.x;
    bool marked = false, depth_rej = false, view_rej = false;
    if (c < P.grid.length) {
        const unsigned long long b = P.bid[c];
        marked = b != kVmBidEmpty;
        int chosen = -1;
        if (marked && b != kVmBidNone) {
            const uint32_t id = vm_bid_id(b);
            const VmPoint pt = P.map.pt[id];
            double pf[3], pc[2];
            int index;
            float dist;
            (void)vm_map_point(P.cam, P.grid, P.fpos, pt.pos, pf, pc, index, dist);
            const int half = P.grid.ps / 2, u0 = (int)pc[0], v0 = (int)pc[1];
            for (int u = -half; u <= half && !depth_rej; u++)
                for (int v = -half; v <= half; v++) {
                    if (u == 0 && v == 0) continue;
                    const uint32_t d = P.depth[(int64_t)(v + v0) * P.cam.w + (u + u0)];  // (half < border)
                    if (d == 0u) continue;
                    float wx, wy, wz, depth = 0.0f;
                    cloud_world_point(P.cloud, P.W, (int)(d - 1u), wx, wy, wz);
                    int64_t key[3], pix;
                    (void)vm_cloud_point(P.cam, P.grid.border, wx, wy, wz, key, pix, depth);
                    if (vm_depth_breaks(pf[2], depth)) {
                        depth_rej = true;
                        break;
                    }
                }
            if (!depth_rej) {
                double cosine = 0.0;
                const VmObs* obs = P.map.obs + (size_t)id * kVmMaxObs;
                const int best = vm_close_view(P.fpos, pt.pos, obs, pt.n_obs, P.map.frame, cosine);
                view_rej = pt.n_obs <= 0 || cosine < 0.5;
                if (!view_rej) {
                    chosen = best;
                    atomicMin(P.owner + obs[best].slot, (uint32_t)c);
                }
            }
        }
        P.cand[c] = chosen;
    }
    static_assert(kVmCtrMarked + 1 == kVmCtrDepth && kVmCtrDepth + 1 == kVmCtrView, "the order");
    const bool pred[3] = {marked, depth_rej, view_rej};
    const uint32_t v = block_tally<kVmWaves>(pred);
    if (threadIdx.x < 3 && v) atomicAdd(P.ctr + kVmCtrMarked + threadIdx.x, (unsigned long long)v);
}

__global__ __launch_bounds__(kVmBlock) void k_vm_warp(VmatchParams P) {
    __shared__ float s_ref[kVmWaves][64], s_cur[kVmWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * kVmWaves + wave;  // one wave per cell
    const int chosen = c < P.grid.length ? P.cand[c] : -1;
    const int ps = P.grid.ps, pst = ps * ps;
    bool shared = false, nan = false, ncc_rej = false, err_rej = false, kept = false;
    uint32_t id = 0u;
    double pc[2] = {0.0, 0.0};
    int level = 0;
    float* stored = nullptr;
    if (chosen >= 0) {
        id = vm_bid_id(P.bid[c]);
        const VmPoint pt = P.map.pt[id];
        const VmObs o = P.map.obs[(size_t)id * kVmMaxObs + chosen];
        stored = P.map.patch + ((size_t)id * kVmMaxObs + chosen) * 3 * pst;
        // Warp_map: the matrix and level of the first cell that met this reference frame
        const int oc = (int)P.owner[o.slot];
        shared = oc != c;
        double A[4];
        if (shared) {
            const uint32_t id2 = vm_bid_id(P.bid[oc]);
            const VmPoint pt2 = P.map.pt[id2];
            const VmObs o2 = P.map.obs[(size_t)id2 * kVmMaxObs + P.cand[oc]];
            vm_warp_matrix(P.cam, P.map.frame[o2.slot], o2, pt2.pos, ps / 2, A);
        } else {
            vm_warp_matrix(P.cam, P.map.frame[o.slot], o, pt.pos, ps / 2, A);
        }
        level = vm_search_level(A, 2);
        float Ai[4];
        vm_inverse2f(A, Ai);
        nan = Ai[0] != Ai[0];
        double pf[3];
        int index;
        float dist;
        (void)vm_map_point(P.cam, P.grid, P.fpos, pt.pos, pf, pc, index, dist);
        if (lane < pst) {
            const uint8_t* ref_img = P.map.img + (size_t)o.slot * P.cam.w * P.cam.h;
            s_ref[wave][lane] =
                nan ? stored[lane] : vm_warp_sample(Ai, o.px, level, ps, lane, ref_img, P.cam.w, P.cam.h);
            s_cur[wave][lane] = vis_getpatch(P.img, P.cam.w, pc, ps, 0, lane);
        }
    }
    __syncthreads();
    if (chosen >= 0) {
        float* dst = P.cpatch + (size_t)c * 3 * pst;
        for (int e = lane; e < 3 * pst; e += 64) dst[e] = e < pst ? s_ref[wave][e] : stored[e];
        if (P.store && !nan && lane < pst) stored[lane] = s_ref[wave][lane];
    }
    if (lane == 0 && c < P.grid.length) {
        if (chosen >= 0) {
            double ncc = 0.0;
            float err = 0.0f;
            if (P.ncc_en) {
                ncc = vm_ncc(s_ref[wave], s_cur[wave], pst);
                ncc_rej = ncc < P.ncc_thre;
            }
            if (!ncc_rej) {
                err = vm_error(s_ref[wave], s_cur[wave], pst);
                err_rej = (double)err > P.err_thre;
            }
            kept = !ncc_rej && !err_rej;
            livo_vmatch_point r;
            r.point_id = (int32_t)id;
            r.cell = c;
            r.obs_index = chosen;
            r.frame_id = P.map.obs[(size_t)id * kVmMaxObs + chosen].frame_id;
            r.search_level = level;
            r.error = err;
            r.ncc = ncc;
            r.u = pc[0];
            r.v = pc[1];
            P.rec[c] = r;
        }
        P.keep[c] = kept ? 1u : 0u;
    }
    static_assert(kVmCtrNcc + 1 == kVmCtrError && kVmCtrError + 1 == kVmCtrShared && kVmCtrShared + 1 == kVmCtrNan &&
                      kVmCtrNan + 1 == kVmCtrOut, "the order");
    const bool one = lane == 0;  // a wave's cell counts once
    const bool pred[5] = {one && ncc_rej, one && err_rej, one && shared, one && nan, one && kept};
    const uint32_t v = block_tally<kVmWaves>(pred);
    if (threadIdx.x < 5 && v) atomicAdd(P.ctr + kVmCtrNcc + threadIdx.x, (unsigned long long)v);
}

__global__ __launch_bounds__(kVmBlock) void k_vm_scatter(VmatchParams P) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * kVmWaves + (threadIdx.x >> 6);
    if (c >= P.grid.length || P.keep[c] == 0u) return;
    const uint32_t pos = P.slot[c];
    const livo_vmatch_point r = P.rec[c];
    if (lane == 0) {
        P.out[pos] = r;
        P.levels[pos] = r.search_level;
    }
    if (lane < 3) P.pos[(size_t)pos * 3 + lane] = P.map.pt[r.point_id].pos[lane];
    const int pst3 = 3 * P.grid.ps * P.grid.ps;
    const float* src = P.cpatch + (size_t)c * pst3;
    float* dst = P.patches + (size_t)pos * pst3;
    for (int e = lane; e < pst3; e += 64) dst[e] = src[e];
}

__global__ __launch_bounds__(kVmBlock) void k_vm_put(VmPutParams P) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kVmWaves + (threadIdx.x >> 6);  // one wave per observation
    if (i >= P.n) return;
    const int point = P.point[i];
    const size_t at = (size_t)point * kVmMaxObs + P.index[i];
    if (lane == 0) {
        P.map.obs[at] = P.obs[i];
        P.map.pt[point].n_obs = P.count[i];
    }
    const float* src = P.patches + (size_t)i * P.pst3;
    float* dst = P.map.patch + at * P.pst3;
    for (int e = lane; e < P.pst3; e += 64) dst[e] = src[e];
}

// p[e] = p[e + s] for e in [0, total), s > 0: words moved to lower addresses over
// a range that overlaps itself, by one wave.  It goes upwards in chunks of
// kVmShift * 64 words: all of a chunk's loads are in registers (vmcnt(0)) before
// its first store is issued, so a store never reaches a word that the chunk has
// yet to read, whatever s is (12 or 48 words of a small patch pyramid, 14 of an
// observation: source and destination overlap inside one chunk); later chunks
// read only above what earlier ones wrote.
typedef uint32_t __attribute__((may_alias)) vm_word;
constexpr int kVmShift = 4;
__device__ __forceinline__ void vm_shift_down(vm_word* p, int total, int s, int lane) {
    for (int base = 0; base < total; base += kVmShift * 64) {
        vm_word v[kVmShift];
#pragma unroll
        for (int u = 0; u < kVmShift; u++) {
            const int e = base + u * 64 + lane;
            v[u] = e < total ? p[e + s] : 0u;
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#pragma unroll
        for (int u = 0; u < kVmShift; u++) {
            const int e = base + u * 64 + lane;
            if (e < total) p[e] = v[u];
        }
    }
}

// livo_vio_observe, LidarSelector::addObservation (:905-962): one wave per item,
// and no point twice, so nothing one wave writes is read by another.  The
// projection, delta_p, the pixel distance and the flags are computed alike on
// every lane; the <= 20 frame distances one per lane into LDS, the choice
// (vm_furthest_view) read from there; the 3 ps^2 samples of the new patch
// pyramid spread over the lanes; the eviction's compaction by the whole wave.
// Everything the item reads of its point is read before the first write.
// kResident (livo_vio_detect): the frame's pose comes from its stored VmFrame,
// which k_vm_frame wrote from the updated state, and the ids and levels from the
// match's records: nothing of either has been on the host.
template <bool kResident>
__global__ __launch_bounds__(kVmBlock) void k_vm_observe(VmObserveParams P) {
    static_assert(sizeof(VmObs) % 4 == 0 && sizeof(livo_vobs_point) == 56, "whole words; a 56-B record");
    constexpr int kObsWords = (int)(sizeof(VmObs) / 4);
    __shared__ double s_dist[kVmWaves][kVmMaxObs];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kVmWaves + wave;
    const bool live = i < P.n;
    const int pst = P.ps * P.ps, pst3 = 3 * pst;
    int id = 0, n_obs = 0, fate = kVmObsBehind;
    double pc[2] = {0.0, 0.0}, delta_p = 0.0, pixel_dist = 0.0;
    VmObs* obs = nullptr;
    if (kResident) {
        const VmFrame& f = P.map.frame[P.slot];
        for (int k = 0; k < 9; k++) P.cam.Rcw[k] = f.Rcw[k];
        for (int k = 0; k < 3; k++) {
            P.cam.Pcw[k] = f.Pcw[k];
            P.cpos[k] = f.pos[k];
        }
    }
    if (live) {
        id = kResident ? P.match[i].point_id : P.point[i];
        const VmPoint& pt = P.map.pt[id];
        n_obs = pt.n_obs;  // (1 .. kVmMaxObs: the host keeps the counts)
        obs = P.map.obs + (size_t)id * kVmMaxObs;
        const double pos[3] = {pt.pos[0], pt.pos[1], pt.pos[2]};
        fate = vm_observe_project(P.cam, P.border, pos, pc);
        if (fate == kVmObsIn) {
            delta_p = vm_observe_delta_p(P.map.frame[obs[0].slot], P.cpos);
            pixel_dist = vm_pixel_dist(pc, obs[0].px);
            if (n_obs >= kVmMaxObs && lane < kVmMaxObs)
                s_dist[wave][lane] = vm_view_dist(P.map.frame[obs[lane].slot].pos, P.cpos);
        } else {
            pc[0] = pc[1] = 0.0;
        }
    }
    __syncthreads();
    bool pose = false, pixel = false, added = false, deleted = false;
    int del = -1, del_frame = -1;
    float score = 0.0f;
    if (live && fate == kVmObsIn) {
        pose = delta_p > 0.5;
        pixel = pixel_dist > 40.0;
        added = pose || pixel;
        float fresh[3] = {0.0f, 0.0f, 0.0f};  // (3 ps^2 <= 192: at most 3 samples a lane)
        if (added) {
            const int64_t at = (int64_t)P.slot * P.cam.w * P.cam.h;
            score = vis_score_at(P.map.img, at, P.cam.w, P.cam.h, (int)pc[0], (int)pc[1]);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int e = q * 64 + lane, level = e / pst;
                if (e < pst3) fresh[q] = vis_getpatch(P.map.img + at, P.cam.w, pc, P.ps, level, e - level * pst);
            }
        }
        float* patch = P.map.patch + (size_t)id * kVmMaxObs * pst3;
        if (n_obs >= kVmMaxObs) {  // getFurthestViewObs / deleteFeatureRef, add_flag or not
            del = vm_furthest_view(s_dist[wave], kVmMaxObs);
            del_frame = obs[del].frame_id;
            const int rest = kVmMaxObs - 1 - del;
            vm_shift_down((vm_word*)(obs + del), rest * kObsWords, kObsWords, lane);
            vm_shift_down((vm_word*)(patch + (size_t)del * pst3), rest * pst3, pst3, lane);
            n_obs = kVmMaxObs - 1;
            deleted = true;
        }
        if (added) {  // addFrameRef
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int e = q * 64 + lane;
                if (e < pst3) patch[(size_t)n_obs * pst3 + e] = fresh[q];
            }
            if (lane == 0) {
                VmObs o{};
                o.frame_id = P.frame_id;
                o.level = kResident ? P.match[i].search_level : P.level[i];
                o.slot = P.slot;
                o.px[0] = pc[0];
                o.px[1] = pc[1];
                vm_cam2world(P.cam, pc[0], pc[1], o.f);
                obs[n_obs] = o;
                P.map.pt[id].value = score;
            }
            n_obs += 1;
        }
        if (lane == 0 && (added || deleted)) P.map.pt[id].n_obs = n_obs;
    }
    if (live && lane == 0) {
        livo_vobs_point r;
        r.point_id = id;
        r.flags = (fate == kVmObsBehind ? LIVO_VOBS_BEHIND : 0) | (fate == kVmObsOutOfFrame ? LIVO_VOBS_OUT_OF_FRAME : 0) |
                  (pose ? LIVO_VOBS_POSE : 0) | (pixel ? LIVO_VOBS_PIXEL : 0) | (deleted ? LIVO_VOBS_DELETED : 0) |
                  (added ? LIVO_VOBS_ADDED : 0);
        r.n_obs = n_obs;
        r.deleted_index = del;
        r.deleted_frame_id = del_frame;
        r.score = score;
        r.u = pc[0];
        r.v = pc[1];
        r.delta_p = delta_p;
        r.pixel_dist = pixel_dist;
        P.rec[i] = r;
    }
    static_assert(kVoCtrBehind == 0 && kVoCtrBare == 6 && kVoCtrN == 7, "the order");
    const bool one = live && lane == 0;  // a wave's item counts once
    const bool pred[7] = {one && fate == kVmObsBehind, one && fate == kVmObsOutOfFrame, one && pose, one && pixel,
                          one && added, one && deleted, one && deleted && !added};
    const uint32_t v = block_tally<kVmWaves>(pred);
    if (threadIdx.x < 7 && v) atomicAdd(P.ctr + threadIdx.x, (unsigned long long)v);
}

// livo_vio_detect: the stored frame of the state the update left in its slot.
__global__ __launch_bounds__(64) void k_vm_frame(VmFrameParams P) {
    if (threadIdx.x != 0) return;
    *P.dst = vm_make_frame(P.frame_id, frame_cam(P.vio, *P.state));
}

// livo_vio_detect: one wave per selected record: lane 0 writes the point and its
// observation 0 (vm_make_point, vm_make_obs), the wave copies the patch pyramid.
__global__ __launch_bounds__(kVmBlock) void k_vm_fresh(VmFreshParams P) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kVmWaves + (threadIdx.x >> 6);
    if (i >= P.n) return;
    const int id = P.base + i;  // (< max_points: checked by the host)
    const size_t at = (size_t)id * kVmMaxObs;
    if (lane == 0) {
        const livo_vis_point r = P.pts[i];
        P.map.pt[id] = vm_make_point(r);
        P.map.obs[at] = vm_make_obs(P.K, P.frame_id, P.slot, 0, r.u, r.v);
    }
    const float* src = P.patches + (size_t)i * P.pst3;
    float* dst = P.map.patch + at * P.pst3;
    for (int e = lane; e < P.pst3; e += 64) dst[e] = src[e];
}

// livo_vmap_release_frames: the observations that name each frame slot.  Block
// (x, y) counts kVmRefPer observation places a thread, those of slots
// [y * kVmRefTile, (y + 1) * kVmRefTile), in LDS; then one add per slot it met.
constexpr int kVmRefPer = 8;
__global__ __launch_bounds__(kVmBlock) void k_vm_frame_refs(VmStore map, int32_t n_slots, uint32_t* refs) {
    __shared__ uint32_t s_cnt[kVmRefTile];
    for (int t = threadIdx.x; t < kVmRefTile; t += kVmBlock) s_cnt[t] = 0u;
    __syncthreads();
    const int lo = (int)blockIdx.y * kVmRefTile;
    const int64_t items = (int64_t)map.n_points * kVmMaxObs;
    const int64_t first = (int64_t)blockIdx.x * (kVmBlock * kVmRefPer) + threadIdx.x;
    for (int q = 0; q < kVmRefPer; q++) {
        const int64_t e = first + (int64_t)q * kVmBlock;
        if (e >= items) break;
        const int64_t point = e / kVmMaxObs;
        if ((int)(e - point * kVmMaxObs) >= map.pt[point].n_obs) continue;
        const int s = map.obs[e].slot - lo;
        if (s >= 0 && s < kVmRefTile && s + lo < n_slots) atomicAdd(&s_cnt[s], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kVmRefTile; t += kVmBlock) {
        const uint32_t v = s_cnt[t];
        if (v) atomicAdd(refs + lo + t, v);  // (lo + t < n_slots: counted above)
    }
}

static inline unsigned vm_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

#define VM_LAUNCH(kernel, count, per)                                                                        \
    if ((count) <= 0) return LIVO_OK;                                                                        \
    hipLaunchKernelGGL(kernel, dim3(vm_blocks((count), (per))), dim3(kVmBlock), 0, (hipStream_t)stream, p); \
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP

int launch_vm_cloud(const VmatchParams& p, void* stream) { VM_LAUNCH(k_vm_cloud, p.cloud.n, kVmBlock); }
int launch_vm_map(const VmatchParams& p, void* stream) { VM_LAUNCH(k_vm_map, (int64_t)p.map.n_points, kVmBlock); }
int launch_vm_cell(const VmatchParams& p, void* stream) { VM_LAUNCH(k_vm_cell, (int64_t)p.grid.length, kVmBlock); }
int launch_vm_warp(const VmatchParams& p, void* stream) { VM_LAUNCH(k_vm_warp, (int64_t)p.grid.length, kVmWaves); }
int launch_vm_scatter(const VmatchParams& p, void* stream) {
    VM_LAUNCH(k_vm_scatter, (int64_t)p.grid.length, kVmWaves);
}
int launch_vm_put(const VmPutParams& p, void* stream) { VM_LAUNCH(k_vm_put, (int64_t)p.n, kVmWaves); }
int launch_vm_observe(const VmObserveParams& p, void* stream) {
    VM_LAUNCH(k_vm_observe<false>, (int64_t)p.n, kVmWaves);
}
int launch_vm_observe_resident(const VmObserveParams& p, void* stream) {
    VM_LAUNCH(k_vm_observe<true>, (int64_t)p.n, kVmWaves);
}
int launch_vm_frame(const VmFrameParams& p, void* stream) {
    hipLaunchKernelGGL(k_vm_frame, dim3(1), dim3(64), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}
int launch_vm_fresh(const VmFreshParams& p, void* stream) { VM_LAUNCH(k_vm_fresh, (int64_t)p.n, kVmWaves); }
int launch_vm_frame_refs(const VmStore& map, int32_t n_slots, uint32_t* refs, void* stream) {
    const int64_t items = (int64_t)map.n_points * kVmMaxObs;  // (below 2^31: livo_vmap_reset)
    if (items <= 0 || n_slots <= 0) return LIVO_OK;
    const dim3 grid(vm_blocks(items, kVmBlock * kVmRefPer), vm_blocks(n_slots, kVmRefTile));
    hipLaunchKernelGGL(k_vm_frame_refs, grid, dim3(kVmBlock), 0, (hipStream_t)stream, map, n_slots, refs);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

}  // namespace livo
