// livo_capi.cpp — the C ABI (include/livo.h): context, device map, resident
// scans, and the host side of the batched IEKF loop.
//
// Host control is launch-only: every evaluation of the IEKF loop
// (laser_mapping.cpp:178) is one k_hshare launch + one k_solve launch on the
// context's stream, and the loop's branches (convergence, rematch, stop) are
// taken on the device (IekfCtrl), so a scan update costs one host->device
// upload of the states and one device->host read of the results, with no
// round trip per iteration.  Evaluations past a scan's stop exit at the first
// instruction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <chrono>
#include <thread>
#include <vector>

#include "host_layouts.h"
#include "livo_internal.h"
#include "upload_plan.h"

using namespace livo;

namespace {

// A resident scan: its device arrays (ScanArrays, upload_plan.h) and its state.
struct ScanBuf : ScanArrays {
    bool used = false;
    int64_t n = 0;
    int32_t nblk = 0;
    std::vector<int32_t> perm;  // d_perm on the host, fetched on first use (host_perm)
    bool searched = false;      // a search has filled the neighbour cache
    bool nn_compact = false;    // a fused batch may have stored hot-only records (kRecNoXyz): ensure_nn_coords
    bool nn_lazy = false;       // the last fused search skipped records: ensure_nn_records rebuilds them ...
    double nn_pose[12] = {};    // ... by the same search at its pose (rot, pos; IekfSlot::nn_pose)
    int64_t cap = 0;            // points the buffers were sized for (>= n; reused after a release)
    hipEvent_t ready = nullptr; // livo_scan_upload_async: recorded on the upload stream when the scan is built
    bool pending = false;       // an asynchronous upload may still be building it (get_scan waits)
};

template <typename T>
static int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    if (hipMalloc((void**)p, count * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        return LIVO_E_OOM;
    }
    return LIVO_OK;
}

template <typename T>
static void dev_free(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

// A grow-only device buffer of `need` bytes: kept if it is large enough, else
// freed and allocated again (its contents are not carried over).
static int ensure_dev_bytes(void** p, size_t* have, size_t need) {
    if (need <= *have) return LIVO_OK;
    if (*p) (void)hipFree(*p);  // (the caller has drained the stream that used it)
    *p = nullptr;
    *have = 0;
    if (hipMalloc(p, need) != hipSuccess) return LIVO_E_OOM;
    *have = need;
    return LIVO_OK;
}

// An image kept on the device for the later calls that pass none (w = h = 0: none).
struct DevImage {
    uint8_t* p = nullptr;
    size_t cap = 0;
    int32_t w = 0, h = 0;
};
static bool image_reusable(const DevImage& m, int32_t w, int32_t h) { return m.p && m.w == w && m.h == h; }
// Enqueues the upload of a host image.  There is no image to reuse from here on:
// the caller sets w and h once its stream synchronise has succeeded.
static int image_stage(DevImage& m, const uint8_t* host, size_t bytes, hipStream_t st) {
    m.w = m.h = 0;
    void* p = m.p;
    const int rc = ensure_dev_bytes(&p, &m.cap, bytes);
    m.p = (uint8_t*)p;
    if (rc) return rc;
    return hipMemcpyAsync(m.p, host, bytes, hipMemcpyHostToDevice, st) == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

// What a LiDAR frame hands to the camera frames behind it (livo_cloud_publish):
// pcl_wait_pub and pg_down, 5 floats a point, in one allocation that grows and
// never shrinks.
struct WorldCloud {
    void* buf = nullptr;
    size_t bytes = 0;
    const float* world = nullptr;  // n rows
    const float* down = nullptr;   // n_down rows (world itself where the filter kept its input)
    int64_t n = -1;                // -1: nothing published
    int64_t n_down = -1;           // -1: pg_down not built
    bool filtered = false;
};

static void free_scan_buf(ScanBuf& s) {
    scan_arrays(s, s.cap, [](auto*& p, size_t) { dev_free(p); });
    if (s.ready) (void)hipEventDestroy(s.ready);
    s.ready = nullptr;
}

}  // namespace

// The resident visual map (livo_vmap_*): the points, their observations and
// patches and the frame table in one buffer, the frames' images in another
// (sized by the first frame), and the host's copy of what validation needs.
struct VmapDev {
    bool ready = false;
    int64_t max_points = 0, max_frames = 0, n_obs = 0;
    int32_t ps = 0, w = 0, h = 0;
    void* buf = nullptr;
    size_t bytes = 0;
    void* img = nullptr;
    size_t img_bytes = 0;
    VmStore dev{};                 // the arrays in buf / img, n_points and n_frames
    CamIntrinsics K{};             // of the frames (the first one's)
    std::vector<int32_t> count;    // observations per point
    std::vector<VmFrame> frames;   // by slot; id < 0: released (livo_vmap_release_frames)
    std::vector<int32_t> free_slots;  // the released slots, descending: the lowest is taken first
    int64_t live_frames() const { return (int64_t)frames.size() - (int64_t)free_slots.size(); }
};

// The device iVox map and its AddPoints / overflow-pass scratch.
struct IvoxDev {
    bool ready = false;
    int kind = -1;  // search kernel (IvoxParams::kind), LIVO_IVOX_KIND=thread|wave|team read by livo_ivox_init
    int64_t add_passes = 0;  // device passes AddPoints took (one per batch, more at LRU conflicts)
    livo_ivox_params prm{};
    float inv_res = 5.0f;
    int nearby = 19;
    GridSlot* slots = nullptr;
    int32_t log2 = 0;
    int64_t table = 0;
    uint32_t *addcnt = nullptr, *tot = nullptr, *newstart = nullptr, *addstart = nullptr;
    float* pts[2] = {nullptr, nullptr};  // CSR double buffer (4 floats per point)
    int64_t pts_cap[2] = {0, 0};
    int cur = 0;
    int64_t npts = 0, ngrids = 0, next_id = 0, max_grid = 0;
    unsigned long long* ctr = nullptr;   // [0] error bits, [1] new grids, [2] max grid
    // batch temporaries
    float* src = nullptr;
    uint32_t *slot_of = nullptr, *iota = nullptr, *skeys = nullptr, *svals = nullptr;
    int64_t src_cap = 0;
    // overflow pass of the search
    SelElem* big = nullptr;
    int64_t big_threads = 0, big_slice = 0;
    // LRU grid cache: per slot last-use id, per-batch first / last touch, eviction mark
    unsigned long long* tlast = nullptr;
    uint32_t *first = nullptr, *lastp1 = nullptr;
    uint8_t* evict = nullptr;
    // eviction scratch (allocated the first time the capacity is reached): ev_cap of each, carved from ev_buf
    void* ev_buf = nullptr;
    size_t ev_bytes = 0;
    unsigned long long *ev_k = nullptr, *ev_k2 = nullptr;
    uint32_t *ev_a = nullptr, *ev_b = nullptr, *ev_c = nullptr, *ev_d = nullptr;
    int64_t ev_cap = 0;
};

// The ikd-Tree incremental map (ikd_incr_kernels.hip): the point set by id
// and the scratch of Add_Points / the grid rebuild.
struct DynDev {
    bool active = false;
    float* all = nullptr;        // per id: x, y, z, id bits
    uint8_t* alive = nullptr;
    int64_t cap = 0, n_ids = 0, n_alive = 0;
    float cmax = 0.f;            // largest |coordinate| (the grid's rounding slack)
    unsigned long long *keys = nullptr, *skeys = nullptr;
    uint32_t *iota = nullptr, *svals = nullptr, *heads = nullptr, *runid = nullptr, *starts = nullptr;
    int64_t sort_cap = 0;
    void* add_buf = nullptr;     // Add_Points' scratch: add_cap points of each array below, one carve
    size_t add_bytes = 0;
    float *W = nullptr, *seq = nullptr, *Ws = nullptr;
    uint32_t *defer = nullptr, *dpos = nullptr, *dlist = nullptr, *keep = nullptr, *apos = nullptr;
    int64_t add_cap = 0;
    float* boxes = nullptr;
    int64_t box_cap = 0;
    unsigned long long *dirty = nullptr, *ctr = nullptr;
    int64_t gslot_cap = 0, gpts_cap = 0;  // capacities of ctx->gslots / ctx->gpts
    livo_map_add_stats last{};
    // The IEKF search keeps the cell and ball runs on the incremental map:
    // the runs index the base point set rpts (the map's points
    // in grid order when the runs were built; ids below base_ids), a deleted
    // base point is marked in rpts (x = NaN, never a candidate of the run scans), and
    // the points added since are searched in the delta grid (dslots / dpts, the
    // cell grid's layout).  When the delta or the deleted share grows past
    // rebase_frac of the base the runs are rebuilt from the current points.
    bool runs = false;
    float* rpts = nullptr;           // base points: x, y, z, id bits (x = NaN once deleted)
    uint32_t* rpos = nullptr;        // base id -> position in rpts (~0: not in the base / marked)
    int64_t base_ids = 0, base_n = 0, rpts_cap = 0, rpos_cap = 0;
    int64_t tomb = 0;                // base points marked deleted
    GridSlot* dslots = nullptr;
    float* dpts = nullptr;
    int32_t dlog2 = 4;
    GridSlot* dvslots = nullptr;     // the delta grid's cell runs (positions in dpts)
    uint32_t* dvidx = nullptr;
    int32_t dvlog2 = 4;
    int64_t d_n = 0, dslot_cap = 0, dpts_cap = 0;
    int64_t rebases = 0;
    double rebase_frac = 0.125;      // LIVO_DYN_REBASE
    float min_gh = 0.f;              // the cell-walk grid's edge range: [box_cell, box_cell_max] x the Add_Points box
    float max_gh = 0.f;
    float box_cell = 1.2f;           // LIVO_DYN_BOX_CELL
    float box_cell_max = 2.0f;       // LIVO_DYN_BOX_CELL_MAX (0: no upper bound)
    // The grid rebuild merges instead of re-sorting (dyn_rebuild_merge): the
    // grid holds every alive id below grid_ids in (key, id) order on cells of
    // edge grid_gh (-1: unknown, the next rebuild sorts), `cells` of them.
    float* gpts_alt = nullptr;       // the merge's output, swapped with ctx->gpts
    int64_t gpts_alt_cap = 0;
    int64_t grid_ids = -1, cells = -1;
    float grid_gh = 0.f;
    bool merge = true;               // LIVO_DYN_MERGE=0: always sort
    int64_t rebuilds_sorted = 0, rebuilds_merged = 0;
    int64_t wide_redos = 0;          // Add_Points batches redone with 64-bit box keys
    int64_t rebuilds_fused = 0;      // merged rebuilds run in Add_Points' pass (one read-back)
    ScanCtx scan;                    // the one-launch scans' ticket and status words
};

// A batch's staging area: its slots, then its jobs, in a device buffer (d) and
// in pinned host memory (h), one contiguous copy each way.
struct Staging {
    char* h = nullptr;
    char* d = nullptr;
    char* h_dev = nullptr;  // h's device address (host-mapped), for the kernel copies; null: DMA copies
    size_t cap = 0;
    void free() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        h = d = h_dev = nullptr;
        cap = 0;
    }
    int ensure(size_t bytes) {
        if (bytes <= cap) return LIVO_OK;
        free();
        // zeroed: a group staged inline (BatchPlan::Group::inl) never copies the slots' ticket
        // lines in; they start at 0 here and every pass's completers leave them at 0
        // (the fill runs on the null stream, which the lanes' non-blocking streams do not wait
        // for: it is finished here, before the batch that asked for the area queues its copies)
        if (hipMalloc((void**)&d, bytes) != hipSuccess || hipMemset(d, 0, bytes) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) {
            (void)hipGetLastError();
            if (d) (void)hipFree(d);
            d = nullptr;
            return LIVO_E_OOM;
        }
        // mapped + coherent: a submitted batch's staging copies are kernels
        // (launch_copy_words) that read and write it; DMA copies behind another
        // lane's kernels held the submitting host 2-3 ms per batch
        if (hipHostMalloc((void**)&h, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            h = nullptr;
            return LIVO_E_OOM;
        }
        if (hipHostGetDevicePointer((void**)&h_dev, h, 0) != hipSuccess) {
            (void)hipGetLastError();
            h_dev = nullptr;  // DMA copies then
        }
        cap = bytes;
        return LIVO_OK;
    }
};

// What batch_enqueue decided for the batch a lane carries; batch_collect reads it.
struct BatchPlan {
    int model = 0;
    int32_t n = 0;
    bool fused = false;  // search + replay + plane pass + solve in one launch per evaluation
    bool kcopy = false;  // staging copies by kernel over host-mapped memory (else DMA)
    bool wb = false;     // the stopping solve writes its slot into the host staging copy itself
    bool iv = false;     // iVox search (its own overflow replay lists)
    bool lazy = false;   // fused: searches after the first skip unread records (KnnParams::rec_lazy)
    int prof = 0;       // profiling level of this batch (0: no event is recorded)
    // livo_lio_frame: the one scan's state lies on the device; its slot is staged there
    // (k_lio_stage_slot) instead of init_slot + the upload
    const livo_state* dev_state = nullptr;
    Staging* stage = nullptr;
    size_t stride = 0;   // bytes from one slot to the next
    int ngroups = 0;
    struct Group {
        int32_t first, count;
        int max_nblk;
        int64_t max_n, off;  // off: the group's start in the lane's replay list
        hipStream_t st;
        bool inl;            // staged in its launches' arguments (EvalInline): no staging copy on its stream
    } g[kMaxGroups];
};

// One batch in flight: its staging (one area per model: LaserMapping slots are
// packed at kLmStride, the part before the IKFoM block; IKFoM slots are whole),
// its plan and its end events.  Every lane queues on the context's streams.
struct BatchLane {
    Staging stage[2];  // by model
    hipStream_t st[kMaxGroups] = {};
    hipEvent_t done[kMaxGroups] = {};  // each group's last operation (its slot copy back)
    bool busy = false;   // submitted, not yet collected
    int32_t ticket = -1;
    int32_t n = 0;
    BatchPlan plan;
    std::vector<int32_t> ids;
};

// pinned staging buffers of livo_scan_upload_async (two batches of 8 ahead)
constexpr int kPinRing = 16;
// A stream / an event created on first use (null again if that fails).
static bool lazy_stream(hipStream_t* s) {
    if (*s || hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess) return true;
    *s = nullptr;
    return false;
}
static bool lazy_event(hipEvent_t* e) {
    if (*e || hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess) return true;
    *e = nullptr;
    return false;
}
struct PinSlot {
    float* h = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;  // the last copy out of h
    bool inflight = false;        // such a copy was enqueued and not yet waited for (pin_take, pin_sent)
};

// What the asynchronous uploads keep.  livo_scan_upload_async copies and builds
// on `up`, out of a ring of pinned staging buffers (each reused once the copy
// out of it is done).  livo_scan_upload_batch_async copies on `cp` into two
// alternating device staging buffers, so batch k+1's copy runs beside batch k's
// build on `up` (Src::copied gates the build, Src::free the next copy into the
// same buffer).  Both build in tmp and sort in prim.
struct UploadDev {
    hipStream_t up = nullptr, cp = nullptr;
    void* tmp = nullptr;  // Morton keys, sort buffers, bounds (single scans: then the packed points)
    size_t tmp_bytes = 0;
    void* prim = nullptr;  // rocPRIM scratch
    size_t prim_bytes = 0;
    PinSlot pin[kPinRing];
    int pin_next = 0;
    struct Src {
        void* p = nullptr;
        size_t bytes = 0;
        hipEvent_t copied = nullptr, free = nullptr;
        bool used = false;  // `free` has been recorded
    } src[2];
    int src_next = 0;

    // The upload stream and (batch) the copy stream and the staging buffers'
    // events: whatever is missing is created.
    // (the builds on a high-priority stream were slower: 3.8k vs 11.8k updates/s
    // with uploads)
    int streams(bool batch) {
        bool ok = lazy_stream(&up);
        if (batch) {
            ok = ok && lazy_stream(&cp);
            for (Src& s : src) ok = ok && lazy_event(&s.copied) && lazy_event(&s.free);
        }
        return ok ? LIVO_OK : LIVO_E_HIP;
    }
    // Every queued upload done: both streams are waited for, whatever the first answers.
    int drain() {
        const bool a = !cp || hipStreamSynchronize(cp) == hipSuccess;
        const bool b = !up || hipStreamSynchronize(up) == hipSuccess;
        return a && b ? LIVO_OK : LIVO_E_HIP;
    }
    void destroy() {
        (void)drain();
        for (Src& s : src) {
            if (s.p) (void)hipFree(s.p);
            if (s.copied) (void)hipEventDestroy(s.copied);
            if (s.free) (void)hipEventDestroy(s.free);
        }
        if (tmp) (void)hipFree(tmp);
        if (prim) (void)hipFree(prim);
        for (PinSlot& P : pin) {
            if (P.h) (void)hipHostFree(P.h);
            if (P.copied) (void)hipEventDestroy(P.copied);
        }
        if (cp) (void)hipStreamDestroy(cp);
        if (up) (void)hipStreamDestroy(up);
    }
};

// IMU forward propagation: a stream of its own (the calls touch neither the map nor
// the scans, so they do not queue behind a batch in flight), one device and one pinned
// staging area, and what livo_imu_propagate leaves for livo_scan_preprocess_imu.
struct ImuDev {
    hipStream_t st = nullptr;
    void* buf = nullptr;   // states, carries, counts, jobs, samples, the batch's Pose6D rows
    size_t bytes = 0;
    void* pin = nullptr;   // the same layout up to the samples, page-locked
    size_t pin_bytes = 0;
    void* table = nullptr; // the resident table (rows x 22 doubles)
    size_t table_bytes = 0;
    int32_t rows = 0;      // 0: no table resident
    bool sorted = true;    // its offset times are non-decreasing (the backward walk needs that)
    double rot_end[9] = {}, pos_end[3] = {};
};

// The sensor handlers' frame (livo_frame_ingest_*): one allocation holds the uploaded message,
// the passes' scratch and the resident result, the time-ordered frame with its sorted keys.
struct IngestDev {
    void* buf = nullptr;
    size_t bytes = 0;
    const float* frame = nullptr;     // n_kept x 5 floats, ascending time (meas.lidar)
    const uint32_t* skeys = nullptr;  // their order-preserving time keys
    unsigned* ctr = nullptr;          // kIngCtr*
    bool have = false;                // an ingest has succeeded
    livo_ingest_info info{};
};

// The loop search (livo_std_*): the database in one allocation sized by livo_std_reset, the
// staged key frame and the search's match arrays in two that grow.
struct StdDev {
    bool ready = false, staged = false, searched = false, cells_known = false;
    livo_std_params prm{};
    int64_t max_descs = 0, max_frames = 0, max_planes = 0;
    int64_t n_descs = 0, n_planes = 0, cells = 0;
    int32_t n_frames = 0;
    std::vector<uint32_t> plane_off;   // the host's copy of the frames' plane ranges
    void* buf = nullptr;               // records, both index copies, planes, the per-frame and per-candidate arrays
    size_t bytes = 0;
    StdHot* hot = nullptr;
    StdVerts* verts = nullptr;
    unsigned long long* skey[2] = {};  // the sorted (cell key, sequence) index; a commit merges cur -> 1 - cur
    uint32_t* sseq[2] = {};
    int cur = 0;
    livo_std_plane* planes = nullptr;
    uint32_t* d_plane_off = nullptr;
    StdParams P{};                     // the search's arrays (those carved from buf; the others per call)
    void* stage = nullptr;             // the staged frame, its new index entries and per-source counts
    size_t stage_bytes = 0;
    livo_std_desc* src = nullptr;
    livo_std_plane* src_planes = nullptr;
    unsigned long long *nkey = nullptr, *snkey = nullptr;
    uint32_t *nseq = nullptr, *snseq = nullptr;
    int64_t n_src = 0, n_src_planes = 0;
    uint32_t id_min = 0, id_max = 0;   // of the staged frame_ids
    void* mbuf = nullptr;              // matches, their keys and order, the success lists
    size_t mbytes = 0;
    int64_t n_matches = 0;
    int32_t n_cand = 0;
    std::vector<livo_std_candidate> cands;  // the last search's records
    std::vector<uint32_t> coff;
};

// GenerateSTDescs (livo_std_key_*, livo_std_generate): the key cloud and the stages' arrays, one
// grow-only allocation per stage (points, voxels, jobs, corners, candidates).
struct StdGenDev {
    float* key = nullptr;              // the key cloud, x y z
    size_t key_bytes = 0;
    int64_t n_key = 0;
    void* buf[5] = {};
    size_t bytes[5] = {};
    StdGen last{};                     // the last generate's arrays (livo_std_gen_debug, livo_std_staged's corners)
    bool have = false;                 // the staged frame is that generate's
};

struct livo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // extra streams for the groups of a batch (overlap of latency-bound kernels)
    hipStream_t xstream[kMaxGroups - 1] = {};
    hipEvent_t xjoin[kMaxGroups - 1] = {};
    // stream groups per batch (LIVO_STREAM_GROUPS; 0: the default of
    // batch_plan, four for the fused and IKFoM paths, two for iVox,
    // profiles/r04_ab_groups.txt)
    int groups = 0;
    int leaf_size = kLeafSize;         // leaf-map points per leaf (LIVO_LEAF_SIZE)
    livo_params params{};
    // map
    MapNode* nodes = nullptr;
    int64_t map_points = 0;
    int64_t map_slots = 0;
    int32_t map_depth = 0;
    LeafNode* lnodes = nullptr;        // leaf map (batched IEKF search)
    float* lpts = nullptr;
    int32_t leaf_depth = 0;
    int64_t leaf_bytes = 0;
    int knn_kind = 2;                  // batched search: 0 leaf map, 1 cell grid, 2 cell grid + LDS tiles (LIVO_KNN_KIND)
    bool fused = true;                 // kind 2: one k_iekf_eval launch per evaluation (LIVO_FUSED=0: separate passes)
    float grid_cell = 0.f;             // cell edge (LIVO_GRID_CELL; 0: from the map)
    float grid_ppc = 0.f;              // target points per occupied cell when chosen from the map (LIVO_GRID_PPC)
    bool vruns = true;                 // cell runs on a static map (LIVO_VRUNS=0: the cell walk)
    // k_iekf_eval block order (LIVO_XCD_CHUNK): XCD-interleaved chunks of 8 blocks, so
    // every XCD holds a share of every scan (distinct-scan pool: 18.6k vs 17.6k /
    // 18.3k vs 17.1k / 17.1k vs 16.4k updates/s against 0, one range per XCD, whose
    // most expensive scan's XCD was the straggler; profiles/r04_ab_block_order.txt)
    int xcd_chunk = 8;
    GridSlot* vslots = nullptr;        // vertex runs (static map only)
    uint32_t* vpts = nullptr;          // run entries: grid positions (indices into gpts)
    int32_t vlog2 = 0;
    // ball runs (static map only): anchor cells of edge bh, runs of radius brmax
    bool bruns = true;                 // LIVO_BRUNS=0: the cell runs only
    // bh = br_ha r5, brmax = sqrt(3)/2 bh + br_r r5 (LIVO_BR_HA / LIVO_BR_R).  R = 6
    // (round 4; 3.2 before): on distinct scans the queries a ball of 3.2 r5 left
    // uncertified (off the surfaces by the prior's pose error) certify in their
    // ball run instead of the cell run and walk: pooled 21.4k vs 18.5k updates/s,
    // first evaluation 0.157 vs 0.231 ms; R = 8 / 10 / 13 no better
    // (profiles/r04_ab_ball_radius.txt)
    float br_ha = 2.0f, br_r = 6.0f;
    GridSlot* bslots = nullptr;
    uint32_t* bpts = nullptr;
    int32_t blog2 = 0;
    float bh = 0.f, brmax = 0.f, br5 = 0.f;
    int64_t bentries = 0;
    int32_t bchunks = 0;               // anchor chunks of the ball runs' build
    GridSlot* gslots = nullptr;        // cell grid
    float* gpts = nullptr;
    float gorg[3] = {0.f, 0.f, 0.f};
    float gh = 1.f, geps = 0.f, gcmax = 0.f;
    DynDev dyn;                        // the incremental map (livo_map_add_points, ...)
    int32_t glog2 = 0;
    int64_t grid_bytes = 0;
    bool has_map = false;
    int backend = LIVO_BACKEND_IKDTREE;  // search structure of h_share / the IEKF loop
    IvoxDev iv;                        // iVox map (LIVO_BACKEND_IVOX)
    void* fe_buf = nullptr;            // scan front-end scratch (livo_scan_preprocess)
    size_t fe_bytes = 0;
    const float* fe_raw = nullptr;     // the last preprocessed frame, de-skewed, full resolution (5 floats a point)
    int64_t fe_n = 0;
    WorldCloud wcloud;                 // livo_cloud_publish: pcl_wait_pub and pg_down
    ImuDev imu;                        // livo_imu_propagate(_batch): stream, staging, the resident Pose6D table
    IngestDev ing;                     // livo_frame_ingest_*: the current frame and its cursor
    StdDev stdb;                       // livo_std_*: the loop search's database, staged frame and last search
    StdGenDev sgen;                    // livo_std_key_*, livo_std_generate
    void* vio_buf = nullptr;           // VIO frame (image, points, partials, slot)
    size_t vio_bytes = 0;
    DevImage bgr_img;                  // livo_cloud_colorize: the last uploaded BGR image (reused by bgr == NULL)
    DevImage gray_img;                 // livo_vio_select: the last uploaded gray image (reused by gray == NULL)
    void* vis_buf = nullptr;           // ... and its cell table, flags, slots, counters, records and patches
    size_t vis_bytes = 0;
    VmapDev vmap;                      // the resident visual map (livo_vmap_*)
    DevImage match_img;                // livo_vio_match: the last uploaded gray image (reused by gray == NULL)
    void* vm_buf = nullptr;            // ... and its voxel set, depth image, bids, records and patches
    size_t vm_bytes = 0;
    DevImage det_img;                  // livo_vio_detect: the frame's gray image, uploaded once
    void* det_buf = nullptr;           // ... and every stage's arrays, one carve
    size_t det_bytes = 0;
    void* prim_tmp = nullptr;         // rocPRIM scratch (sorts, scans)
    size_t prim_bytes = 0;
    // scans
    std::vector<ScanBuf> scans;
    // released scans' device buffers, reused by the next upload of a scan that
    // fits (a drop-in run uploads and releases one scan per frame: hipMalloc /
    // hipFree of its buffers cost more than the update itself)
    std::vector<ScanBuf> spare;
    // upload scratch: Morton keys, sort buffers, bounds and the packed source points
    void* up_tmp = nullptr;
    size_t up_tmp_bytes = 0;
    UploadDev up;  // livo_scan_upload_async, livo_scan_upload_batch_async: streams, scratch, staging
    // one slot and one job: the scratch of the single-scan entry points (ensure_slot)
    IekfSlot* d_slots = nullptr;
    // batches in flight (livo_iekf_update_batch_submit): lane 0 also carries
    // every synchronous batch
    BatchLane lane[LIVO_MAX_INFLIGHT];
    int32_t lane_gen = 0;  // tickets: generation * LIVO_MAX_INFLIGHT + lane
    // LIVO_LANE_SERIAL=1: a queued batch starts only once every group of the one
    // before it is done; default 0: its group 0 starts when stream 0 frees, beside
    // the other groups' tails (20.5k vs 19.1k updates/s, profiles/r03_ab_lanes.txt)
    bool lane_serial = false;
    bool slot_wb = true;            // fused batches: the stopping solve writes the slot back (LIVO_SLOT_WB)
    bool stage_copy = false;        // submitted fused batches stage by copy kernel as before (LIVO_STAGE_COPY=1)
    // the fused run searches on a static map store hot-only neighbour records, the
    // coordinates filled on demand (LIVO_REC_COMPACT=0: full records)
    bool rec_compact = true;
    // ... and their later searches skip the records nothing in the loop reads; a scan's
    // records are rebuilt on demand (ensure_nn_records; LIVO_REC_LAZY=0: stored)
    bool rec_lazy = true;
    // LIVO_EVAL_GEN=1: every fused evaluation takes the generic kernel (the A/B and test reference
    // of the static-map specialisation)
    bool eval_gen = false;
    int last_lane = -1;             // lane of the batch enqueued last
    unsigned long long last_replays = 0;  // profiled batches: the replay counter read back
    IekfSlot* h_slots = nullptr;  // pinned
    HsJob* d_jobs = nullptr;
    HsJob* h_jobs = nullptr;      // pinned
    // exact-replay list of the k-NN passes
    unsigned* d_replay_count = nullptr;
    unsigned long long* d_replay_total = nullptr;
    unsigned long long* d_replay_list = nullptr;
    int64_t replay_cap = 0;
    // iVox: the wave pass's overflow for the global-memory pass (KnnParams::replay_list2);
    // per group of lane 0 (the iVox batches are synchronous)
    unsigned* d_replay_count2 = nullptr;
    unsigned long long* d_replay_list2 = nullptr;
    // scratch for livo_knn / debug outputs
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    // ensure_nn_records: the plane cache and plane states its launch writes (the scan's own stay)
    void* rec_tmp = nullptr;
    size_t rec_tmp_bytes = 0;
    // profiling
    int profiling = 0;
    hipEvent_t ev[kMaxGroups][3 * LIVO_MAX_EVALS + 2] = {};
    hipEvent_t b_start = nullptr, b_end[2] = {};  // profiling level 2: batch span and the gap before it
    int b_par = 0;
    bool b_prev = false;
    bool events_ready = false;
    livo_timings last{};
};

#define HIP_TRY(x)                                  \
    do {                                            \
        if ((x) != hipSuccess) return LIVO_E_HIP;   \
    } while (0)
#define RC_TRY(x)                  \
    do {                           \
        const int rc_ = (x);       \
        if (rc_) return rc_;       \
    } while (0)

// Host wait for a stream: spin on hipStreamQuery (microseconds to notice
// completion), then fall back to the blocking wait after ~50 ms.
static hipError_t stream_wait(hipStream_t st) {
    for (int k = 0; k < 200000; k++) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
    }
    return hipStreamSynchronize(st);
}

// The same for an event (a batch's end when other work may queue behind it).
static hipError_t event_wait(hipEvent_t ev) {
    for (int k = 0; k < 200000; k++) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
    }
    return hipEventSynchronize(ev);
}

static int set_device(livo_ctx* c) {
    return hipSetDevice(c->device) == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

// Devices the runtime sees (0 where it reports an error): the entry points added since the
// context-free ones answer LIVO_E_HIP on it before they touch their context.
static int hip_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

static int ensure_scratch(livo_ctx* c, size_t bytes) {
    return ensure_dev_bytes(&c->scratch, &c->scratch_bytes, bytes);
}

// The single-scan entry points' slot and job (livo_knn, livo_h_share, livo_ivox_knn,
// livo_map_incremental), device and pinned host; batches stage in their lane.
static int ensure_slot(livo_ctx* c) {
    if (!c->d_slots && dev_alloc(&c->d_slots, 1)) return LIVO_E_OOM;
    if (!c->d_jobs && dev_alloc(&c->d_jobs, 1)) return LIVO_E_OOM;
    if (!c->h_slots && hipHostMalloc((void**)&c->h_slots, sizeof(IekfSlot), hipHostMallocDefault) != hipSuccess) {
        c->h_slots = nullptr;
        return LIVO_E_OOM;
    }
    if (!c->h_jobs && hipHostMalloc((void**)&c->h_jobs, sizeof(HsJob), hipHostMallocDefault) != hipSuccess) {
        c->h_jobs = nullptr;
        return LIVO_E_OOM;
    }
    return LIVO_OK;
}

// kLmStride-packed LaserMapping slots + jobs of a batch of n (host pinned and device).
constexpr size_t kLmStride = (kSlotLmBytes + 255) & ~(size_t)255;
static_assert(kLmStride % alignof(HsJob) == 0 && kLmStride % alignof(IekfSlot) == 0, "packed slot alignment");
static_assert(kLmStride % 16 == 0, "kernel staging copies move 16-B words");
// bytes of a batch's packed staging area, rounded up to whole 16-B words
static size_t lm_bytes(int32_t n) { return ((size_t)n * (kLmStride + sizeof(HsJob)) + 15) & ~(size_t)15; }
// bytes of a batch's staging area by model, never less than a batch of 8 needs
static size_t stage_bytes(int model, int32_t n) {
    n = std::max(n, 8);
    return model == kModelIkfom ? (size_t)n * (sizeof(IekfSlot) + sizeof(HsJob)) : lm_bytes(n);
}

// A lane's end events and group streams.  Every lane queues on the context's
// streams: a batch submitted behind another starts the moment the device
// finishes the first (no host round trip, copy or launch latency in between),
// without running beside it (MI355X, 8 x 100k: two batches on streams of their
// own, so concurrent, 10-13k updates/s against 16.9k for one at a time,
// profiles/r03_ab_lanes.txt).
static int lane_streams(livo_ctx* c, int L) {
    BatchLane& B = c->lane[L];
    if (B.st[0]) return LIVO_OK;
    for (int k = 0; k < kMaxGroups; k++)
        if (!B.done[k] && hipEventCreateWithFlags(&B.done[k], hipEventDisableTiming) != hipSuccess) return LIVO_E_HIP;
    B.st[0] = c->stream;
    for (int k = 0; k < kMaxGroups - 1; k++) B.st[k + 1] = c->xstream[k];
    return LIVO_OK;
}

static bool any_inflight(const livo_ctx* c) {
    for (const BatchLane& B : c->lane)
        if (B.busy) return true;
    return false;
}

// Coordinates on demand: a scan whose last fused batch may have stored hot-only
// neighbour records gets their cold halves on `st`, ahead of a consumer on that
// stream that reads coordinates from the records.  (The keys index the cell
// grid as it is now: fill_all_nn_coords runs before anything replaces it.)
static int ensure_nn_records(livo_ctx* c, ScanBuf* s, hipStream_t st);
static int ensure_nn_coords(livo_ctx* c, ScanBuf* s, hipStream_t st) {
    RC_TRY(ensure_nn_records(c, s, st));  // (skipped records first: they come back whole)
    if (!s->nn_compact) return LIVO_OK;
    s->nn_compact = false;
    if (s->n == 0 || !c->gpts) return LIVO_OK;
    return launch_fill_nn_coords(s->nn, s->n, c->gpts, st);
}
// Before the map, its grid or its runs change: every flagged live scan, finished.
static int fill_all_nn_coords(livo_ctx* c) {
    bool any = false;
    for (auto& s : c->scans) {
        if (!s.used || !s.nn_compact) continue;
        if (s.pending && s.ready) HIP_TRY(hipEventSynchronize(s.ready));
        const int rc = ensure_nn_coords(c, &s, c->stream);
        if (rc) return rc;
        any = true;
    }
    if (any) HIP_TRY(hipStreamSynchronize(c->stream));
    return LIVO_OK;
}

static bool params_valid(const livo_params* p) {
    return p && p->laser_point_cov > 0.0 && p->max_iterations >= 0 && p->max_iterations + 1 <= LIVO_MAX_EVALS &&
           p->flags == 0;
}

// Replay counters and lists per lane (LIVO_MAX_INFLIGHT slices: lane L's
// counters at L * kMaxGroups, its list at L * replay_cap), so two unfused
// batches in flight (IKFoM) keep theirs apart.
static int ensure_replay(livo_ctx* c, int64_t total) {
    if (!c->d_replay_count && dev_alloc(&c->d_replay_count, (size_t)kMaxGroups * LIVO_MAX_INFLIGHT)) return LIVO_E_OOM;
    if (!c->d_replay_total) {
        if (dev_alloc(&c->d_replay_total, 1)) return LIVO_E_OOM;
        HIP_TRY(hipMemset(c->d_replay_total, 0, sizeof(unsigned long long)));
    }
    if (!c->d_replay_count2) {
        if (dev_alloc(&c->d_replay_count2, (size_t)kMaxGroups)) return LIVO_E_OOM;
        HIP_TRY(hipMemset(c->d_replay_count2, 0, sizeof(unsigned) * kMaxGroups));
    }
    if (total <= c->replay_cap) return LIVO_OK;
    dev_free(c->d_replay_list);  // (hipFree waits for the device: no batch is still using it)
    dev_free(c->d_replay_list2);
    c->replay_cap = 0;
    if (dev_alloc(&c->d_replay_list, (size_t)total * LIVO_MAX_INFLIGHT)) return LIVO_E_OOM;
    if (dev_alloc(&c->d_replay_list2, (size_t)total)) return LIVO_E_OOM;
    c->replay_cap = total;
    return LIVO_OK;
}

static IvoxParams ivox_params(livo_ctx* c);

static KnnParams make_knn_params(livo_ctx* c) {
    KnnParams kp{};
    kp.nodes = c->nodes;
    kp.jobs = c->d_jobs;
    kp.replay_count = c->d_replay_count;
    kp.replay_list = c->d_replay_list;
    kp.replay_count2 = c->d_replay_count2;
    kp.replay_list2 = c->d_replay_list2;
    kp.replay_total = c->d_replay_total;
    std::memcpy(kp.R_LI, c->params.R_LI, sizeof(kp.R_LI));
    std::memcpy(kp.t_LI, c->params.t_LI, sizeof(kp.t_LI));
    kp.has_map = c->has_map && c->map_points > 0 ? 1 : 0;
    kp.force = -1;
    kp.depth = c->map_depth;
    kp.n_nodes = c->has_map ? c->map_slots : 0;
    kp.lnodes = c->lnodes;
    kp.lpts = c->lpts;
    kp.ldepth = c->leaf_depth;
    kp.lM = c->has_map ? c->map_points : 0;
    kp.gslots = c->gslots;
    kp.gpts = c->gpts;
    std::memcpy(kp.gorg, c->gorg, sizeof(kp.gorg));
    kp.gh = c->gh;
    kp.geps = c->geps;
    kp.glog2 = c->glog2;
    // the incremental map keeps the runs of its base point set (+ deletion marks
    // and the delta grid, dyn_runs_update) or, without them, the cell walk
    const bool dyn_runs = c->dyn.active && c->dyn.runs;
    const bool vr = c->vslots && (!c->dyn.active || dyn_runs);
    kp.rpts = dyn_runs ? c->dyn.rpts : c->gpts;
    kp.dslots = dyn_runs && c->dyn.d_n > 0 ? c->dyn.dslots : nullptr;
    kp.dpts = dyn_runs ? c->dyn.dpts : nullptr;
    kp.dlog2 = c->dyn.dlog2;
    kp.dvslots = dyn_runs && c->dyn.d_n > 0 ? c->dyn.dvslots : nullptr;
    kp.dvidx = c->dyn.dvidx;
    kp.dvlog2 = c->dyn.dvlog2;
    kp.dyn_runs = dyn_runs ? 1 : 0;
    kp.vslots = vr ? c->vslots : nullptr;
    kp.vpts = vr ? c->vpts : nullptr;
    kp.vlog2 = c->vlog2;
    const bool br = vr && c->bslots;
    kp.bslots = br ? c->bslots : nullptr;
    kp.bpts = br ? c->bpts : nullptr;
    kp.blog2 = c->blog2;
    kp.bh = c->bh;
    // certification: every point within the final bound lies in the ball (the build
    // keeps points with cr_rho2 <= brmax^2 in float: a relative 1e-5 below covers its rounding)
    kp.bcert2 = c->brmax * c->brmax * (1.0f - 1e-5f);
    kp.xcd_chunk = c->xcd_chunk;
    kp.identity = 0;
    kp.iv = ivox_params(c);
    kp.canon = c->dyn.active ? 1 : 0;
    kp.rec_compact = (c->rec_compact && vr && !c->dyn.active) ? 1 : 0;
    kp.rec_lazy = (kp.rec_compact && c->rec_lazy && !c->eval_gen) ? 1 : 0;
    kp.eval_gen = c->eval_gen ? 1 : 0;
    return kp;
}

// k-NN pass + exact replay of its flagged queries (one replay list per pass).
static int knn_pass(const KnnParams& kp, int n_jobs, int64_t max_n, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(kp.replay_count, 0, sizeof(unsigned), st));
    // the incremental map has no reference-order tree: the grid search + canonical replay
    if (kp.canon) return launch_knn_grid(kp, n_jobs, max_n, false, false, st);
    return launch_knn_pass(kp, n_jobs, max_n, st);
}

static float morton_scale() {
    static const float scale = [] {  // cells per metre (LIVO_MORTON_SCALE tuning knob)
        const char* e = std::getenv("LIVO_MORTON_SCALE");
        const float v = e ? (float)std::atof(e) : 4.0f;
        return v > 0.0f ? v : 4.0f;
    }();
    return scale;
}

static HsParams make_hs_params(livo_ctx* c) {
    HsParams hp{};
    hp.jobs = c->d_jobs;
    std::memcpy(hp.R_LI, c->params.R_LI, sizeof(hp.R_LI));
    std::memcpy(hp.t_LI, c->params.t_LI, sizeof(hp.t_LI));
    hp.inv_r = 1.0 / c->params.laser_point_cov;
    hp.lpc = c->params.laser_point_cov;
    hp.max_res = c->params.max_residual;
    hp.plane_thr = c->params.plane_threshold;
    // the iVox branch has no sqdist gate (laser_mapping.cpp:519-525)
    hp.max_sqd = c->backend == LIVO_BACKEND_IVOX ? INFINITY : c->params.max_nn_sqdist;
    hp.force = -1;
    hp.keypts = c->gpts;
    return hp;
}

static void fill_job(HsJob& j, ScanBuf& s, IekfSlot* slot) {
    j.pts = s.pts;
    j.nn = s.nn;
    j.partial = s.partial;
    j.plane = s.plane;
    j.pstate = s.pstate;
    j.ikrows = s.ikrows;
    j.ikcnt = s.ikcnt;
    j.host_slot = nullptr;
    j.slot = slot;
    j.n = (int32_t)s.n;
    j.nblk = s.nblk;
}

// IKFoM: x_ = x_propagated = the input state (its cov is P_propagated); the
// first h_dyn_share searches (dyn_share.converge = true, esekfom.hpp:1623).
static void init_slot_ik(IekfSlot& s, const livo_ikfom_state& st, int max_iter) {
    std::memset(&s, 0, sizeof(IekfSlot));
    s.model = kModelIkfom;
    s.ik.x = st;
    s.ik.xp = st;
    s.ctrl.search_en = 1;
    s.ctrl.iter_count = -1;
    s.ctrl.max_iter = max_iter;
}

// The covariance factors of the device solve (IekfSlot::covL / covB): the
// state covariance is fixed for the whole IEKF loop of a scan (it changes only
// when the loop stops, laser_mapping.cpp:224-227), so the 6x6 Cholesky of its
// pose block S = P(0:6, 0:6) = L L^T and B = P(:, 0:6) L^-T are formed once, on
// the host, when the slot is staged.  cov_ok = 0 (the device then takes its
// pivoted 6x6 LU path) unless P's first six rows and columns are symmetric and
// S is numerically positive definite.
static void cov_factor(IekfSlot& s) {
    const double* P = s.state.cov;
    constexpr int D = kDim;
    s.cov_ok = 0;
    double amax = 0.0;
    for (int i = 0; i < D; i++)
        for (int j = 0; j < 6; j++) {
            const double a = P[i * D + j], b = P[j * D + i];
            if (!std::isfinite(a) || !std::isfinite(b)) return;
            amax = std::max(amax, std::fabs(a));
        }
    for (int i = 0; i < D; i++)
        for (int j = 0; j < 6; j++)
            if (std::fabs(P[i * D + j] - P[j * D + i]) > 1e-12 * amax) return;
    double Lm[36] = {};
    for (int j = 0; j < 6; j++) {
        double d = P[j * D + j];
        for (int k = 0; k < j; k++) d -= Lm[j * 6 + k] * Lm[j * 6 + k];
        if (!(d > 1e-13 * P[j * D + j]) || !(d > 0.0)) return;  // not (numerically) positive definite
        const double l = std::sqrt(d);
        Lm[j * 6 + j] = l;
        for (int i = j + 1; i < 6; i++) {
            double v = P[i * D + j];
            for (int k = 0; k < j; k++) v -= Lm[i * 6 + k] * Lm[j * 6 + k];
            Lm[i * 6 + j] = v / l;
        }
    }
    double Bm[(D - 6) * 6];
    for (int r = 6; r < D; r++)  // B(r, :) L^T = P(r, 0:6): forward substitution
        for (int j = 0; j < 6; j++) {
            double v = P[r * D + j];
            for (int k = 0; k < j; k++) v -= Bm[(r - 6) * 6 + k] * Lm[j * 6 + k];
            Bm[(r - 6) * 6 + j] = v / Lm[j * 6 + j];
        }
    for (double v : Bm)
        if (!std::isfinite(v)) return;
    std::memcpy(s.covL, Lm, sizeof(Lm));
    std::memcpy(s.covB, Bm, sizeof(Bm));
    s.cov_ok = 1;
}

// bytes: how much of the slot to clear; the batched LaserMapping update uploads
// and reads only its first kSlotLmBytes, so it clears only those
static void init_slot(IekfSlot& s, const livo_state& st, const livo_state& prior, int max_iter,
                      size_t bytes = sizeof(IekfSlot)) {
    std::memset(&s, 0, bytes);
    s.state = st;
    s.prior = prior;
    s.ctrl.stop = 0;
    s.ctrl.search_en = 1;
    s.ctrl.iter_count = -1;
    s.ctrl.rematch_num = 0;
    s.ctrl.max_iter = max_iter;
    cov_factor(s);
}

// Records on demand: a scan whose last fused search left out the records nothing in the
// loop read (nn_lazy) gets all of them back -- the same search again, at the pose that
// search ran at (nn_pose), against the map as it still is (every caller that changes the
// map comes here first, fill_all_nn_coords).  One k_iekf_eval<false> launch that searches,
// stores full records (rec_compact off: both halves, as LIVO_REC_COMPACT=0 stores them),
// replays its flagged queries and stops at the sums (no solve): deterministic, so the
// bytes are those the loop's search would have stored.  The launch's plane cache and plane
// states go to a buffer of the context's: the scan's own stay as the loop left them (an
// evaluation after the last search may have fitted planes the search left at state 0).
// Finished on `st` before it returns: the staging slot and that buffer are the context's.
static int ensure_nn_records(livo_ctx* c, ScanBuf* s, hipStream_t st) {
    if (!s->nn_lazy) return LIVO_OK;
    s->nn_lazy = false;
    if (!s->searched || s->n == 0) return LIVO_OK;  // (invalidated records: searched again before any read)
    RC_TRY(ensure_slot(c));
    RC_TRY(ensure_replay(c, s->n));
    livo_state pose{};
    std::memcpy(pose.rot, s->nn_pose, 9 * sizeof(double));
    std::memcpy(pose.pos, s->nn_pose + 9, 3 * sizeof(double));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (an earlier user of the staging slot)
    RC_TRY(ensure_dev_bytes(&c->rec_tmp, &c->rec_tmp_bytes, carve_bytes(plane_tmp_layout, (size_t)s->n)));
    Carve k{(char*)c->rec_tmp};
    const PlaneTmp T = plane_tmp_layout(k, (size_t)s->n);
    init_slot(c->h_slots[0], pose, pose, c->params.max_iterations);
    fill_job(c->h_jobs[0], *s, c->d_slots);
    c->h_jobs[0].plane = T.plane;
    c->h_jobs[0].pstate = T.pstate;
    HIP_TRY(hipMemcpyAsync(c->d_slots, c->h_slots, sizeof(IekfSlot), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->d_jobs, c->h_jobs, sizeof(HsJob), hipMemcpyHostToDevice, st));
    KnnParams kp = make_knn_params(c);
    kp.rec_compact = 0;
    kp.rec_lazy = 0;
    HsParams hp = make_hs_params(c);
    hp.solve = 0;
    RC_TRY(launch_iekf_eval(kp, hp, 1, s->n, false, st));
    HIP_TRY(hipStreamSynchronize(st));
    s->nn_compact = false;  // (full records)
    return LIVO_OK;
}

static int create_group_streams(livo_ctx* c) {
    for (int k = 0; k < kMaxGroups - 1; k++) {
        if (hipStreamCreateWithFlags(&c->xstream[k], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->xjoin[k], hipEventDisableTiming) != hipSuccess)
            return 1;
    }
    return 0;
}


// ------------------------------------------------------------------ iVox --
static void ivox_free(IvoxDev& v) {
    dev_free(v.slots);
    dev_free(v.addcnt); dev_free(v.tot); dev_free(v.newstart); dev_free(v.addstart);
    dev_free(v.pts[0]); dev_free(v.pts[1]);
    dev_free(v.ctr);
    dev_free(v.src); dev_free(v.slot_of); dev_free(v.iota); dev_free(v.skeys); dev_free(v.svals);
    dev_free(v.big);
    dev_free(v.tlast); dev_free(v.first); dev_free(v.lastp1); dev_free(v.evict);
    dev_free(v.ev_buf);
    v = IvoxDev{};
}

// Rehash into a table of 2^log2 slots (and per-slot arrays to match).
static int ivox_rehash_to(livo_ctx* c, int log2) {
    IvoxDev& v = c->iv;
    if (log2 > 31) return LIVO_E_RANGE;
    const int64_t table = (int64_t)1 << log2;
    GridSlot* slots = nullptr;
    unsigned long long* tlast = nullptr;
    if (dev_alloc(&slots, (size_t)table) || dev_alloc(&tlast, (size_t)table)) {
        dev_free(slots);
        return LIVO_E_OOM;
    }
    int rc = launch_ivox_clear(slots, table, c->stream);
    if (!rc && v.slots) rc = launch_ivox_rehash(v.slots, v.tlast, v.table, slots, tlast, log2, c->stream);
    if (rc) {
        dev_free(slots);
        dev_free(tlast);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    dev_free(v.slots);
    dev_free(v.tlast);
    dev_free(v.addcnt); dev_free(v.tot); dev_free(v.newstart); dev_free(v.addstart);
    dev_free(v.first); dev_free(v.lastp1); dev_free(v.evict);
    v.slots = slots;
    v.tlast = tlast;
    v.table = table;
    v.log2 = log2;
    if (dev_alloc(&v.addcnt, table) || dev_alloc(&v.tot, table) || dev_alloc(&v.newstart, table) ||
        dev_alloc(&v.addstart, table) || dev_alloc(&v.first, table) || dev_alloc(&v.lastp1, table) ||
        dev_alloc(&v.evict, table))
        return LIVO_E_OOM;
    HIP_TRY(hipMemsetAsync(v.addcnt, 0, (size_t)table * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(v.first, 0xFF, (size_t)table * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(v.lastp1, 0, (size_t)table * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(v.evict, 0, (size_t)table, c->stream));
    return LIVO_OK;
}

static int table_log2_for(int64_t grids) {
    int log2 = 10;
    while (((int64_t)1 << log2) < 4 * grids) log2++;
    return log2;
}

// Hash table with room for `grids` grids at load factor <= 1/2 (rehash on growth).
static int ivox_ensure_table(livo_ctx* c, int64_t grids) {
    IvoxDev& v = c->iv;
    if (v.table >= 2 * grids && v.table > 0) return LIVO_OK;
    return ivox_rehash_to(c, table_log2_for(grids));
}

// After an insert sized for its worst case (every point a new grid): shrink a
// table left below 1/16 full, so the per-slot passes of later inserts stay short.
static int ivox_trim_table(livo_ctx* c) {
    IvoxDev& v = c->iv;
    const int log2 = table_log2_for(std::max<int64_t>(v.ngrids, 256));
    return log2 + 2 <= v.log2 ? ivox_rehash_to(c, log2) : LIVO_OK;
}

static int ivox_ensure_src(livo_ctx* c, int64_t n) {
    IvoxDev& v = c->iv;
    if (n <= v.src_cap) return LIVO_OK;
    const int64_t cap = std::max<int64_t>(n, 4096);
    dev_free(v.src); dev_free(v.slot_of); dev_free(v.iota); dev_free(v.skeys); dev_free(v.svals);
    v.src_cap = 0;
    if (dev_alloc(&v.src, (size_t)cap * 4) || dev_alloc(&v.slot_of, cap) || dev_alloc(&v.iota, cap) ||
        dev_alloc(&v.skeys, cap) || dev_alloc(&v.svals, cap))
        return LIVO_E_OOM;
    v.src_cap = cap;
    return LIVO_OK;
}

static int ensure_prim(livo_ctx* c, size_t bytes) {
    return ensure_dev_bytes(&c->prim_tmp, &c->prim_bytes, bytes);
}

// Exclusive scan of n u32 through rocPRIM (out != in).
static int scan_u32(livo_ctx* c, const uint32_t* in, uint32_t* out, int64_t n) {
    size_t tb = 0;
    int rc = prim_exclusive_scan_u32(nullptr, &tb, in, out, n, c->stream);
    if (!rc) rc = ensure_prim(c, tb);
    tb = c->prim_bytes;
    if (!rc) rc = prim_exclusive_scan_u32(c->prim_tmp, &tb, in, out, n, c->stream);
    return rc;
}

// The count behind an exclusive scan, pos[n - 1] + flags[n - 1]: read() enqueues
// the two copies (none for n == 0), sum() holds once the caller has synchronised.
struct ScanCount {
    uint32_t w[2] = {0u, 0u};
    int read(const uint32_t* pos, const uint32_t* flags, int64_t n, hipStream_t st) {
        if (n <= 0) return LIVO_OK;
        HIP_TRY(hipMemcpyAsync(&w[0], pos + n - 1, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&w[1], flags + n - 1, 4, hipMemcpyDeviceToHost, st));
        return LIVO_OK;
    }
    int64_t sum() const { return (int64_t)w[0] + w[1]; }
};

// Stable radix sort of n (key, value) pairs through rocPRIM (`sort`: prim_sort_pairs_u32 /
// _u64) on `st`: sized with a null scratch, the scratch grown, then run.  drain: the stream
// is synchronised before its scratch grows (the upload streams, which may still be sorting in it).
template <class K>
static int sort_pairs_on(int (*sort)(void*, size_t*, const K*, K*, const uint32_t*, uint32_t*, int64_t, int, void*),
                         hipStream_t st, void** prim, size_t* prim_bytes, bool drain, const K* kin, K* kout,
                         const uint32_t* vin, uint32_t* vout, int64_t n, int bits) {
    size_t tb = 0;
    int rc = sort(nullptr, &tb, kin, kout, vin, vout, n, bits, st);
    if (!rc && drain && tb > *prim_bytes && hipStreamSynchronize(st) != hipSuccess) rc = LIVO_E_HIP;
    if (!rc) rc = ensure_dev_bytes(prim, prim_bytes, tb);
    tb = *prim_bytes;
    if (!rc) rc = sort(*prim, &tb, kin, kout, vin, vout, n, bits, st);
    return rc;
}
static int sort_u32_on(hipStream_t st, void** prim, size_t* prim_bytes, bool drain, const uint32_t* kin, uint32_t* kout,
                       const uint32_t* vin, uint32_t* vout, int64_t n, int bits) {
    return sort_pairs_on(prim_sort_pairs_u32, st, prim, prim_bytes, drain, kin, kout, vin, vout, n, bits);
}
// ... on the context's stream and scratch
static int sort_u32(livo_ctx* c, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, int64_t n,
                    int bits) {
    return sort_u32_on(c->stream, &c->prim_tmp, &c->prim_bytes, false, kin, kout, vin, vout, n, bits);
}
static int sort_u64(livo_ctx* c, const unsigned long long* kin, unsigned long long* kout, const uint32_t* vin,
                    uint32_t* vout, int64_t n) {
    return sort_pairs_on(prim_sort_pairs_u64, c->stream, &c->prim_tmp, &c->prim_bytes, false, kin, kout, vin, vout, n, 64);
}

static IvoxParams ivox_params(livo_ctx* c) {
    IvoxDev& v = c->iv;
    IvoxParams P{};
    P.slots = v.slots;
    P.pts = v.pts[v.cur];
    P.npts = v.pts[1 - v.cur];
    P.src = v.src;
    P.table = v.table;
    P.addcnt = v.addcnt;
    P.tot = v.tot;
    P.newstart = v.newstart;
    P.addstart = v.addstart;
    P.slot_of = v.slot_of;
    P.iota = v.iota;
    P.skeys = v.skeys;
    P.svals = v.svals;
    P.ctr = v.ctr;
    P.base_id = v.next_id;
    P.inv_res = v.inv_res;
    P.log2 = v.log2;
    P.nearby = v.nearby;
    P.max_num = kNN;
    P.kind = v.kind;
    P.range2 = 5.0 * 5.0;  // GetClosestPoint's default max_range (ivox3d.h:79), laser_mapping.cpp:520
    P.scratch = v.big;
    P.slice = v.big_slice;
    P.tlast = v.tlast;
    P.first = v.first;
    P.lastp1 = v.lastp1;
    P.evict = v.evict;
    return P;
}

// Overflow-pass scratch: a slice holds every candidate one query can hold at once.
static int ivox_ensure_big(livo_ctx* c) {
    IvoxDev& v = c->iv;
    const int64_t slice = (int64_t)v.nearby * kNN + v.max_grid + 8;
    if (slice <= v.big_slice && v.big) return LIVO_OK;
    const int64_t budget = (int64_t)1 << 28;  // 256 MiB per stream group
    int64_t threads = budget / (slice * (int64_t)sizeof(SelElem));
    threads = std::max<int64_t>(64, std::min<int64_t>(16384, threads)) / 64 * 64;
    dev_free(v.big);
    v.big_slice = 0;
    v.big_threads = 0;
    if (dev_alloc(&v.big, (size_t)(kMaxGroups * threads * slice))) return LIVO_E_OOM;  // one set per stream group
    v.big_slice = slice;
    v.big_threads = threads;
    return LIVO_OK;
}

// IVox::AddPoints of the n points in v.src (insertion order), on the device.
static int ivox_ev_scratch(livo_ctx* c, int64_t need) {
    IvoxDev& v = c->iv;
    if (need <= v.ev_cap) return LIVO_OK;
    v.ev_cap = 0;
    const size_t cap = (size_t)need;
    auto layout = [&](Carve k) {
        v.ev_k = k.take<unsigned long long>(cap);
        v.ev_k2 = k.take<unsigned long long>(cap);
        v.ev_a = k.take<uint32_t>(cap);
        v.ev_b = k.take<uint32_t>(cap);
        v.ev_c = k.take<uint32_t>(cap);
        v.ev_d = k.take<uint32_t>(cap);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&v.ev_buf, &v.ev_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)v.ev_buf});
    v.ev_cap = need;
    return LIVO_OK;
}

// The longest prefix [0, *pend) of the batch whose evictions all take old
// grids the prefix never touches, and their count *evs (0: the first eviction
// already needs a grid the batch touched before it).  At eviction k (the point
// t_ev[k] creating a new grid) grids_cache_.back() is the oldest old grid the
// batch has not touched before t_ev[k] (touched ones moved to the front,
// ivox3d.h:263-268); a victim the batch touches again later would be
// re-created, so the prefix ends before that touch.  Victims advance
// monotonically along the LRU order: one host pass over the old grids' first
// touches.
static int ivox_evict_prefix(livo_ctx* c, const IvoxParams& P, int64_t n_old, const std::vector<uint32_t>& t_ev,
                             int64_t n, int64_t* pend, int64_t* evs) {
    IvoxDev& v = c->iv;
    std::vector<uint32_t> f((size_t)n_old);
    int rc = launch_ivox_oldfirst(P, v.ev_b, n_old, v.ev_a, c->stream);
    if (rc) return rc;
    if (n_old > 0) HIP_TRY(hipMemcpyAsync(f.data(), v.ev_a, (size_t)n_old * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t end = n, k = 0, i = 0;
    for (; k < (int64_t)t_ev.size() && (int64_t)t_ev[k] < end; k++) {
        const uint32_t t = t_ev[k];
        while (i < n_old && f[(size_t)i] < t) i++;  // touched before this eviction: not the oldest
        if (i == n_old) {                            // no untouched old grid left
            end = t;
            break;
        }
        if (f[(size_t)i] != 0xFFFFFFFFu) end = std::min<int64_t>(end, f[(size_t)i]);
        i++;
    }
    *pend = end;
    *evs = k;
    return LIVO_OK;
}

// IVox::AddPoints (ivox3d.h:256-281) of the points src[off, off + n) as one
// device batch, with the LRU eviction at capacity.  *done = points consumed:
// all of them, or (when an eviction would hit a grid the batch itself touches
// later, or every old grid is touched first) the prefix up to and including
// the first evicting point, processed with its single eviction -- AddPoints of
// a prefix then of the rest is AddPoints of the whole.
static int ivox_add_part(livo_ctx* c, int64_t off, int64_t n, int64_t* done) {
    IvoxDev& v = c->iv;
    *done = 0;
    if (v.npts + n > (int64_t)0xFFFFFFFF || v.next_id + n > (int64_t)0x7FFFFFFF) return LIVO_E_RANGE;
    int rc = ivox_ensure_table(c, v.ngrids + n);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(v.ctr, 0, 5 * sizeof(unsigned long long), c->stream));
    IvoxParams P = ivox_params(c);
    P.src = v.src + 4 * off;
    P.n_src = n;
    rc = launch_ivox_insert(P, c->stream);
    if (rc) return rc;
    unsigned long long ctr[5];
    HIP_TRY(hipMemcpyAsync(ctr, v.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ctr[0] & 1ull) {
        rc = launch_ivox_rollback(P, c->stream);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
        return rc ? rc : LIVO_E_RANGE;
    }
    const int64_t E = v.ngrids, N_new = (int64_t)ctr[1], C = v.prm.capacity;
    int64_t ev = std::max<int64_t>(0, E + N_new - (C - 1));  // grids_map_.size() >= capacity_ after a creation
    int64_t consumed = n;
    if (ev > 0) {
        rc = ivox_ev_scratch(c, std::max<int64_t>(v.table, n));
        if (rc) return rc;
        // the point of the first eviction: the (C - 1 - E)-th new grid by creation
        unsigned long long* cnt = v.ctr + 3;  // (scratch counter; ctr[3] is set again below)
        HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), c->stream));
        rc = launch_ivox_newfirst(P, v.ev_a, cnt, c->stream);
        if (!rc) rc = sort_u32(c, v.ev_a, v.ev_b, v.ev_a, v.ev_c, N_new, 32);
        if (rc) return rc;
        // creation index of each new grid from the (C - 1 - E)-th: the eviction times
        const int64_t c0 = std::max<int64_t>(0, C - 1 - E);
        std::vector<uint32_t> t_ev((size_t)(N_new - c0));
        HIP_TRY(hipMemcpyAsync(t_ev.data(), v.ev_b + c0, t_ev.size() * 4, hipMemcpyDeviceToHost, c->stream));
        // the old grids from the least recently used: victims and the conflict check
        HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), c->stream));
        rc = launch_ivox_oldkeys(P, v.ev_k, v.ev_a, cnt, c->stream);
        if (rc) return rc;
        const int64_t n_old = E;
        rc = sort_u64(c, v.ev_k, v.ev_k2, v.ev_a, v.ev_b, n_old);
        if (!rc) rc = launch_ivox_untouched(P, v.ev_b, n_old, v.ev_c, c->stream);
        if (!rc) rc = scan_u32(c, v.ev_c, v.ev_d, n_old);
        ScanCount untouched;
        if (!rc) rc = untouched.read(v.ev_d, v.ev_c, n_old, c->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint32_t j_first = t_ev[0];
        bool conflict = ev > untouched.sum();
        if (!conflict) {
            HIP_TRY(hipMemsetAsync(v.ctr + 3, 0, sizeof(unsigned long long), c->stream));
            rc = launch_ivox_victims(P, v.ev_b, v.ev_d, n_old, ev, j_first, c->stream);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(ctr, v.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            conflict = (ctr[0] & 2ull) != 0;
        }
        if (conflict) {
            // A run of evictions: the longest prefix whose victims are old grids
            // it leaves untouched (ivox_evict_prefix), inserted again alone.
            int64_t pend = 0, evs = 0;
            rc = ivox_evict_prefix(c, P, n_old, t_ev, n, &pend, &evs);
            if (rc) return rc;
            rc = launch_ivox_rollback(P, c->stream);
            if (rc) return rc;
            if (evs > 0) {
                P.n_src = pend;
                HIP_TRY(hipMemsetAsync(v.ctr, 0, 5 * sizeof(unsigned long long), c->stream));
                rc = launch_ivox_insert(P, c->stream);
                if (!rc) rc = launch_ivox_untouched(P, v.ev_b, n_old, v.ev_c, c->stream);
                if (!rc) rc = scan_u32(c, v.ev_c, v.ev_d, n_old);
                // (the victims kernel's conflict flag is conservative -- it also flags
                // an older grid touched between two evictions -- the scan is exact: off)
                if (!rc) rc = launch_ivox_victims(P, v.ev_b, v.ev_d, n_old, evs, 0xFFFFFFFFu, c->stream);
                if (rc) return rc;
                HIP_TRY(hipMemcpyAsync(ctr, v.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                if ((ctr[0] & 2ull) || E + (int64_t)ctr[1] - (C - 1) != evs) {  // (the scan's invariant)
                    // undo the prefix's uncommitted slots, so the table stays clean for the next AddPoints
                    rc = launch_ivox_rollback(P, c->stream);
                    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
                    return rc ? rc : LIVO_E_HIP;
                }
                consumed = pend;
                ev = evs;
                conflict = false;
            }
        }
        if (conflict) {
            // the first eviction's victim is a grid the batch touched before it:
            // the prefix [0, j_first] alone, one eviction, of the grid least
            // recently used at its last point (new grids included)
            consumed = (int64_t)j_first + 1;
            P.n_src = consumed;
            HIP_TRY(hipMemsetAsync(v.ctr, 0, 5 * sizeof(unsigned long long), c->stream));
            rc = launch_ivox_insert(P, c->stream);
            if (rc) return rc;
            HIP_TRY(hipMemsetAsync(v.ctr + 4, 0xFF, sizeof(unsigned long long), c->stream));
            rc = launch_ivox_tcur_min(P, c->stream);
            if (!rc) rc = launch_ivox_mark_min(P, c->stream);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(ctr, v.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            ev = 1;
        }
    }
    const int64_t N_new_b = (int64_t)ctr[1];
    // new CSR buffer
    const int other = 1 - v.cur;
    const int64_t need = v.npts + consumed + 3;
    if (v.pts_cap[other] < need) {
        dev_free(v.pts[other]);
        v.pts_cap[other] = 0;
        const int64_t cap = std::max<int64_t>(need + need / 2, 1 << 16);
        if (dev_alloc(&v.pts[other], (size_t)cap * 4)) return LIVO_E_OOM;
        v.pts_cap[other] = cap;
        P.npts = v.pts[other];
    }
    rc = launch_ivox_prepare(P, c->stream);
    if (!rc) rc = scan_u32(c, v.tot, v.newstart, v.table);
    if (!rc) rc = scan_u32(c, v.addcnt, v.addstart, v.table);
    if (!rc) {
        int bits = 1;
        while (((int64_t)1 << bits) <= v.table) bits++;  // the out-of-range key `table` included
        rc = sort_u32(c, v.slot_of, v.skeys, v.iota, v.svals, consumed, bits);
    }
    if (!rc) rc = launch_ivox_move(P, c->stream);
    if (!rc) rc = launch_ivox_place(P, c->stream);
    if (!rc) rc = launch_ivox_fix(P, c->stream);
    if (!rc) rc = launch_ivox_commit(P, c->stream);
    if (!rc && ev > 0) rc = launch_ivox_drop(P, c->stream);
    if (rc) return rc;
    // the number of points the evicted grids held leaves the map
    ScanCount npts_new;
    RC_TRY(npts_new.read(v.newstart, v.tot, v.table, c->stream));
    HIP_TRY(hipMemcpyAsync(ctr, v.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.cur = other;
    v.npts = npts_new.sum();
    v.ngrids += N_new_b - ev;
    v.next_id += consumed;
    v.max_grid = (int64_t)ctr[2];
    if (ev > 0) {
        rc = ivox_rehash_to(c, v.log2);  // evicted slots leave holes in the probe chains
        if (rc) return rc;
    }
    *done = consumed;
    v.add_passes++;
    return LIVO_OK;
}

static int ivox_add_dev(livo_ctx* c, int64_t n) {
    IvoxDev& v = c->iv;
    int64_t off = 0;
    while (off < n) {
        int64_t done = 0;
        const int rc = ivox_add_part(c, off, n - off, &done);
        if (rc) return rc;
        off += done;
    }
    (void)v;
    const int rc = ivox_trim_table(c);
    return rc ? rc : ivox_ensure_big(c);
}

static bool map_ready(const livo_ctx* c) {
    return c->backend == LIVO_BACKEND_IVOX ? c->iv.ready : c->has_map;
}

// The search of one evaluation with the context's backend (+ its exact /
// overflow pass); `later`: an evaluation after the first (seeded / gated).
static int backend_knn(livo_ctx* c, const KnnParams& kp, int n_jobs, int64_t max_n, bool later, hipStream_t st) {
    if (c->backend == LIVO_BACKEND_IVOX) return launch_ivox_knn(kp, n_jobs, max_n, later, c->iv.big_threads, st);
    return c->knn_kind >= 1 ? launch_knn_grid(kp, n_jobs, max_n, later, c->knn_kind == 2, st)
                            : launch_knn_leaf(kp, n_jobs, max_n, later, st);
}

// ---------------------------------------------- ikd-Tree incremental map --
extern "C" {
static ScanBuf* get_scan(livo_ctx* c, int32_t id);
static ScanBuf* get_scan_q(livo_ctx* c, int32_t id);
}
static int build_cell_runs(livo_ctx* c, int64_t M);
static int build_ball_runs(livo_ctx* c, int64_t M, float r5, double ext);
static int build_cell_runs_into(livo_ctx* c, const float* pts, int64_t M, GridSlot** slots, uint32_t** idx,
                                int32_t* log2, int64_t* words);
static void dyn_free(DynDev& d) {
    dev_free(d.all); dev_free(d.alive);
    dev_free(d.keys); dev_free(d.skeys); dev_free(d.iota); dev_free(d.svals);
    dev_free(d.heads); dev_free(d.runid); dev_free(d.starts);
    dev_free(d.add_buf);
    dev_free(d.boxes); dev_free(d.ctr);  // (d.dirty lives in d.ctr's allocation)
    dev_free(d.rpts); dev_free(d.rpos); dev_free(d.dslots); dev_free(d.dpts);
    dev_free(d.dvslots); dev_free(d.dvidx); dev_free(d.gpts_alt);
    dev_free(d.scan.ticket); dev_free(d.scan.status);
    d = DynDev{};
}

static int dyn_grow(livo_ctx* c, int64_t need) {  // id capacity
    DynDev& d = c->dyn;
    if (need <= d.cap) return LIVO_OK;
    if (need > kMaxMapPoints) return LIVO_E_RANGE;
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(need + (need >> 1), 1 << 16), kMaxMapPoints);
    float* a = nullptr;
    uint8_t* l = nullptr;
    if (dev_alloc(&a, (size_t)cap * 4) || dev_alloc(&l, (size_t)cap)) {
        dev_free(a);
        dev_free(l);
        return LIVO_E_OOM;
    }
    HIP_TRY(hipMemsetAsync(l, 0, (size_t)cap, c->stream));
    if (d.n_ids > 0) {
        HIP_TRY(hipMemcpyAsync(a, d.all, (size_t)d.n_ids * 16, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(l, d.alive, (size_t)d.n_ids, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    dev_free(d.all);
    dev_free(d.alive);
    d.all = a;
    d.alive = l;
    d.cap = cap;
    return LIVO_OK;
}

static int dyn_sort_scratch(livo_ctx* c, int64_t n) {
    DynDev& d = c->dyn;
    if (n <= d.sort_cap) return LIVO_OK;
    const int64_t cap = std::max<int64_t>(n + (n >> 2), 4096);
    dev_free(d.keys); dev_free(d.skeys); dev_free(d.iota); dev_free(d.svals);
    dev_free(d.heads); dev_free(d.runid); dev_free(d.starts);
    d.sort_cap = 0;
    if (dev_alloc(&d.keys, cap) || dev_alloc(&d.skeys, cap) || dev_alloc(&d.iota, cap) || dev_alloc(&d.svals, cap) ||
        dev_alloc(&d.heads, cap) || dev_alloc(&d.runid, cap) || dev_alloc(&d.starts, cap + 1))
        return LIVO_E_OOM;
    d.sort_cap = cap;
    return LIVO_OK;
}

static int dyn_add_scratch(livo_ctx* c, int64_t n) {
    DynDev& d = c->dyn;
    if (n <= d.add_cap) return LIVO_OK;
    const size_t cap = (size_t)std::max<int64_t>(n + (n >> 2), 4096);
    d.add_cap = 0;
    auto layout = [&](Carve k) {
        d.W = k.take<float>(cap * 4);
        d.seq = k.take<float>(cap * 4);
        d.Ws = k.take<float>(cap * 4);
        d.defer = k.take<uint32_t>(cap);
        d.dpos = k.take<uint32_t>(cap);
        d.dlist = k.take<uint32_t>(cap);
        d.keep = k.take<uint32_t>(cap);
        d.apos = k.take<uint32_t>(cap);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&d.add_buf, &d.add_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)d.add_buf});
    d.add_cap = (int64_t)cap;
    return LIVO_OK;
}

// The one-launch scans' state for up to n values (status words cleared once;
// every call tags its own with a new epoch).
static int dyn_scan_ready(livo_ctx* c, int64_t n) {
    ScanCtx& sc = c->dyn.scan;
    sc.err = c->dyn.ctr + kDynError;
    if (!sc.ticket) {
        if (dev_alloc(&sc.ticket, 1)) return LIVO_E_OOM;
        HIP_TRY(hipMemsetAsync(sc.ticket, 0, 8, c->stream));
        sc.issued = 0;
    }
    const int64_t tiles = scan_tiles(n + 1) + 1;
    if (sc.status_cap < tiles) {
        const int64_t cap = tiles + (tiles >> 1) + 64;
        dev_free(sc.status);
        sc.status_cap = 0;
        if (dev_alloc(&sc.status, (size_t)cap)) return LIVO_E_OOM;
        HIP_TRY(hipMemsetAsync(sc.status, 0, (size_t)cap * 8, c->stream));
        sc.status_cap = cap;
    }
    return LIVO_OK;
}

// The runs' base point set = the current cell grid (c->gpts, c->map_points
// points in grid order; the runs were built on it): rpts a copy of it (the
// grid itself is rebuilt by every change), rpos the position of each id,
// ids below n_ids the base, no deletion marks, an empty delta.
static int dyn_base_from_grid(livo_ctx* c) {
    DynDev& d = c->dyn;
    d.runs = false;
    const int64_t na = c->map_points;
    if (d.rpts_cap < na + 3) {
        dev_free(d.rpts);
        d.rpts_cap = 0;
        const int64_t cap = (na + 3) + ((na + 3) >> 3);
        if (dev_alloc(&d.rpts, (size_t)cap * 4)) return LIVO_E_OOM;
        d.rpts_cap = cap;
    }
    if (d.rpos_cap < d.n_ids) {
        dev_free(d.rpos);
        d.rpos_cap = 0;
        const int64_t cap = std::max<int64_t>(d.n_ids + (d.n_ids >> 3), 1);
        if (dev_alloc(&d.rpos, (size_t)cap)) return LIVO_E_OOM;
        d.rpos_cap = cap;
    }
    HIP_TRY(hipMemcpyAsync(d.rpts, c->gpts, (size_t)(na + 3) * 16, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d.rpos, 0xFF, (size_t)std::max<int64_t>(d.n_ids, 1) * 4, c->stream));
    int rc = launch_dyn_rpos(d.rpts, na, d.rpos, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    d.base_ids = d.n_ids;
    d.base_n = na;
    d.tomb = 0;
    d.d_n = 0;
    d.runs = true;
    return LIVO_OK;
}

// The runs rebuilt from the current points (the grid just rebuilt by
// dyn_rebuild): cell runs, ball runs with the build's r5, then the new base.
static int dyn_rebase(livo_ctx* c) {
    DynDev& d = c->dyn;
    d.runs = false;
    const int64_t na = c->map_points;
    const bool balls = c->bslots != nullptr && c->br5 > 0.f;
    int rc = na > 0 && na * 27 + kRunPad < (int64_t)0xFFFFFFFFll ? build_cell_runs(c, na) : LIVO_E_RANGE;
    if (!rc && balls) {
        const int brc = build_ball_runs(c, na, c->br5, 2.0 * (double)d.cmax);
        if (brc == LIVO_E_OOM) {
            (void)hipGetLastError();
            dev_free(c->bslots);
            dev_free(c->bpts);
            c->bentries = 0;
        } else if (brc) {
            rc = brc;
        }
    }
    if (!rc) rc = dyn_base_from_grid(c);
    if (rc == LIVO_E_OOM || rc == LIVO_E_RANGE) {  // the cell walk serves the map from here on
        (void)hipGetLastError();
        dev_free(c->vslots);
        dev_free(c->vpts);
        dev_free(c->bslots);
        dev_free(c->bpts);
        c->bentries = 0;
        d.runs = false;
        return LIVO_OK;
    }
    if (!rc) d.rebases++;
    return rc;
}

// After every change of the incremental map (dyn_rebuild): mark the base points
// deleted since, count the delta, rebase when it or the marks outgrow the
// base, else build the delta grid of the points added since the base.
static int dyn_runs_update(livo_ctx* c) {
    DynDev& d = c->dyn;
    if (!d.runs) return LIVO_OK;
    HIP_TRY(hipMemsetAsync(d.ctr + kDynTomb, 0, 2 * sizeof(unsigned long long), c->stream));
    int rc = launch_dyn_tomb(d.rpts, d.rpos, d.alive, d.base_ids, d.ctr, c->stream);
    const int64_t nd_ids = d.n_ids - d.base_ids;
    if (!rc && nd_ids > 0) rc = launch_count_alive(d.alive + d.base_ids, nd_ids, d.ctr, c->stream);
    if (rc) return rc;
    unsigned long long h[2];
    HIP_TRY(hipMemcpyAsync(h, d.ctr + kDynTomb, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    d.tomb += (int64_t)h[0];
    const int64_t nd = (int64_t)h[1];
    if ((double)nd > d.rebase_frac * (double)d.base_n || (double)d.tomb > 2.0 * d.rebase_frac * (double)d.base_n)
        return dyn_rebase(c);
    d.d_n = nd;
    if (nd == 0) return LIVO_OK;
    // the delta grid: cell keys of the ids since the base, sorted, gathered (k_dyn_gather pads 3)
    rc = launch_dyn_cellkeys(d.all + 4 * d.base_ids, d.alive + d.base_ids, nd_ids, c->gorg, 1.0f / c->gh, d.keys, d.iota,
                             d.ctr, c->stream);
    if (!rc) rc = sort_u64(c, d.keys, d.skeys, d.iota, d.svals, nd_ids);
    if (rc) return rc;
    if (d.dpts_cap < nd + 3) {
        dev_free(d.dpts);
        d.dpts_cap = 0;
        const int64_t cap = (nd + 3) + ((nd + 3) >> 1);
        if (dev_alloc(&d.dpts, (size_t)cap * 4)) return LIVO_E_OOM;
        d.dpts_cap = cap;
    }
    rc = launch_dyn_gather(d.skeys, d.svals, nd, d.all + 4 * d.base_ids, d.dpts, d.heads, c->stream);
    if (!rc) rc = scan_u32(c, d.heads, d.runid, nd);
    if (!rc) rc = launch_dyn_runs(d.heads, d.runid, nd, d.starts, d.ctr + kDynRuns, c->stream);
    if (rc) return rc;
    unsigned long long cells = 0;
    HIP_TRY(hipMemcpyAsync(&cells, d.ctr + kDynRuns, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int log2 = 4;
    while (((int64_t)1 << log2) < 4 * (int64_t)cells) log2++;
    const int64_t table = (int64_t)1 << log2;
    if (d.dslot_cap < table) {
        dev_free(d.dslots);
        d.dslot_cap = 0;
        if (dev_alloc(&d.dslots, (size_t)table)) return LIVO_E_OOM;
        d.dslot_cap = table;
    }
    rc = launch_ivox_clear(d.dslots, table, c->stream);
    if (!rc) rc = launch_dyn_slots(d.skeys, d.starts, (int64_t)cells, d.dslots, log2, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    d.dlog2 = log2;
    // and its cell runs: a query scans its cube's delta points in one run, as the base's
    int64_t words = 0;
    rc = build_cell_runs_into(c, d.dpts, nd, &d.dvslots, &d.dvidx, &d.dvlog2, &words);
    if (rc) {
        (void)hipGetLastError();
        dev_free(d.dvslots);
        dev_free(d.dvidx);
        return rc == LIVO_E_OOM || rc == LIVO_E_RANGE ? dyn_rebase(c) : rc;
    }
    return LIVO_OK;
}

static int dyn_rebuild(livo_ctx* c);

// The built map becomes the incremental point set (ids = build indices).
static int dyn_activate(livo_ctx* c) {
    DynDev& d = c->dyn;
    if (d.active) return LIVO_OK;
    if (!c->has_map) return LIVO_E_NOMAP;
    if (c->knn_kind == 0) return LIVO_E_INVALID;  // kept on the cell grid (not LIVO_KNN_KIND=leaf)
    if (int frc = fill_all_nn_coords(c)) return frc;  // (the grid the records' keys index is about to change)
    if (!d.ctr) {
        if (dev_alloc(&d.ctr, kDynCtrPad + kDynDirtyCap)) return LIVO_E_OOM;
        d.dirty = d.ctr + kDynCtrPad;  // (one allocation: dyn_add clears both with one memset)
    }
    const int64_t M = c->map_points;
    d.n_ids = d.n_alive = 0;
    int rc = dyn_grow(c, M + 1);
    if (rc) return rc;
    if (M == 0) {  // an empty build chose its cell from nothing: use 0.4 m cells at the origin
        c->gh = 0.4f;
        c->gorg[0] = c->gorg[1] = c->gorg[2] = 0.f;
    }
    rc = launch_dyn_seed(c->gpts, M, d.all, d.alive, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    d.n_ids = d.n_alive = M;
    d.cmax = c->gcmax;
    d.gslot_cap = (int64_t)1 << c->glog2;
    d.gpts_cap = M + 3;
    d.active = true;
    d.runs = false;
    d.d_n = 0;
    d.grid_ids = -1;  // (the build's grid: the first rebuild sorts)
    if (const char* env = std::getenv("LIVO_DYN_MERGE")) d.merge = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_DYN_BOX_CELL_MAX")) {  // tuning knob (0: off)
        const double v = std::atof(env);
        if (v >= 0.0 && v < 100.0) d.box_cell_max = (float)v;
    }
    if (const char* env = std::getenv("LIVO_DYN_BOX_CELL")) {  // tuning knob (0: off)
        const double v = std::atof(env);
        if (v >= 0.0 && v < 100.0) d.box_cell = (float)v;
    }
    if (const char* env = std::getenv("LIVO_DYN_REBASE")) {
        const double v = std::atof(env);
        if (v > 0.0 && v < 100.0) d.rebase_frac = v;
    }
    // The runs on the incremental map are opt-in (LIVO_DYN_RUNS=1): they take the
    // IEKF from 0.253 to 0.215 ms per scan on a map the scans built, but keeping
    // them (marks, delta grid and runs, rebases) takes Add_Points from 0.56 to
    // 1.34 ms, so the odometry loop runs at half the rate.
    const char* env_runs = std::getenv("LIVO_DYN_RUNS");
    if (c->vslots && c->vpts && M > 0 && env_runs && std::atoi(env_runs) == 1) {
        rc = dyn_base_from_grid(c);  // the built map's runs index its grid: the grid becomes the base
        if (rc == LIVO_E_OOM) {
            (void)hipGetLastError();
            rc = LIVO_OK;  // (the cell walk then serves the incremental map, as without runs)
        }
        if (rc) return rc;
    }
    return LIVO_OK;
}

constexpr int kMergeRetry = -1000;  // dyn_rebuild_merge: the counts disagree, sort instead
static int dyn_rebuild_merge(livo_ctx* c);

// The cell grid of k_knn_grid rebuilt from the alive points (same layout as
// build_grid_map: cells in key order, a cell's points in id order).
static int dyn_rebuild(livo_ctx* c) {
    DynDev& d = c->dyn;
    if (!d.runs && (c->gh < d.min_gh || (d.max_gh > 0.f && c->gh > d.max_gh))) {
        const float lo = (float)(2.0 * (double)d.cmax / (double)(kGridBias - 2));
        const float h = c->gh < d.min_gh ? d.min_gh : std::max(d.max_gh, d.min_gh);
        c->gh = std::max(h, lo * 1.01f);
    }
    if (d.merge && d.grid_ids >= 0 && d.cells >= 0 && d.grid_gh == c->gh && d.grid_ids <= d.n_ids) {
        const int rc = dyn_rebuild_merge(c);
        if (rc != kMergeRetry) return rc;
        (void)hipGetLastError();  // (the merge found an inconsistency: sort instead)
    }
    int rc = dyn_sort_scratch(c, std::max<int64_t>(d.n_ids, 1));
    if (rc) return rc;
    const int64_t na = d.n_alive;
    if (d.gpts_cap < na + 3) {
        const int64_t cap = (na + 3) + ((na + 3) >> 2);
        dev_free(c->gpts);
        if (dev_alloc(&c->gpts, (size_t)cap * 4)) return LIVO_E_OOM;
        d.gpts_cap = cap;
    }
    HIP_TRY(hipMemsetAsync(d.ctr, 0, kDynCtrN * sizeof(unsigned long long), c->stream));
    if (d.n_ids > 0) {
        rc = launch_dyn_cellkeys(d.all, d.alive, d.n_ids, c->gorg, 1.0f / c->gh, d.keys, d.iota, d.ctr, c->stream);
        if (!rc) rc = sort_u64(c, d.keys, d.skeys, d.iota, d.svals, d.n_ids);
    }
    if (!rc) rc = launch_dyn_gather(d.skeys, d.svals, na, d.all, c->gpts, d.heads, c->stream);
    if (!rc && na > 0) rc = scan_u32(c, d.heads, d.runid, na);
    if (!rc && na > 0) rc = launch_dyn_runs(d.heads, d.runid, na, d.starts, d.ctr + kDynRuns, c->stream);
    if (rc) return rc;
    unsigned long long h[kDynCtrN];
    HIP_TRY(hipMemcpyAsync(h, d.ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[kDynError]) return LIVO_E_RANGE;
    const int64_t cells = (int64_t)h[kDynRuns];
    int log2 = 4;
    while (((int64_t)1 << log2) < 4 * cells) log2++;  // load factor <= 1/4, as build_grid_map
    const int64_t table = (int64_t)1 << log2;
    if (d.gslot_cap < table) {  // (twice: headroom for Add_Points' fused rebuild)
        dev_free(c->gslots);
        d.gslot_cap = 0;
        if (dev_alloc(&c->gslots, (size_t)(2 * table))) return LIVO_E_OOM;
        d.gslot_cap = 2 * table;
    }
    rc = launch_ivox_clear(c->gslots, table, c->stream);
    if (!rc) rc = launch_dyn_slots(d.skeys, d.starts, cells, c->gslots, log2, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->glog2 = log2;
    c->map_points = na;
    c->geps = (float)(32.0 * std::ldexp(1.0, -24) * (double)d.cmax + 1e-7);
    c->grid_bytes = table * (int64_t)sizeof(GridSlot) + d.gpts_cap * 16;
    for (auto& s : c->scans) s.searched = false;  // cached neighbours refer to the old map
    d.grid_ids = d.n_ids;
    d.grid_gh = c->gh;
    d.cells = cells;
    d.rebuilds_sorted++;
    return dyn_runs_update(c);
}

// The grid after a change without sorting the map again: the ids added since
// the last rebuild (a few hundred per scan) are keyed and sorted, the old
// grid's survivors are ranked by a scan, and k_dyn_merge places both (the
// same (key, id) order a sort gives, so the same grid bit for bit).  The hash
// table is sized for the old cell count + the new points (a bound: each new
// point opens at most one cell), so nothing is read back before it is filled;
// one read-back at the end.  kMergeRetry: inconsistent counts (the caller
// sorts instead).
static int dyn_rebuild_merge(livo_ctx* c) {
    DynDev& d = c->dyn;
    const int64_t na_old = c->map_points, na = d.n_alive, g0 = d.grid_ids, m = d.n_ids - g0;
    int rc = dyn_sort_scratch(c, std::max<int64_t>(std::max<int64_t>(na_old, na), m) + 1);
    if (rc) return rc;
    if (d.gpts_alt_cap < na + 3) {
        const int64_t cap = (na + 3) + ((na + 3) >> 2);
        dev_free(d.gpts_alt);
        d.gpts_alt_cap = 0;
        if (dev_alloc(&d.gpts_alt, (size_t)cap * 4)) return LIVO_E_OOM;
        d.gpts_alt_cap = cap;
    }
    const float inv = 1.0f / c->gh;
    HIP_TRY(hipMemsetAsync(d.ctr, 0, kDynCtrN * sizeof(unsigned long long), c->stream));
    if (m > 0 && m <= kNewSortMax) {  // (a scan's few hundred winners: one workgroup)
        rc = launch_dyn_newsort(d.all + 4 * g0, d.alive + g0, m, c->gorg, inv, d.skeys, d.svals, d.ctr, c->stream);
    } else if (m > 0) {
        rc = launch_dyn_cellkeys(d.all + 4 * g0, d.alive + g0, m, c->gorg, inv, d.keys, d.iota, d.ctr, c->stream);
        if (!rc) rc = sort_u64(c, d.keys, d.skeys, d.iota, d.svals, m);
    }
    if (!rc) rc = dyn_scan_ready(c, std::max(na_old, na) + 1);
    if (!rc) rc = launch_scan_flags(d.scan, c->gpts, na_old, d.alive, d.runid, c->stream);
    if (rc) return rc;
    DynMergeParams P{};
    P.gpts = c->gpts; P.na_old = na_old; P.rank = d.runid; P.alive = d.alive;
    P.nkeys = d.skeys; P.nidx = d.svals; P.m = m; P.g0 = g0; P.all = d.all;
    P.out = d.gpts_alt; P.okeys = d.keys; P.na = na;
    std::memcpy(P.org, c->gorg, sizeof(P.org));
    P.inv = inv; P.ctr = d.ctr;
    rc = launch_dyn_merge(P, c->stream);
    if (!rc && na > 0) rc = launch_scan_runs(d.scan, d.keys, na, d.starts, d.ctr + kDynRuns, c->stream);
    if (rc) return rc;
    const int64_t bound = std::max<int64_t>(std::min<int64_t>(na, d.cells + m), 1);
    int log2 = 4;
    while (((int64_t)1 << log2) < 4 * bound) log2++;  // load factor <= 1/4, as build_grid_map
    const int64_t table = (int64_t)1 << log2;
    if (d.gslot_cap < table) {  // (twice: the fused pass's bound, + kNewSortMax, fits the next calls)
        dev_free(c->gslots);
        d.gslot_cap = 0;
        if (dev_alloc(&c->gslots, (size_t)(2 * table))) return LIVO_E_OOM;
        d.gslot_cap = 2 * table;
    }
    rc = launch_ivox_clear(c->gslots, table, c->stream);
    if (!rc && na > 0) rc = launch_dyn_slots(d.keys, d.starts, bound, c->gslots, log2, c->stream, d.ctr + kDynRuns,
                                             d.ctr + kDynError);
    if (rc) return rc;
    unsigned long long h[kDynCtrN];
    HIP_TRY(hipMemcpyAsync(h, d.ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[kDynError] & 64ull) return LIVO_E_HIP;  // a scan's look-back gave up
    if (h[kDynError] & (8ull | 16ull)) return kMergeRetry;  // (c->gpts untouched: the sort rebuilds from it)
    if (h[kDynError]) return LIVO_E_RANGE;
    std::swap(c->gpts, d.gpts_alt);
    std::swap(d.gpts_cap, d.gpts_alt_cap);
    c->glog2 = log2;
    c->map_points = na;
    c->geps = (float)(32.0 * std::ldexp(1.0, -24) * (double)d.cmax + 1e-7);
    c->grid_bytes = table * (int64_t)sizeof(GridSlot) + d.gpts_cap * 16;
    for (auto& s : c->scans) s.searched = false;  // cached neighbours refer to the old map
    d.grid_ids = d.n_ids;
    d.cells = (int64_t)h[kDynRuns];
    d.rebuilds_merged++;
    return dyn_runs_update(c);
}

// Add_Points of the n points in d.W (filled by the caller).
// world: map_incremental's scan and state (k_add_prep transforms the points into d.W), or null (d.W filled)
struct DynWorldIn {
    const float* pts;
    const int32_t* perm;
    const livo_state* state;      // host, or
    const livo_state* dev_state;  // ... non-null: on the device (livo_lio_frame)
};
static int dyn_add(livo_ctx* c, int64_t n, float ds, bool downsample, livo_map_add_stats* out,
                   const DynWorldIn* world = nullptr) {
    DynDev& d = c->dyn;
    // Add_Points' downsampling leaves one point per box of edge ds where the
    // scans pass: the cell walk's grid (rebuilt after this change) takes cells
    // of [box_cell, box_cell_max] * ds = [0.6, 1.0] m for 0.5 m boxes, so a walk
    // through thinned regions probes a few cells, not a cube of near-empty ones
    // sized for a dense built map (IEKF 0.58 vs 0.78 ms per scan on the thinned
    // 1M map), and a map built from one sparse scan does not keep cells sized
    // for its first few thousand points (0.245 vs 0.272 ms, Add_Points 0.48 vs
    // 0.62 ms; profiles/r04_ab_dyn_box_cell.txt).  The runs, when kept, index
    // the built grid.
    if (downsample && ds > 0.f && !d.runs) {
        d.min_gh = std::max(d.min_gh, d.box_cell * ds);
        if (d.box_cell_max > 0.f) d.max_gh = std::max(d.max_gh, d.box_cell_max * ds);
    }
    livo_map_add_stats st{};
    if (n > 0) {
        if (d.n_ids + n > kMaxMapPoints || n > (int64_t)0x7FFFFFFF) return LIVO_E_RANGE;
        int rc = dyn_grow(c, d.n_ids + n);
        if (!rc) rc = dyn_sort_scratch(c, n + 1);
        if (rc) return rc;
        // The merged grid rebuild runs in the same stream pass with the counts on
        // the device (one read-back for both), when the grid covers every id, its
        // cell edge stays, and the kept points fit k_dyn_newsort's workgroup (else,
        // or on any flag, dyn_rebuild runs after the read-back as before).
        const bool gh_stays = !(c->gh < d.min_gh || (d.max_gh > 0.f && c->gh > d.max_gh));
        bool fused = downsample && d.merge && !d.runs && d.grid_ids == d.n_ids && d.cells >= 0 &&
                     d.grid_gh == c->gh && gh_stays;
        const int64_t na_old = c->map_points, g0 = d.n_ids, m_ub = std::min<int64_t>(n, kNewSortMax);
        const int64_t na_ub = na_old + m_ub, cell_bound = std::max<int64_t>(std::min(na_ub, d.cells + m_ub), 1);
        int log2 = 4;
        while (((int64_t)1 << log2) < 4 * cell_bound) log2++;  // load factor <= 1/4, as build_grid_map
        const int64_t table = (int64_t)1 << log2;
        if (fused) {
            rc = dyn_sort_scratch(c, std::max(n, na_ub) + 1);
            if (!rc) rc = dyn_scan_ready(c, std::max(n, na_ub) + 1);
            if (!rc && d.gpts_alt_cap < na_ub + 3) {
                const int64_t cap = (na_ub + 3) + ((na_ub + 3) >> 2);
                dev_free(d.gpts_alt);
                d.gpts_alt_cap = 0;
                if (dev_alloc(&d.gpts_alt, (size_t)cap * 4)) rc = LIVO_E_OOM;
                else d.gpts_alt_cap = cap;
            }
            if (rc) return rc;
            // the add reads the current table: a table that must grow takes the
            // separate rebuild this time (which leaves headroom for the next)
            if (d.gslot_cap < table) fused = false;
        }
        // The box keys sort as 30-bit keys (10 bits per axis, wrapped): k_scan_boxes
        // finds two boxes sharing a wrapped key and the batch is redone with the
        // 64-bit keys (ctr bit 32: nothing changed).  LIVO_DYN_WIDE_KEYS=1: always 64-bit.
        static const bool wide_env = [] {
            const char* e = std::getenv("LIVO_DYN_WIDE_KEYS");
            return e && std::atoi(e) == 1;
        }();
        unsigned long long h[kDynCtrN];
        for (bool wide = wide_env;; wide = true) {
            HIP_TRY(hipMemsetAsync(d.ctr, 0, (kDynCtrPad + kDynDirtyCap) * sizeof(unsigned long long), c->stream));
            DynAddParams P{};
            P.W = d.W; P.n = n; P.ds = ds; P.downsample = downsample ? 1 : 0;
            P.gslots = c->gslots; P.gpts = c->gpts; P.glog2 = c->glog2;
            std::memcpy(P.gorg, c->gorg, sizeof(P.gorg));
            P.gh = c->gh; P.ginv = 1.0f / c->gh; P.geps = c->geps;
            P.base = d.n_ids; P.alive = d.alive;
            P.keys = d.keys; P.iota = d.iota; P.skeys = d.skeys; P.svals = d.svals; P.Ws = d.Ws;
            P.heads = d.heads; P.runid = d.runid; P.starts = d.starts;
            P.defer = d.defer; P.dpos = d.dpos; P.dlist = d.dlist; P.keep = d.keep; P.seq = d.seq;
            P.dirty = d.dirty; P.dirty_cap = kDynDirtyCap; P.ctr = d.ctr;
            if (world) {
                P.wpts = world->pts; P.wperm = world->perm;
                static_assert(offsetof(livo_state, rot) == 0 && offsetof(livo_state, pos) == 9 * sizeof(double),
                              "rot[9], pos[3] lead the state");
                if (world->dev_state) {
                    P.wdev = reinterpret_cast<const double*>(world->dev_state);
                } else {
                    std::memcpy(P.wrot, world->state->rot, sizeof(P.wrot));
                    std::memcpy(P.wpos, world->state->pos, sizeof(P.wpos));
                }
                std::memcpy(P.R_LI, c->params.R_LI, sizeof(P.R_LI));
                std::memcpy(P.t_LI, c->params.t_LI, sizeof(P.t_LI));
            }
            P.bigs = d.dlist;  // (dlist is free from the sort until k_add_finish)
            P.dlist_u = d.dpos; P.klist = d.apos;  // (dpos: free once k_scan_boxes has read the sorted keys)
            if (downsample && !wide) {  // (dlist / dpos are free until k_add_box)
                P.keys32 = d.dlist; P.skeys32 = d.dpos; P.skeys_w = d.skeys;
            }
            // k_add_prep refuses an out-of-range batch (ctr[kDynError] bit 0): the
            // passes that change the map (k_add_box, k_add_seq, k_add_append) then
            // do nothing, so the one read-back at the end decides
            rc = launch_add_prep(P, c->stream);
            if (rc) return rc;
            if (downsample) {
                if (P.keys32) rc = sort_u32(c, P.keys32, P.skeys32, d.iota, d.svals, n, 30);
                else rc = sort_u64(c, d.keys, d.skeys, d.iota, d.svals, n);
                if (!rc) rc = dyn_scan_ready(c, n);
                if (!rc) rc = launch_scan_boxes(d.scan, P, c->stream);
                if (!rc) rc = launch_add_group(P, c->stream);
            }
            if (!rc) rc = launch_add_finish(P, d.all, d.alive, c->stream);
            if (!rc && fused) {  // the merged rebuild on the device counts (kDynR*: its flags, runs, size)
                unsigned long long* rctr = d.ctr + (kDynRErr - kDynError);  // (rctr + kDynError = ctr + kDynRErr)
                const float inv = 1.0f / c->gh;
                rc = launch_dyn_newsort(d.all + 4 * g0, d.alive + g0, m_ub, c->gorg, inv, d.skeys, d.svals, rctr,
                                        c->stream, d.ctr + kDynAdded, d.ctr + kDynRErr);
                if (!rc) rc = launch_scan_flags(d.scan, c->gpts, na_old, d.alive, d.runid, c->stream, c->gslots, table);
                DynMergeParams M{};
                M.gpts = c->gpts; M.na_old = na_old; M.rank = d.runid; M.alive = d.alive;
                M.nkeys = d.skeys; M.nidx = d.svals; M.m = m_ub; M.g0 = g0; M.all = d.all;
                M.out = d.gpts_alt; M.okeys = d.keys; M.na = na_ub;
                std::memcpy(M.org, c->gorg, sizeof(M.org));
                M.inv = inv; M.ctr = rctr;
                M.dm = d.ctr + kDynAdded; M.dna = d.ctr + kDynRNa;
                if (!rc) rc = launch_dyn_merge(M, c->stream);
                if (!rc) rc = launch_scan_runs(d.scan, d.keys, na_ub, d.starts, d.ctr + kDynRRuns, c->stream,
                                               d.ctr + kDynRNa);
                if (!rc) rc = launch_dyn_slots(d.keys, d.starts, cell_bound, c->gslots, log2, c->stream,
                                               d.ctr + kDynRRuns, d.ctr + kDynRErr);
            }
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(h, d.ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (fused && (h[kDynError] & (1ull | 32ull | 64ull))) {
                // the fused pass refilled the table from an unchanged point set, hashed
                // with its bound's log2 (not c->glog2): rebuild it as the grid's own
                // before returning or before the 64-bit-key redo reads it (bit 32)
                const int rrc = dyn_rebuild(c);
                if (rrc) return rrc;
            }
            if (h[kDynError] & 1ull) return LIVO_E_RANGE;  // nothing changed
            if (h[kDynError] & 64ull) return LIVO_E_HIP;   // a scan's look-back gave up (nothing changed)
            if (!(h[kDynError] & 32ull) || wide) break;
            d.wide_redos++;
        }
        // k_add_prep checked the range of every box the later passes read, so
        // the group / sequential passes cannot fail once the map is modified
        if (h[kDynError]) {
            if (fused) (void)dyn_rebuild(c);
            return LIVO_E_HIP;
        }
        const int64_t added = (int64_t)h[kDynAdded];
        st.events = (int64_t)h[kDynEvents];
        st.deleted = (int64_t)h[kDynDeleted];
        st.ambiguous = (int64_t)h[kDynAmbig];
        st.deferred = downsample ? (int64_t)h[kDynDeferred] : 0;
        st.added = added;
        d.n_ids += added;
        d.n_alive += added - st.deleted;
        const uint32_t am = (uint32_t)h[kDynAbsMax];
        float amf;
        std::memcpy(&amf, &am, 4);
        d.cmax = std::max(d.cmax, amf);
        if (fused && h[kDynRErr] == 0 && (int64_t)h[kDynRNa] == d.n_alive && d.n_ids - g0 <= m_ub) {
            std::swap(c->gpts, d.gpts_alt);
            std::swap(d.gpts_cap, d.gpts_alt_cap);
            c->glog2 = log2;
            c->map_points = d.n_alive;
            c->geps = (float)(32.0 * std::ldexp(1.0, -24) * (double)d.cmax + 1e-7);
            c->grid_bytes = table * (int64_t)sizeof(GridSlot) + d.gpts_cap * 16;
            for (auto& sc : c->scans) sc.searched = false;  // cached neighbours refer to the old map
            d.grid_ids = d.n_ids;
            d.cells = (int64_t)h[kDynRRuns];
            d.rebuilds_merged++;
            d.rebuilds_fused++;
            rc = dyn_runs_update(c);
        } else {
            rc = dyn_rebuild(c);  // (c->gpts untouched by the fused pass)
        }
        if (rc) return rc;
    }
    st.map_points = d.n_alive;
    d.last = st;
    if (out) *out = st;
    return LIVO_OK;
}

// map_incremental with USE_ikdtree (laser_mapping.cpp:343-345, 383-384): every
// point to the world frame at the state, then Add_Points(feats_down_world, true)
// with downsample_size = filter_size_map_min (set_downsample_param, :138).
static int map_incremental_ikd(livo_ctx* c, int32_t id, const livo_state* state, const livo_state* dev_state, double fs,
                               uint8_t* cat, int64_t counts[2]) {
    if (!c->has_map) return LIVO_E_NOMAP;
    ScanBuf* s = get_scan(c, id);
    if (!s) return LIVO_E_NOSCAN;
    if (set_device(c)) return LIVO_E_HIP;
    const int64_t N = s->n;
    if (counts) counts[0] = counts[1] = 0;
    // (this path reads no neighbour record; dyn_activate fills every hot-only one before the grid changes)
    int rc = dyn_activate(c);
    if (!rc) rc = dyn_add_scratch(c, std::max<int64_t>(N, 1));
    if (rc) return rc;
    // (feats_down_world: k_add_prep takes the points to the world frame, the state in its arguments)
    const DynWorldIn world{s->pts, s->d_perm, state, dev_state};
    livo_map_add_stats st{};
    rc = dyn_add(c, N, (float)fs, true, &st, &world);
    if (rc) return rc;
    if (cat && N > 0) std::memset(cat, 1, (size_t)N);  // every point is handed to Add_Points
    if (counts) {
        counts[0] = st.events;
        counts[1] = st.deleted;
    }
    return LIVO_OK;
}

extern "C" {

int livo_abi_version(void) { return LIVO_ABI_VERSION; }

const char* livo_error_string(int code) {
    switch (code) {
        case LIVO_OK: return "ok";
        case LIVO_E_INVALID: return "invalid argument";
        case LIVO_E_HIP: return "HIP runtime error (no usable GPU or launch failure)";
        case LIVO_E_NOMAP: return "map not built";
        case LIVO_E_NOSCAN: return "unknown scan id";
        case LIVO_E_OOM: return "device allocation failed";
        case LIVO_E_RANGE: return "size out of supported range";
        case LIVO_E_CAPACITY: return "capacity exceeded";
        case LIVO_E_BUSY: return "batches in flight (collect them with livo_iekf_update_batch_wait first)";
        default: return "unknown error";
    }
}

int livo_params_default(livo_params* p) {
    if (!p) return LIVO_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->laser_point_cov = 0.001;
    p->R_LI[0] = p->R_LI[4] = p->R_LI[8] = 1.0;
    p->max_residual = 2.0;
    p->plane_threshold = 0.1f;
    p->max_nn_sqdist = 5.0f;
    p->max_iterations = 4;
    p->flags = 0;
    return LIVO_OK;
}

int livo_ctx_create(int device, const livo_params* p, livo_ctx** out) {
    if (!out) return LIVO_E_INVALID;
    *out = nullptr;
    livo_params def;
    livo_params_default(&def);
    if (p && !params_valid(p)) return LIVO_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return LIVO_E_HIP;
    if (device < 0 || device >= ndev) return LIVO_E_INVALID;
    livo_ctx* c = new (std::nothrow) livo_ctx();
    if (!c) return LIVO_E_OOM;
    c->device = device;
    c->params = p ? *p : def;
    if (const char* env = std::getenv("LIVO_STREAM_GROUPS")) {  // tuning knob
        const int v = std::atoi(env);
        if (v >= 1 && v <= kMaxGroups) c->groups = v;
    }
    if (const char* env = std::getenv("LIVO_LEAF_SIZE")) {  // tuning knob
        const int v = std::atoi(env);
        if (v >= 2 && v <= 256) c->leaf_size = v;
    }
    if (const char* env = std::getenv("LIVO_FUSED")) c->fused = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_KNN_KIND"))
        c->knn_kind = std::strcmp(env, "leaf") == 0 ? 0 : std::strcmp(env, "grid") == 0 ? 1 : 2;
    if (const char* env = std::getenv("LIVO_VRUNS")) c->vruns = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_BRUNS")) c->bruns = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_BR_HA")) {
        const float v = (float)std::atof(env);
        if (v > 0.2f && v < 20.f) c->br_ha = v;
    }
    if (const char* env = std::getenv("LIVO_BR_R")) {
        const float v = (float)std::atof(env);
        if (v > 0.5f && v < 20.f) c->br_r = v;
    }
    if (const char* env = std::getenv("LIVO_LANE_SERIAL")) c->lane_serial = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_SLOT_WB")) c->slot_wb = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_STAGE_COPY")) c->stage_copy = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_REC_COMPACT")) c->rec_compact = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_REC_LAZY")) c->rec_lazy = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_EVAL_GEN")) c->eval_gen = std::atoi(env) != 0;
    if (const char* env = std::getenv("LIVO_XCD_CHUNK")) c->xcd_chunk = std::max(0, std::atoi(env));  // tuning knob
    if (const char* env = std::getenv("LIVO_GRID_PPC")) {  // tuning knob
        const float v = (float)std::atof(env);
        if (v > 0.f) c->grid_ppc = v;
    }
    if (const char* env = std::getenv("LIVO_GRID_CELL")) {
        const float v = (float)std::atof(env);
        if (v > 0.f) c->grid_cell = v;
    }
    if (set_device(c) || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        create_group_streams(c)) {
        delete c;
        return LIVO_E_HIP;
    }
    *out = c;
    return LIVO_OK;
}

int livo_ctx_destroy(livo_ctx* c) {
    if (!c) return LIVO_E_INVALID;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (int k = 0; k < kMaxGroups - 1; k++)  // batches never collected: let them finish
        if (c->xstream[k]) (void)hipStreamSynchronize(c->xstream[k]);
    c->up.destroy();  // (waits for the uploads still queued)
    for (auto& s : c->scans) free_scan_buf(s);
    for (auto& s : c->spare) free_scan_buf(s);
    if (c->up_tmp) (void)hipFree(c->up_tmp);
    ivox_free(c->iv);
    dyn_free(c->dyn);
    if (c->fe_buf) (void)hipFree(c->fe_buf);
    if (c->wcloud.buf) (void)hipFree(c->wcloud.buf);
    if (c->ing.buf) (void)hipFree(c->ing.buf);
    if (c->stdb.buf) (void)hipFree(c->stdb.buf);
    if (c->stdb.stage) (void)hipFree(c->stdb.stage);
    if (c->stdb.mbuf) (void)hipFree(c->stdb.mbuf);
    if (c->sgen.key) (void)hipFree(c->sgen.key);
    for (void* b : c->sgen.buf)
        if (b) (void)hipFree(b);
    if (c->imu.st) (void)hipStreamSynchronize(c->imu.st);
    if (c->imu.buf) (void)hipFree(c->imu.buf);
    if (c->imu.table) (void)hipFree(c->imu.table);
    if (c->imu.pin) (void)hipHostFree(c->imu.pin);
    if (c->imu.st) (void)hipStreamDestroy(c->imu.st);
    if (c->prim_tmp) (void)hipFree(c->prim_tmp);
    if (c->vio_buf) (void)hipFree(c->vio_buf);
    dev_free(c->bgr_img.p);
    dev_free(c->gray_img.p);
    if (c->vis_buf) (void)hipFree(c->vis_buf);
    dev_free(c->match_img.p);
    if (c->vm_buf) (void)hipFree(c->vm_buf);
    dev_free(c->det_img.p);
    if (c->det_buf) (void)hipFree(c->det_buf);
    if (c->vmap.buf) (void)hipFree(c->vmap.buf);
    if (c->vmap.img) (void)hipFree(c->vmap.img);
    dev_free(c->nodes);
    dev_free(c->lnodes);
    dev_free(c->lpts);
    dev_free(c->gslots);
    dev_free(c->gpts);
    dev_free(c->vslots);
    dev_free(c->vpts);
    dev_free(c->bslots);
    dev_free(c->bpts);
    dev_free(c->d_replay_count);
    dev_free(c->d_replay_total);
    dev_free(c->d_replay_list);
    dev_free(c->d_replay_count2);
    dev_free(c->d_replay_list2);
    dev_free(c->d_slots);
    dev_free(c->d_jobs);
    if (c->h_slots) (void)hipHostFree(c->h_slots);
    if (c->h_jobs) (void)hipHostFree(c->h_jobs);
    for (BatchLane& B : c->lane) {
        for (Staging& s : B.stage) s.free();
        for (hipEvent_t e : B.done)
            if (e) (void)hipEventDestroy(e);
    }
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->rec_tmp) (void)hipFree(c->rec_tmp);
    if (c->events_ready) {
        for (auto& g : c->ev)
            for (auto& e : g) (void)hipEventDestroy(e);
        (void)hipEventDestroy(c->b_start);
        (void)hipEventDestroy(c->b_end[0]);
        (void)hipEventDestroy(c->b_end[1]);
    }
    for (int k = 0; k < kMaxGroups - 1; k++) {
        if (c->xstream[k]) (void)hipStreamSynchronize(c->xstream[k]);
        if (c->xjoin[k]) (void)hipEventDestroy(c->xjoin[k]);
        if (c->xstream[k]) (void)hipStreamDestroy(c->xstream[k]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return LIVO_OK;
}

int livo_ctx_set_params(livo_ctx* c, const livo_params* p) {
    if (!c || !params_valid(p)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    c->params = *p;
    return LIVO_OK;
}

int livo_ctx_set_profiling(livo_ctx* c, int enable) {
    if (!c) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (set_device(c)) return LIVO_E_HIP;
    if (enable && !c->events_ready) {
        for (auto& g : c->ev)
            for (auto& e : g) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventCreate(&c->b_start));
        HIP_TRY(hipEventCreate(&c->b_end[0]));
        HIP_TRY(hipEventCreate(&c->b_end[1]));
        c->events_ready = true;
    }
    c->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    c->b_prev = false;
    return LIVO_OK;
}

int livo_last_timings(livo_ctx* c, livo_timings* out) {
    if (!c || !out) return LIVO_E_INVALID;
    *out = c->last;
    return LIVO_OK;
}

// Index runs from n key-sorted entries (skeys; e2 / pt give each entry's grid
// position, as k_run_place): heads, run ids, run starts, lengths rounded up to
// 4, their exclusive scan (pstart) and the placed positions in *out (the
// padded total + kRunPad words, zero-filled), then the runs' hash slots
// (load factor <= 1/4).  plen / pstart: scratch of n + 1 words each.
static int build_index_runs(livo_ctx* c, int64_t n, const unsigned long long* skeys, const uint32_t* e2,
                            const uint32_t* pt, uint32_t* heads, uint32_t* runid, uint32_t* starts,
                            unsigned long long* nruns_dev, uint32_t* plen, uint32_t* pstart, uint32_t** out,
                            GridSlot** slots, int* log2_out, int64_t* words) {
    int rc = launch_run_heads(skeys, n, heads, c->stream);
    if (!rc) rc = scan_u32(c, heads, runid, n);
    if (!rc) rc = launch_dyn_runs(heads, runid, n, starts, nruns_dev, c->stream);
    unsigned long long runs = 0;
    if (!rc && hipMemcpyAsync(&runs, nruns_dev, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = LIVO_E_HIP;
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
    if (rc) return rc;
    if (runs == 0) return LIVO_E_INVALID;
    rc = launch_run_plen(starts, (int64_t)runs, plen, c->stream);
    if (!rc) rc = scan_u32(c, plen, pstart, (int64_t)runs);
    ScanCount padded;
    if (!rc) rc = padded.read(pstart, plen, (int64_t)runs, c->stream);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
    if (rc) return rc;
    const int64_t total = padded.sum();  // (u32 lengths: the scan wraps beyond 2^32 words)
    if (total < n || total + kRunPad >= (int64_t)0xFFFFFFFFll) return LIVO_E_RANGE;
    if (dev_alloc(out, (size_t)(total + kRunPad))) return LIVO_E_OOM;
    rc = hipMemsetAsync(*out, 0, (size_t)(total + kRunPad) * sizeof(uint32_t), c->stream) == hipSuccess ? LIVO_OK
                                                                                                         : LIVO_E_HIP;
    if (!rc) rc = launch_run_place(e2, pt, heads, runid, starts, pstart, n, *out, c->stream);
    int log2 = 4;
    while (((int64_t)1 << log2) < 4 * (int64_t)runs) log2++;
    const int64_t table = (int64_t)1 << log2;
    if (!rc && dev_alloc(slots, (size_t)table)) rc = LIVO_E_OOM;
    if (!rc) rc = launch_ivox_clear(*slots, table, c->stream);
    if (!rc) rc = launch_run_slots(skeys, starts, pstart, (int64_t)runs, *slots, log2, c->stream);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
    if (rc) {
        dev_free(*out);
        dev_free(*slots);
        return rc;
    }
    *log2_out = log2;
    *words = total + kRunPad;
    return LIVO_OK;
}

// The cell runs of the static map's grid (livo_internal.h), built on the
// device: two stable radix sorts (rho2, then the run key) of the 27 M entries,
// the runs' heads and starts, and their hash table (load factor <= 1/4).
static int build_cell_runs(livo_ctx* c, int64_t M) {
    int64_t words = 0;
    const int rc = build_cell_runs_into(c, c->gpts, M, &c->vslots, &c->vpts, &c->vlog2, &words);
    if (!rc && M > 0) c->grid_bytes += (int64_t)(((int64_t)1 << c->vlog2) * sizeof(GridSlot) + words * sizeof(uint32_t));
    return rc;
}
// The cell runs of M grid-ordered points pts (the map's grid; on the incremental
// map also its delta grid): *slots / *idx replaced, run entries = positions in pts.
static int build_cell_runs_into(livo_ctx* c, const float* pts, int64_t M, GridSlot** slots, uint32_t** idx,
                                int32_t* log2, int64_t* words) {
    dev_free(*slots);
    dev_free(*idx);
    if (M <= 0) return LIVO_OK;
    const int64_t n = M * 27;
    if (n + 8 >= (int64_t)kRunPosLimit) return LIVO_E_RANGE;  // 31-bit run positions (kRunPos)
    char* scr = nullptr;
    if (hipMalloc((void**)&scr, carve_bytes(run_build_layout, (size_t)n, false)) != hipSuccess) return LIVO_E_OOM;
    Carve k{scr};
    const RunBuild L = run_build_layout(k, (size_t)n, false);
    int rc = launch_cr_rho(pts, n, c->gorg, c->gh, L.rho, L.iota, c->stream);
    if (!rc) rc = sort_u32(c, L.rho, L.srho, L.iota, L.e1, n, 32);
    if (!rc) rc = launch_cr_key(pts, L.e1, n, c->gorg, c->gh, L.keys, c->stream);
    if (!rc) rc = sort_u64(c, L.keys, L.skeys, L.e1, L.e2, n);
    // the padded run lengths and their scan (in rho and iota, dead after the sorts)
    if (!rc) rc = build_index_runs(c, n, L.skeys, L.e2, nullptr, L.heads, L.runid, L.starts, L.nruns, L.plen, L.pstart,
                                   idx, slots, log2, words);
    (void)hipFree(scr);
    return rc;
}

// The index ball runs, built in chunks of anchors (their x index in [x0, x1)),
// each chunk at most `cap` entries (LIVO_BR_CHUNK, default 2^29: ~26 GB of sort
// scratch), so the 32-bit sort indices and offsets of one chunk never wrap
// however many entries the map has (config 5's 10M map with 6 r5 balls passes
// 2^31).  A chunk is counted, placed behind the runs of the chunks before it in
// one run array (every run starts on a 4-word boundary), and its runs recorded
// as {key, start / 4, count}; the hash table then takes every record, so a slot's
// start addresses 2^34 words.  The runs' contents and order do not depend on
// the chunking.
static int build_ball_runs_idx(livo_ctx* c, int64_t M, float r5, float bh, float brmax, double ext) {
    int64_t cap = (int64_t)1 << 29;
    if (const char* env = std::getenv("LIVO_BR_CHUNK")) cap = std::max<int64_t>(1 << 16, std::atoll(env));
    cap = std::min<int64_t>(cap, ((int64_t)1 << 31) - 64);
    uint32_t* cnt = nullptr;
    uint32_t* off = nullptr;
    unsigned long long* tot = nullptr;
    // an early return leaves nothing behind: the counts, their scan and the run array so far
    // (c->bpts is null on entry: build_ball_runs has freed it)
    auto fail = [&](int rc) {
        dev_free(cnt);
        dev_free(off);
        dev_free(tot);
        dev_free(c->bpts);
        return rc;
    };
    if (dev_alloc(&cnt, (size_t)M) || dev_alloc(&off, (size_t)M) || dev_alloc(&tot, 1)) return fail(LIVO_E_OOM);
    // entries of the anchors with x index in [x0, x1) (a count pass over the map)
    auto count = [&](int x0, int x1, unsigned long long* n_out) -> int {
        int rc = hipMemsetAsync(tot, 0, 8, c->stream) == hipSuccess ? LIVO_OK : LIVO_E_HIP;
        if (!rc) rc = launch_br_count(c->gpts, M, c->gorg, bh, brmax, cnt, tot, c->stream, x0, x1);
        if (!rc && hipMemcpyAsync(n_out, tot, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = LIVO_E_HIP;
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
        return rc;
    };
    // the anchors' x range: the map spans [gorg, gorg + ext] on every axis (the
    // grid's origin is its minimum corner), a point's anchors lie within brmax
    const int xlo = (int)std::floor(-(double)brmax / (double)bh) - 2;
    const int xhi = (int)std::floor((ext + (double)brmax) / (double)bh) + 3;  // exclusive
    struct Chunk {
        int x0, x1;
        int64_t n;
    };
    std::vector<Chunk> chunks, todo{{xlo, xhi, -1}};
    int64_t total_entries = 0, max_n = 0;
    int rc = LIVO_OK;
    while (!todo.empty() && !rc) {  // bisect the x range until every chunk fits
        Chunk ch = todo.back();
        todo.pop_back();
        unsigned long long n64 = 0;
        rc = count(ch.x0, ch.x1, &n64);
        if (rc) break;
        if ((int64_t)n64 > cap && ch.x1 - ch.x0 > 1) {
            const int mid = ch.x0 + (ch.x1 - ch.x0) / 2;
            todo.push_back({mid, ch.x1, -1});
            todo.push_back({ch.x0, mid, -1});
            continue;
        }
        if ((int64_t)n64 > cap) rc = LIVO_E_RANGE;  // one anchor column beyond the cap
        if (n64 == 0) continue;
        ch.n = (int64_t)n64;
        chunks.push_back(ch);
        total_entries += ch.n;
        max_n = std::max(max_n, ch.n);
    }
    dev_free(tot);
    if (rc || total_entries == 0) return fail(rc);
    // the run array: the entries plus the padding of every run to 4 words (grown if short)
    int64_t words_cap = total_entries + total_entries / 8 + 4096 + kRunPad;
    if (dev_alloc(&c->bpts, (size_t)words_cap) ||
        hipMemsetAsync(c->bpts, 0, (size_t)words_cap * sizeof(uint32_t), c->stream) != hipSuccess)
        return fail(LIVO_E_OOM);
    // one carve for the largest chunk, reused by every chunk
    char* scr = nullptr;
    if (hipMalloc((void**)&scr, carve_bytes(run_build_layout, (size_t)max_n, true)) != hipSuccess)
        return fail(LIVO_E_OOM);
    Carve k{scr};
    const RunBuild L = run_build_layout(k, (size_t)max_n, true);
    GridSlot* trip = nullptr;
    int64_t trip_cap = 0, runs_total = 0, base = 0;
    for (const Chunk& ch : chunks) {
        const int64_t nc = ch.n;
        rc = launch_br_count(c->gpts, M, c->gorg, bh, brmax, cnt, L.nruns, c->stream, ch.x0, ch.x1);
        if (!rc) rc = scan_u32(c, cnt, off, M);
        if (!rc)
            rc = launch_br_emit(c->gpts, M, c->gorg, bh, brmax, off, L.rho, L.keys, L.pt, L.iota, c->stream, ch.x0, ch.x1);
        if (!rc) rc = sort_u32(c, L.rho, L.srho, L.iota, L.e1, nc, 32);
        if (!rc) rc = launch_br_gather_keys(L.keys, L.e1, nc, L.key1, c->stream);
        if (!rc) rc = sort_u64(c, L.key1, L.skeys, L.e1, L.e2, nc);
        // runs: heads, starts, lengths padded to 4 and their scan (runid, pstart: in rho and
        // srho, dead after the first sort)
        if (!rc) rc = launch_run_heads(L.skeys, nc, L.heads, c->stream);
        if (!rc) rc = scan_u32(c, L.heads, L.runid, nc);
        if (!rc && hipMemsetAsync(L.nruns, 0, 8, c->stream) != hipSuccess) rc = LIVO_E_HIP;
        if (!rc) rc = launch_dyn_runs(L.heads, L.runid, nc, L.starts, L.nruns, c->stream);
        unsigned long long runs = 0;
        if (!rc && hipMemcpyAsync(&runs, L.nruns, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = LIVO_E_HIP;
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
        if (rc) break;
        if (runs == 0) continue;
        rc = launch_run_plen(L.starts, (int64_t)runs, L.plen, c->stream);
        if (!rc) rc = scan_u32(c, L.plen, L.pstart, (int64_t)runs);
        ScanCount padded;
        if (!rc) rc = padded.read(L.pstart, L.plen, (int64_t)runs, c->stream);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
        if (rc) break;
        const int64_t words = padded.sum();
        if (words < nc || words >= (int64_t)0xFFFFFFFFll) {
            rc = LIVO_E_RANGE;
            break;
        }
        if (base + words + kRunPad > words_cap) {  // more padding than reserved: grow the run array
            const int64_t ncap = (base + words + kRunPad) + (base + words) / 8;
            uint32_t* nb = nullptr;
            if (dev_alloc(&nb, (size_t)ncap)) {
                rc = LIVO_E_OOM;
                break;
            }
            if (hipMemsetAsync(nb, 0, (size_t)ncap * sizeof(uint32_t), c->stream) != hipSuccess ||
                hipMemcpyAsync(nb, c->bpts, (size_t)base * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream) !=
                    hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess)
                rc = LIVO_E_HIP;
            dev_free(c->bpts);
            c->bpts = nb;
            words_cap = ncap;
            if (rc) break;
        }
        if (runs_total + (int64_t)runs > trip_cap) {  // the run records (grown by doubling)
            const int64_t ncap = std::max<int64_t>(2 * trip_cap, runs_total + (int64_t)runs + 4096);
            GridSlot* nt = nullptr;
            if (dev_alloc(&nt, (size_t)ncap)) {
                rc = LIVO_E_OOM;
                break;
            }
            if (runs_total > 0 &&
                (hipMemcpyAsync(nt, trip, (size_t)runs_total * sizeof(GridSlot), hipMemcpyDeviceToDevice,
                                c->stream) != hipSuccess ||
                 hipStreamSynchronize(c->stream) != hipSuccess))
                rc = LIVO_E_HIP;
            dev_free(trip);
            trip = nt;
            trip_cap = ncap;
            if (rc) break;
        }
        rc = launch_run_place(L.e2, L.pt, L.heads, L.runid, L.starts, L.pstart, nc, c->bpts + base, c->stream);
        if (!rc) rc = launch_run_trip(L.skeys, L.starts, L.pstart, (int64_t)runs, (unsigned long long)base,
                                      trip + runs_total, c->stream);
        if (rc) break;
        base += words;
        runs_total += (int64_t)runs;
    }
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
    (void)hipFree(scr);
    dev_free(cnt);
    dev_free(off);
    if (!rc && (base >> 2) >= ((int64_t)1 << 32)) rc = LIVO_E_RANGE;  // start / 4 in 32 bits
    int log2 = 4;
    while (((int64_t)1 << log2) < 4 * runs_total) log2++;
    if (!rc && runs_total > 0) {
        const int64_t table = (int64_t)1 << log2;
        if (dev_alloc(&c->bslots, (size_t)table)) rc = LIVO_E_OOM;
        if (!rc) rc = launch_ivox_clear(c->bslots, table, c->stream);
        if (!rc) rc = launch_trip_slots(trip, runs_total, c->bslots, log2, c->stream);
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = LIVO_E_HIP;
    }
    dev_free(trip);
    if (rc || runs_total == 0) {
        dev_free(c->bslots);
        dev_free(c->bpts);
        return rc;
    }
    c->blog2 = log2;
    c->bh = bh;
    c->brmax = brmax;
    c->br5 = r5;
    c->bentries = total_entries;
    c->bchunks = (int32_t)chunks.size();
    c->grid_bytes += (int64_t)(((int64_t)1 << log2) * sizeof(GridSlot) + words_cap * sizeof(uint32_t));
    return LIVO_OK;
}

// The ball runs of the static map (livo_internal.h KnnParams::bslots), built on
// the device: every grid point emits one entry per anchor cell (edge bh) whose
// centre lies within brmax (k_br_count, a scan, k_br_emit); a stable radix sort
// by rho2, a gather of the anchor keys and a stable sort by key leave each
// anchor's run contiguous and sorted by rho2 (build_ball_runs_idx, chunk by
// chunk).  r5: the map's median 5-NN distance (sample_knn_radius).
static int build_ball_runs(livo_ctx* c, int64_t M, float r5, double ext) {
    dev_free(c->bslots);
    dev_free(c->bpts);
    c->bentries = 0;
    if (M <= 0 || !(r5 > 0.f)) return LIVO_OK;
    const float bh = std::max(c->br_ha * r5, 1e-3f);
    const float brmax = 0.8660254f * bh + c->br_r * r5;
    // anchor keys are 21-bit per axis (grid_key, kGridBias = 2^20) and the device
    // clamps a query's anchor to +-(kGridBias - 8): a map whose extent (+ the
    // ball radius) spans that many anchors keeps the cell runs only, rather
    // than letting keys alias into a run not sorted about its own anchor
    if ((ext + 2.0 * (double)brmax) / (double)bh + 4.0 >= (double)(kGridBias - 8)) return LIVO_OK;
    return build_ball_runs_idx(c, M, r5, bh, brmax, ext);
}

int livo_map_build(livo_ctx* c, const float* xyz, int64_t M, int64_t stride_bytes) {
    if (!c || M < 0 || (M > 0 && !xyz)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (set_device(c)) return LIVO_E_HIP;
    int rc = fill_all_nn_coords(c);  // (hot-only records' keys refer to the map being replaced)
    if (rc) return rc;
    HostMap hm;
    rc = build_host_map(xyz, M, stride_bytes, &hm);
    if (rc) return rc;
    HostLeafMap lm;
    HostGridMap gm;
    // (a map of more than ~79M points keeps the cell walk: run positions are 31-bit)
    const bool vr = c->knn_kind == 2 && c->vruns && M * 27 + 8 < (int64_t)kRunPosLimit;
    rc = c->knn_kind >= 1 ? build_grid_map(xyz, M, stride_bytes, c->grid_cell, &gm, c->grid_ppc > 0.f ? c->grid_ppc
                                                                                    : (vr ? -kVrunPpc : 0.f))
                          : build_leaf_map(xyz, M, stride_bytes, c->leaf_size, &lm);
    if (rc) {
        free_host_map(&hm);
        free_grid_map(&gm);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < kMaxGroups - 1; k++) HIP_TRY(hipStreamSynchronize(c->xstream[k]));
    dev_free(c->nodes);
    dev_free(c->lnodes);
    dev_free(c->lpts);
    dev_free(c->gslots);
    dev_free(c->gpts);
    dev_free(c->vslots);
    dev_free(c->vpts);
    dev_free(c->bslots);
    dev_free(c->bpts);
    c->nodes = nullptr;
    c->lnodes = nullptr;
    c->lpts = nullptr;
    c->gslots = nullptr;
    c->gpts = nullptr;
    c->leaf_bytes = c->grid_bytes = 0;
    c->has_map = false;
    c->dyn.active = false;  // a new static map (the incremental buffers are kept for reuse)
    c->dyn.min_gh = c->dyn.max_gh = 0.f;
    c->dyn.runs = false;
    c->dyn.d_n = 0;
    c->dyn.n_ids = c->dyn.n_alive = 0;
    c->dyn.last = livo_map_add_stats{};
    const size_t bytes = (size_t)(hm.num_slots + 1) * sizeof(MapNode);
    const size_t ppb = (size_t)(M + 3) * 4 * sizeof(float);  // chunk padding
    hipError_t e = hipSuccess;
    bool oom = hipMalloc((void**)&c->nodes, bytes) != hipSuccess;
    if (c->knn_kind >= 1) {
        const size_t gsb = ((size_t)1 << gm.log2_slots) * sizeof(GridSlot);
        oom = oom || hipMalloc((void**)&c->gslots, gsb) != hipSuccess || hipMalloc((void**)&c->gpts, ppb) != hipSuccess;
        if (!oom) e = hipMemcpy(c->gslots, gm.slots, gsb, hipMemcpyHostToDevice);
        if (!oom && e == hipSuccess) e = hipMemcpy(c->gpts, gm.pts, ppb, hipMemcpyHostToDevice);
        c->grid_bytes = (int64_t)(gsb + ppb);
        std::memcpy(c->gorg, gm.org, sizeof(c->gorg));
        c->gh = gm.h;
        c->glog2 = gm.log2_slots;
        // slack for float rounding in the cell assignment (host) and cell bounds (device)
        c->geps = (float)(32.0 * std::ldexp(1.0, -24) * (double)gm.cmax + 1e-7);
        c->gcmax = gm.cmax;
    } else {
        const size_t lnb = (size_t)std::max<int64_t>(((int64_t)1 << lm.depth) - 1, 1) * sizeof(LeafNode);
        oom = oom || hipMalloc((void**)&c->lnodes, lnb) != hipSuccess || hipMalloc((void**)&c->lpts, ppb) != hipSuccess;
        if (!oom) e = hipMemcpy(c->lnodes, lm.nodes, lnb, hipMemcpyHostToDevice);
        if (!oom && e == hipSuccess) e = hipMemcpy(c->lpts, lm.pts, ppb, hipMemcpyHostToDevice);
        c->leaf_depth = lm.depth;
        c->leaf_bytes = (int64_t)(lnb + ppb);
    }
    if (!oom && e == hipSuccess) e = hipMemcpy(c->nodes, hm.nodes, bytes, hipMemcpyHostToDevice);
    const float r5 = (vr && c->bruns && c->knn_kind >= 1) ? sample_knn_radius(gm, 8192) : 0.f;
    const double gext = gm.ext;
    free_host_map(&hm);
    free_leaf_map(&lm);
    free_grid_map(&gm);
    if (oom) return LIVO_E_OOM;
    if (e != hipSuccess) return LIVO_E_HIP;
    if (vr) {
        rc = build_cell_runs(c, M);
        if (rc) return rc;
        if (r5 > 0.f) {
            // the ball runs are a speed-up over the cell runs: a map they do not
            // fit (their scratch is ~68 B per entry, ~60 entries per point) keeps
            // the cell runs and builds; other errors still fail the build
            const int brc = build_ball_runs(c, M, r5, gext);
            if (brc == LIVO_E_OOM) {
                (void)hipGetLastError();
                dev_free(c->bslots);
                dev_free(c->bpts);
                c->bentries = 0;
            } else if (brc) {
                return brc;
            }
        }
    }
    c->map_points = M;
    c->map_slots = hm.num_slots;
    c->map_depth = hm.depth;
    c->has_map = true;
    for (auto& s : c->scans) s.searched = false;  // cached neighbours refer to the old map
    return LIVO_OK;
}

int livo_map_get_info(livo_ctx* c, livo_map_info* out) {
    if (!c || !out) return LIVO_E_INVALID;
    if (!c->has_map) return LIVO_E_NOMAP;
    out->num_points = c->map_points;
    out->depth = c->map_depth;
    out->ball_chunks = c->bslots ? c->bchunks : 0;
    out->ball_entries = c->bslots ? c->bentries : 0;
    out->num_slots = c->map_slots;
    out->device_bytes = (c->map_slots + 1) * (int64_t)sizeof(MapNode) + c->leaf_bytes + c->grid_bytes +
                        c->dyn.cap * 17;
    return LIVO_OK;
}

int livo_knn(livo_ctx* c, const float* q, int64_t n, int32_t k, int32_t* idx, float* d) {
    if (!c || n < 0 || k < 1 || k > kNN || (n > 0 && (!q || !idx || !d))) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (!c->has_map) return LIVO_E_NOMAP;
    if (n == 0) return LIVO_OK;
    if (n > (int64_t)0x7FFFFFFF - kBlock) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    int rc = ensure_slot(c);
    if (rc) return rc;
    const size_t qb = (size_t)n * 4 * sizeof(float), rb = (size_t)n * sizeof(NNRec);
    rc = ensure_scratch(c, carve_bytes(knn_query_layout<NNRec>, (size_t)n));
    if (rc) return rc;
    Carve cv{(char*)c->scratch};
    const KnnQuery<NNRec> Q = knn_query_layout<NNRec>(cv, (size_t)n);
    std::vector<float> hq((size_t)n * 4);
    for (int64_t i = 0; i < n; i++) {
        hq[4 * i] = q[3 * i]; hq[4 * i + 1] = q[3 * i + 1]; hq[4 * i + 2] = q[3 * i + 2]; hq[4 * i + 3] = 0.f;
    }
    IekfSlot zero{};
    std::memset(&zero, 0, sizeof(zero));
    c->h_slots[0] = zero;
    HsJob& j = c->h_jobs[0];
    j = HsJob{};
    j.pts = Q.q; j.nn = Q.rec; j.slot = c->d_slots; j.n = (int32_t)n; j.nblk = 0;
    HIP_TRY(hipMemcpyAsync(Q.q, hq.data(), qb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_slots, c->h_slots, sizeof(IekfSlot), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_jobs, c->h_jobs, sizeof(HsJob), hipMemcpyHostToDevice, c->stream));
    rc = ensure_replay(c, n);
    if (rc) return rc;
    KnnParams kp = make_knn_params(c);
    kp.force = 1;
    kp.identity = 1;
    rc = knn_pass(kp, 1, n, c->stream);
    if (rc) return rc;
    std::vector<NNRec> hr((size_t)n);
    HIP_TRY(hipMemcpyAsync(hr.data(), Q.rec, rb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; i++)
        for (int t = 0; t < k; t++) {
            idx[i * k + t] = rec_host_idx(hr[i], t);
            d[i * k + t] = rec_host_sqdist(hr[i], t);
        }
    return LIVO_OK;
}

static int32_t register_scan(livo_ctx* c, const ScanBuf& s) {
    int32_t id = -1;
    for (size_t i = 0; i < c->scans.size(); i++)
        if (!c->scans[i].used) { id = (int32_t)i; break; }
    if (id < 0) {
        id = (int32_t)c->scans.size();
        c->scans.push_back(s);
    } else {
        c->scans[id] = s;
    }
    return id;
}

// The device buffers of a scan of N points: a released scan's when one fits
// (capacity N .. 2N + 4096), else fresh allocations sized for N.
// Released scan buffers are kept for reuse up to a byte budget (LIVO_SPARE_MB,
// default 8192): a hipFree synchronises the whole device, so freeing one while
// a farm's batches and uploads are in flight stalled the pipeline (a 12.9 ms
// upload call; the farm with uploads at 5.4k instead of 12.4k updates/s).
// (a scan's arrays and their bytes: scan_arrays, scan_buf_bytes, upload_plan.h)
static size_t spare_budget() {
    static const size_t b = [] {
        const char* e = std::getenv("LIVO_SPARE_MB");
        const long long mb = e ? std::atoll(e) : 8192;
        return (size_t)std::max(0LL, mb) << 20;
    }();
    return b;
}
static int alloc_scan_buf(livo_ctx* c, ScanBuf& s, int64_t N) {
    int best = -1;
    for (size_t k = 0; k < c->spare.size(); k++) {
        const int64_t cap = c->spare[k].cap;
        if (cap >= N && cap <= 2 * N + 4096 && (best < 0 || cap < c->spare[best].cap)) best = (int)k;
    }
    if (best >= 0) {
        s = c->spare[best];
        c->spare.erase(c->spare.begin() + best);
    } else {
        s = ScanBuf{};
        int rc = 0;
        scan_arrays(s, N, [&](auto*& p, size_t count) { rc |= dev_alloc(&p, count); });
        if (rc) {
            free_scan_buf(s);
            return LIVO_E_OOM;
        }
        s.cap = N;
    }
    s.used = true;
    s.searched = false;
    s.nn_compact = s.nn_lazy = false;
    s.n = N;
    s.nblk = (int32_t)scan_blocks(N);
    s.pending = false;
    s.perm.clear();
    return LIVO_OK;
}

// Back to the spare list (the caller has synchronised the context's streams).
static void release_scan_buf(livo_ctx* c, ScanBuf& s) {
    size_t kept = scan_buf_bytes(s.cap);
    for (const ScanBuf& x : c->spare) kept += scan_buf_bytes(x.cap);
    while (!c->spare.empty() && kept > spare_budget()) {  // the oldest go first
        kept -= scan_buf_bytes(c->spare.front().cap);
        free_scan_buf(c->spare.front());
        c->spare.erase(c->spare.begin());
    }
    ScanBuf r = s;
    r.used = false;
    r.pending = false;
    r.perm = std::vector<int32_t>();
    c->spare.push_back(r);
    s = ScanBuf{};
}

// Upload scratch of N points: scan_build_layout's arrays, then (livo_scan_upload,
// livo_scan_upload_async) the packed source points (scan_upload_layout).
static size_t up_tmp_bytes(int64_t N, bool src = false) { return carve_bytes(scan_upload_layout, (size_t)N, src); }
static int ensure_up_tmp(livo_ctx* c, size_t bytes) {
    return ensure_dev_bytes(&c->up_tmp, &c->up_tmp_bytes, bytes);  // (synchronous: no upload is in flight)
}

// Where a scan is built: the stream, the sort scratch (up_tmp_bytes) and the
// rocPRIM scratch, grown on demand.
struct UpTarget {
    hipStream_t st;
    void** tmp;
    size_t* tmp_bytes;
    void** prim;
    size_t* prim_bytes;
};

// Morton-order N device points (x, y, z at d_src + stride * i floats) into the
// scan buffers s on U.st: the same keys and stable order as a host sort.  Only
// enqueues; the caller synchronises or records an event.
static int scan_build_on(const UpTarget& U, const float* d_src, int stride, int64_t N, ScanBuf& s) {
    if (N <= 0) return LIVO_OK;
    Carve k{(char*)*U.tmp};
    const ScanBuild L = scan_build_layout(k, (size_t)N, 6);
    int rc = LIVO_OK;
    // bounds start at (+max, -max) in the order-preserving encoding
    if (hipMemsetD32Async((hipDeviceptr_t)L.bounds, 0xFFFFFFFFu, 3, U.st) != hipSuccess ||
        hipMemsetD32Async((hipDeviceptr_t)(L.bounds + 3), 0u, 3, U.st) != hipSuccess)
        rc = LIVO_E_HIP;
    if (!rc) rc = launch_fe_minmax(d_src, N, stride, L.bounds, U.st);
    if (!rc) rc = launch_fe_morton(d_src, N, stride, L.bounds, morton_scale(), L.keys, L.iota, U.st);
    // (the stream drained before its rocPRIM scratch grows: an earlier build may still sort in it)
    if (!rc) rc = sort_u32_on(U.st, U.prim, U.prim_bytes, true, L.keys, L.skeys, L.iota, L.svals, N, 27);
    if (!rc) rc = launch_fe_gather(d_src, N, stride, L.svals, s.pts, s.d_iperm, U.st);
    if (!rc && (hipMemcpyAsync(s.d_perm, L.svals, (size_t)N * 4, hipMemcpyDeviceToDevice, U.st) != hipSuccess ||
                hipMemsetAsync(s.nn, 0, (size_t)N * sizeof(NNRec), U.st) != hipSuccess ||
                hipMemsetAsync(s.pstate, 0, (size_t)N, U.st) != hipSuccess))
        rc = LIVO_E_HIP;
    return rc;
}

// A resident scan from N device points (x, y, z at d_src + stride * i floats),
// built synchronously on the context's stream.
static int scan_create_device(livo_ctx* c, const float* d_src, int stride, int64_t N, int32_t* scan_id) {
    ScanBuf s;
    int rc = alloc_scan_buf(c, s, N);
    if (rc) return rc;
    if (N > 0) {
        rc = ensure_up_tmp(c, up_tmp_bytes(N));
        const UpTarget U{c->stream, &c->up_tmp, &c->up_tmp_bytes, &c->prim_tmp, &c->prim_bytes};
        if (!rc) rc = scan_build_on(U, d_src, stride, N, s);
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = LIVO_E_HIP;
        if (rc) {
            release_scan_buf(c, s);
            return rc;
        }
    }
    *scan_id = register_scan(c, s);
    return LIVO_OK;
}

// The caller's points packed to x, y, z (a strided PointType array is read once).
static void pack_xyz(const float* xyz, int64_t N, int64_t stride_bytes, float* out) {
    const char* base = (const char*)xyz;
    if (stride_bytes == (int64_t)(3 * sizeof(float))) {
        std::memcpy(out, xyz, (size_t)N * 3 * sizeof(float));
        return;
    }
    for (int64_t i = 0; i < N; i++) std::memcpy(out + 3 * i, base + i * stride_bytes, 3 * sizeof(float));
}

// What every upload entry point checks of a scan's size and stride (0: packed x, y, z).
static int upload_args(int64_t N, int64_t& stride_bytes) {
    if (N < 0) return LIVO_E_INVALID;
    if (N > (int64_t)0x7FFFFFFF - kBlock) return LIVO_E_RANGE;
    if (stride_bytes == 0) stride_bytes = 3 * sizeof(float);
    return stride_bytes < (int64_t)(3 * sizeof(float)) ? LIVO_E_INVALID : LIVO_OK;
}

int livo_scan_upload(livo_ctx* c, const float* xyz, int64_t N, int64_t stride_bytes, int32_t* scan_id) {
    if (!c || !scan_id || (N > 0 && !xyz)) return LIVO_E_INVALID;
    RC_TRY(upload_args(N, stride_bytes));
    if (set_device(c)) return LIVO_E_HIP;
    // the caller's points packed to x, y, z, copied to HBM behind the upload
    // scratch, then Morton-ordered on the device (scan_create_device)
    float* d_src = nullptr;
    if (N > 0) {
        int rc = ensure_up_tmp(c, up_tmp_bytes(N, true));
        if (rc) return rc;
        Carve k{(char*)c->up_tmp};
        d_src = scan_upload_layout(k, (size_t)N, true).src;
        float* h = nullptr;
        const bool packed = stride_bytes == (int64_t)(3 * sizeof(float));
        if (!packed) {
            h = (float*)std::malloc((size_t)N * 3 * sizeof(float));
            if (!h) return LIVO_E_OOM;
            pack_xyz(xyz, N, stride_bytes, h);
        }
        const hipError_t e = hipMemcpyAsync(d_src, packed ? xyz : h, (size_t)N * 3 * sizeof(float),
                                            hipMemcpyHostToDevice, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);
        std::free(h);
        if (e != hipSuccess || e2 != hipSuccess) return LIVO_E_HIP;
    }
    return scan_create_device(c, d_src, 3, N, scan_id);
}

// The ring's oldest pinned staging buffer, the copy last sent out of it done,
// grown to `bytes`.
static int pin_take(UploadDev& U, size_t bytes, PinSlot** out) {
    PinSlot& P = U.pin[U.pin_next];
    U.pin_next = (U.pin_next + 1) % kPinRing;
    if (P.inflight && hipEventSynchronize(P.copied) != hipSuccess) return LIVO_E_HIP;
    P.inflight = false;
    if (!lazy_event(&P.copied)) return LIVO_E_HIP;
    if (bytes > P.bytes) {
        if (P.h) (void)hipHostFree(P.h);
        P.h = nullptr;
        P.bytes = 0;
        if (hipHostMalloc((void**)&P.h, bytes, hipHostMallocDefault) != hipSuccess) {
            P.h = nullptr;
            return LIVO_E_OOM;
        }
        P.bytes = bytes;
    }
    *out = &P;
    return LIVO_OK;
}
// A copy out of P has been enqueued on st: the slot is in flight from here on,
// whatever fails next (without the event the stream is waited for instead).
static int pin_sent(PinSlot& P, hipStream_t st) {
    P.inflight = true;
    if (hipEventRecord(P.copied, st) == hipSuccess) return LIVO_OK;
    (void)hipStreamSynchronize(st);
    return LIVO_E_HIP;
}

// A scan about to be built by an asynchronous upload passes through three
// steps.  pending_scan: its buffers and `ready` event, named in no launch yet.
// publish_pending: the build is queued on st; the scan is registered, gated by
// `ready` (s is empty afterwards).  drop_pending: the upload failed before
// that; the upload streams are drained, then the buffers still held in s[]
// return to the spare pool -- the only way back for a buffer that a queued
// launch may name (release_scan_buf's rule).
static int pending_scan(livo_ctx* c, int64_t N, ScanBuf& s) {
    const int rc = alloc_scan_buf(c, s, N);
    if (rc || lazy_event(&s.ready)) return rc;
    release_scan_buf(c, s);
    return LIVO_E_HIP;
}
static int publish_pending(livo_ctx* c, ScanBuf& s, hipStream_t st, int32_t* id) {
    if (hipEventRecord(s.ready, st) != hipSuccess) return LIVO_E_HIP;
    s.pending = true;
    *id = register_scan(c, s);
    s = ScanBuf{};
    return LIVO_OK;
}
static void drop_pending(livo_ctx* c, ScanBuf* s, int count) {
    (void)c->up.drain();
    for (int k = 0; k < count; k++)
        if (s[k].used) release_scan_buf(c, s[k]);
}

// livo_scan_upload without waiting: the points go through a pinned staging
// buffer (the caller's array is free again on return) and are copied and
// Morton-ordered on the context's upload stream, beside whatever the batch
// lanes run; the scan's `ready` event gates its users (batch_enqueue waits for
// it on the device, every other call through get_scan on the host).
int livo_scan_upload_async(livo_ctx* c, const float* xyz, int64_t N, int64_t stride_bytes, int32_t* scan_id) {
    if (!c || !scan_id || (N > 0 && !xyz)) return LIVO_E_INVALID;
    RC_TRY(upload_args(N, stride_bytes));
    if (N == 0) return livo_scan_upload(c, xyz, N, stride_bytes, scan_id);
    UploadDev& U = c->up;
    if (set_device(c) || U.streams(false)) return LIVO_E_HIP;
    const size_t need = up_tmp_bytes(N, true), bytes = (size_t)N * 3 * sizeof(float);
    if (need > U.tmp_bytes) {  // (growing: the uploads queued on it finish first)
        HIP_TRY(hipStreamSynchronize(U.up));
        RC_TRY(ensure_dev_bytes(&U.tmp, &U.tmp_bytes, need));
    }
    PinSlot* P = nullptr;
    RC_TRY(pin_take(U, bytes, &P));
    pack_xyz(xyz, N, stride_bytes, P->h);
    ScanBuf s;
    RC_TRY(pending_scan(c, N, s));
    // nothing is queued above this line; below it every failure leaves through drop_pending
    Carve k{(char*)U.tmp};
    float* d_src = scan_upload_layout(k, (size_t)N, true).src;
    int rc = hipMemcpyAsync(d_src, P->h, bytes, hipMemcpyHostToDevice, U.up) == hipSuccess ? pin_sent(*P, U.up)
                                                                                             : LIVO_E_HIP;
    const UpTarget T{U.up, &U.tmp, &U.tmp_bytes, &U.prim, &U.prim_bytes};
    if (!rc) rc = scan_build_on(T, d_src, 3, N, s);
    if (!rc) rc = publish_pending(c, s, U.up, scan_id);
    if (rc) drop_pending(c, &s, 1);
    return rc;
}

// True if p lies in page-locked host memory (livo_host_register, hipHostMalloc):
// the copy engine reads it directly.
static bool host_pinned(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
// Both ends of [p, p + bytes) page-locked: a caller that registered a shorter
// range than the array takes the staging path, not a device page fault.
static bool host_pinned_range(const void* p, size_t bytes) {
    return host_pinned(p) && (bytes <= 1 || host_pinned((const char*)p + bytes - 1));
}

int livo_host_register(livo_ctx* c, void* p, size_t bytes) {
    if (!c || !p || bytes == 0) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    // mapped + portable: the copy engine addresses the pages directly from any
    // stream (hipHostRegisterDefault alone left some processes copying at ~6 GB/s,
    // 1.5 ms of host time per 8 x 100k batch)
    return hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable) == hipSuccess ? LIVO_OK
                                                                                                    : LIVO_E_HIP;
}
int livo_host_unregister(livo_ctx* c, void* p) {
    if (!c || !p) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return LIVO_E_HIP;  // (no copy may still read it)
    return hipHostUnregister(p) == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

// LIVO_UPLOAD_TRACE (development): the host time of a batch pass's phases to
// stderr.  mark(k) ends phase k; a phase that is not marked takes no time.
struct UploadTrace {
    const bool on = std::getenv("LIVO_UPLOAD_TRACE") != nullptr;
    double t[4] = {};
    static double now_us() {
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void mark(int k) {
        if (on) std::fill(t + k, t + 4, now_us());
    }
    void print(int m, bool direct) const {
        if (on)
            std::fprintf(stderr, "[upload] %d scans %s: pinned check %.1f us, ring wait %.1f, pack / copies %.1f, build %.1f\n",
                         m, direct ? "direct" : "staged", t[1] - t[0], t[2] - t[1], t[3] - t[2], now_us() - t[3]);
    }
};

// livo_scan_upload_async for a batch of scans, kFeSegMax scans to a pass
// (upload_pass, upload_plan.h; xyz, N and sb below are the pass's own scans):
// one staging copy (pass_source), then one bounds pass, one key pass, ONE
// stable sort of the whole pass (the scan in the key's top bits) and one
// gather that also clears the neighbour records, on the upload stream
// (pass_build); then the scans get their ids (pass_register).  Each scan is
// stored exactly as livo_scan_upload stores it.

// The pass's points packed into the staging buffer S, on the copy stream; the
// upload stream waits for them.  The pass's scratch grows here, before anything
// of the pass is queued.  *direct: read from the caller's page-locked arrays.
static int pass_source(livo_ctx* c, const float* const* xyz, const int64_t* N, int64_t stride_bytes,
                       const UploadPass& P, UploadDev::Src& S, UploadTrace& T, bool* direct) {
    UploadDev& U = c->up;
    // build scratch (up): scan_build_layout with 6 bounds per scan; the packed points in S (cp copies into it)
    const size_t tmp_need = carve_bytes(scan_build_layout, (size_t)P.tot, (size_t)6 * kFeSegMax);
    const size_t bytes = (size_t)P.tot * 3 * sizeof(float);
    if (tmp_need > U.tmp_bytes || bytes > S.bytes) {  // (growing: the uploads in flight finish first)
        RC_TRY(U.drain());
        RC_TRY(ensure_dev_bytes(&U.tmp, &U.tmp_bytes, tmp_need));
        RC_TRY(ensure_dev_bytes(&S.p, &S.bytes, bytes));
    }
    float* d_src = (float*)S.p;
    // the copy into this buffer waits for the build that last read it
    if (S.used) HIP_TRY(hipStreamWaitEvent(U.cp, S.free, 0));
    // the points: straight from page-locked caller memory, else through a
    // pinned staging buffer of the ring (the caller's arrays are free on return)
    T.mark(0);
    *direct = stride_bytes == (int64_t)(3 * sizeof(float));
    for (int32_t b = 0; b < P.m && *direct; b++)
        if (N[b] > 0 && !host_pinned_range(xyz[b], (size_t)N[b] * 3 * sizeof(float))) *direct = false;
    T.mark(1);
    int rc = LIVO_OK;
    if (!*direct) {
        PinSlot* H = nullptr;
        RC_TRY(pin_take(U, bytes, &H));
        T.mark(2);
        // one host thread per scan (up to 8): a single thread's copy into pinned
        // memory ran at ~9 GB/s (1.07 ms per 8 x 100k batch)
        auto pack = [&](int32_t b) {
            if (N[b] > 0) pack_xyz(xyz[b], N[b], stride_bytes, H->h + 3 * P.off[b]);
        };
        if (bytes < ((size_t)1 << 20) || P.m == 1) {
            for (int32_t b = 0; b < P.m; b++) pack(b);
        } else {
            const int nt = std::min<int>(8, P.m);
            std::vector<std::thread> th;
            for (int t = 1; t < nt; t++)
                th.emplace_back([&, t] {
                    for (int32_t b = t; b < P.m; b += nt) pack(b);
                });
            for (int32_t b = 0; b < P.m; b += nt) pack(b);
            for (auto& x : th) x.join();
        }
        T.mark(3);
        HIP_TRY(hipMemcpyAsync(d_src, H->h, bytes, hipMemcpyHostToDevice, U.cp));
        rc = pin_sent(*H, U.cp);
    } else {
        // page-locked caller arrays: one kernel reads them through their mapped
        // device addresses (no DMA command per scan: a hipMemcpyAsync of one
        // held the host 13-16 ms now and then inside a running farm); an
        // array without a device mapping: DMA copies
        FeSrc F{};
        bool mapped = true;
        for (int32_t b = 0; b < P.m; b++) {
            F.off[b] = P.off[b];
            F.n[b] = N[b];
            void* dp = nullptr;
            if (mapped && N[b] > 0 &&
                (hipHostGetDevicePointer(&dp, const_cast<float*>(xyz[b]), 0) != hipSuccess || !dp)) {
                (void)hipGetLastError();
                mapped = false;
            }
            F.src[b] = (const float*)dp;
        }
        if (mapped) {
            rc = launch_fe_copy_seg(F, P.m, P.max_n, d_src, U.cp);
        } else {
            for (int32_t b = 0; b < P.m && !rc; b++)
                if (N[b] > 0 && hipMemcpyAsync(d_src + 3 * P.off[b], xyz[b], (size_t)N[b] * 3 * sizeof(float),
                                               hipMemcpyHostToDevice, U.cp) != hipSuccess)
                    rc = LIVO_E_HIP;
        }
        T.mark(3);  // (the copies' host time)
    }
    if (!rc && (hipEventRecord(S.copied, U.cp) != hipSuccess || hipStreamWaitEvent(U.up, S.copied, 0) != hipSuccess))
        rc = LIVO_E_HIP;
    return rc;
}

// The non-empty scans' buffers (sb) and their build out of S on the upload
// stream; S.free marks the end of the build's reads of S.
static int pass_build(livo_ctx* c, const int64_t* N, const UploadPass& P, UploadDev::Src& S, ScanBuf* sb) {
    UploadDev& U = c->up;
    Carve cv{(char*)U.tmp};
    const ScanBuild L = scan_build_layout(cv, (size_t)P.tot, (size_t)6 * kFeSegMax);
    const float* d_src = (const float*)S.p;
    FeSegs G{};
    int rc = LIVO_OK;
    for (int32_t b = 0; b < P.m && !rc; b++) {
        G.off[b] = P.off[b];
        G.n[b] = N[b];
        if (N[b] == 0) continue;  // (nothing to build: the kernels read none of its pointers)
        rc = pending_scan(c, N[b], sb[b]);
        G.pts4[b] = sb[b].pts;
        G.iperm[b] = sb[b].d_iperm;
        G.perm[b] = sb[b].d_perm;
        G.nn[b] = sb[b].nn;
        G.pstate[b] = sb[b].pstate;
    }
    // bounds start at +max (mins) and ~(-max) (maxes, stored inverted) in the order-preserving encoding
    if (!rc && hipMemsetD32Async((hipDeviceptr_t)L.bounds, 0xFFFFFFFFu, 6 * kFeSegMax, U.up) != hipSuccess)
        rc = LIVO_E_HIP;
    if (!rc) rc = launch_fe_build_seg(d_src, G, P.m, P.max_n, L.bounds, morton_scale(), L.keys, L.iota, U.up);
    if (!rc)
        rc = sort_u32_on(U.up, &U.prim, &U.prim_bytes, true, L.keys, L.skeys, L.iota, L.svals, P.tot, P.key_bits);
    if (!rc) rc = launch_fe_gather_seg(d_src, G, P.m, P.max_n, L.svals, U.up);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(S.free, U.up));
    S.used = true;
    return LIVO_OK;
}

// The pass's scans get their ids, in order: a built one behind its `ready`
// event, an empty one as livo_scan_upload registers it.  *done counts them.
static int pass_register(livo_ctx* c, const int64_t* N, const UploadPass& P, ScanBuf* sb, int32_t* ids, int32_t* done) {
    for (int32_t b = 0; b < P.m; b++, ++*done) {
        if (N[b] > 0) {
            RC_TRY(publish_pending(c, sb[b], c->up.up, ids + b));
            continue;
        }
        ScanBuf s;
        RC_TRY(alloc_scan_buf(c, s, 0));
        ids[b] = register_scan(c, s);
    }
    return LIVO_OK;
}

// A pass that fails gives up its unregistered scans (drop_pending) and the call
// releases the scans it registered before, so a failed call leaves no scan
// behind (scan_ids unspecified).
int livo_scan_upload_batch_async(livo_ctx* c, const float* const* xyz, const int64_t* N, int32_t n,
                                 int64_t stride_bytes, int32_t* scan_ids) {
    if (!c || !xyz || !N || !scan_ids || n < 0) return LIVO_E_INVALID;
    RC_TRY(upload_args(0, stride_bytes));
    for (int32_t b = 0; b < n; b++) {
        if (N[b] > 0 && !xyz[b]) return LIVO_E_INVALID;
        RC_TRY(upload_args(N[b], stride_bytes));
    }
    if (set_device(c) || c->up.streams(true)) return LIVO_E_HIP;
    int rc = LIVO_OK;
    int32_t done = 0;
    for (int32_t b0 = 0; b0 < n && !rc; b0 += kFeSegMax) {
        UploadPass P;
        ScanBuf sb[kFeSegMax];
        UploadTrace T;
        bool direct = false;
        rc = upload_pass(N, n, b0, &P);
        if (!rc && P.tot > 0) {  // (else: empty scans only)
            UploadDev::Src& S = c->up.src[c->up.src_next];
            c->up.src_next ^= 1;
            rc = pass_source(c, xyz + b0, N + b0, stride_bytes, P, S, T, &direct);
            if (!rc) rc = pass_build(c, N + b0, P, S, sb);
        }
        if (!rc) rc = pass_register(c, N + b0, P, sb, scan_ids + b0, &done);
        if (rc) drop_pending(c, sb, P.m);
        else if (P.tot > 0) T.print(P.m, direct);
    }
    if (rc)
        for (int32_t b = 0; b < done; b++) (void)livo_scan_release(c, scan_ids[b]);
    return rc;
}

int livo_scan_release(livo_ctx* c, int32_t id) {
    if (!c) return LIVO_E_INVALID;
    if (id < 0 || id >= (int32_t)c->scans.size() || !c->scans[id].used) return LIVO_E_NOSCAN;
    // a scan of a submitted batch is released once that batch is collected; every
    // other call that reads a scan returns only when its device work is done, so
    // the buffers are idle once the scan's own upload is (no stream drain: the
    // farm releases scans while the next batches run)
    for (int l = 0; l < LIVO_MAX_INFLIGHT; l++)
        if (c->lane[l].busy)
            for (int32_t x : c->lane[l].ids)
                if (x == id) return LIVO_E_BUSY;
    (void)hipSetDevice(c->device);
    ScanBuf& s = c->scans[id];
    if (s.pending && hipEventSynchronize(s.ready) != hipSuccess) return LIVO_E_HIP;
    s.pending = false;
    release_scan_buf(c, s);
    return LIVO_OK;
}

// A resident scan, its asynchronous upload finished (host wait); get_scan_q:
// without the wait (batch_enqueue, which waits for it on the device).
static ScanBuf* get_scan_q(livo_ctx* c, int32_t id) {
    if (id < 0 || id >= (int32_t)c->scans.size() || !c->scans[id].used) return nullptr;
    return &c->scans[id];
}
static ScanBuf* get_scan(livo_ctx* c, int32_t id) {
    ScanBuf* s = get_scan_q(c, id);
    if (s && s->pending) {
        if (hipEventSynchronize(s->ready) != hipSuccess) return nullptr;
        s->pending = false;
    }
    return s;
}
// The scan's stored -> caller order on the host (the per-point outputs), copied
// from the device on first use.
static int host_perm(ScanBuf* s) {
    if ((int64_t)s->perm.size() == s->n) return LIVO_OK;
    s->perm.resize((size_t)s->n);
    if (s->n > 0 && hipMemcpy(s->perm.data(), s->d_perm, (size_t)s->n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        s->perm.clear();
        return LIVO_E_HIP;
    }
    return LIVO_OK;
}

int livo_scan_neighbors(livo_ctx* c, int32_t id, int32_t* idx, float* sqdist) {
    if (!c) return LIVO_E_INVALID;
    ScanBuf* s = get_scan(c, id);
    if (!s || !s->searched) return LIVO_E_NOSCAN;
    // a scan of a submitted batch is being searched on a group stream: its
    // records are collected with the batch (livo_iekf_update_batch_wait) first
    for (const BatchLane& B : c->lane)
        if (B.busy && std::find(B.ids.begin(), B.ids.end(), id) != B.ids.end()) return LIVO_E_BUSY;
    if (set_device(c)) return LIVO_E_HIP;
    RC_TRY(ensure_nn_records(c, s, c->stream));  // (the records the last fused search left out)
    std::vector<NNRec> rec((size_t)s->n);
    if (s->n > 0) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(rec.data(), s->nn, (size_t)s->n * sizeof(NNRec), hipMemcpyDeviceToHost));
    }
    if (host_perm(s)) return LIVO_E_HIP;
    for (int64_t j = 0; j < s->n; j++) {
        const int64_t o = (int64_t)s->perm[(size_t)j];  // caller's point index
        for (int k = 0; k < kNN; k++) {
            if (idx) idx[o * kNN + k] = rec_host_idx(rec[(size_t)j], k);
            if (sqdist) sqdist[o * kNN + k] = rec_host_sqdist(rec[(size_t)j], k);
        }
    }
    return LIVO_OK;
}

int livo_h_share(livo_ctx* c, int32_t id, const livo_state* state, int search_en, double HTH[81], double HTL[9],
                 int64_t* effct, const livo_point_out* out) {
    if (!c || !state || !HTH || !HTL) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    ScanBuf* s = get_scan(c, id);
    if (!s) return LIVO_E_NOSCAN;
    if (!map_ready(c)) return LIVO_E_NOMAP;
    if (set_device(c)) return LIVO_E_HIP;
    int rc = ensure_slot(c);
    if (rc) return rc;
    const int64_t N = s->n;
    // debug scratch: normvec N*4, world N*3, sel N; laserCloudOri compaction: flags N, pos N, ori N*3, corr N*4
    const bool want_ori = out && (out->ori_xyz || out->corr_normvec || out->n_ori);
    rc = ensure_scratch(c, carve_bytes(hshare_dbg_layout, (size_t)N, want_ori));
    if (rc) return rc;
    Carve cv{(char*)c->scratch};
    const HShareDbg D = hshare_dbg_layout(cv, (size_t)N, want_ori);
    rc = ensure_nn_coords(c, s, c->stream);  // (cached neighbours may be read: search_en 0, iVox queries out of range)
    if (rc) return rc;
    init_slot(c->h_slots[0], *state, *state, c->params.max_iterations);
    fill_job(c->h_jobs[0], *s, c->d_slots);
    HIP_TRY(hipMemcpyAsync(c->d_slots, c->h_slots, sizeof(IekfSlot), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_jobs, c->h_jobs, sizeof(HsJob), hipMemcpyHostToDevice, c->stream));
    HsParams hp = make_hs_params(c);
    hp.force = search_en ? 1 : 0;
    const bool want_nv = out && out->normvec, want_sel = out && out->selected, want_w = out && out->world_xyz;
    hp.dbg.normvec = (want_nv || want_ori) ? D.normvec : nullptr;
    hp.dbg.world = want_w ? D.world : nullptr;
    hp.dbg.sel = (want_sel || want_ori) ? D.sel : nullptr;
    if (search_en) {
        rc = ensure_replay(c, N);
        if (rc) return rc;
        KnnParams kp = make_knn_params(c);
        kp.force = 1;
        if (c->backend == LIVO_BACKEND_IVOX) {
            HIP_TRY(hipMemsetAsync(kp.replay_count, 0, sizeof(unsigned), c->stream));
            HIP_TRY(hipMemsetAsync(kp.replay_count2, 0, sizeof(unsigned), c->stream));
            rc = backend_knn(c, kp, 1, N, false, c->stream);
        } else {
            rc = knn_pass(kp, 1, N, c->stream);
        }
        if (rc) return rc;
    } else if (!s->searched && N > 0) {
        // no cached neighbours yet: nothing is matched (points_near.size() < 5, :525)
        HIP_TRY(hipMemsetAsync(s->nn, 0, (size_t)N * sizeof(NNRec), c->stream));
    }
    rc = launch_hshare(hp, 1, std::max(s->nblk, 1), search_en != 0, c->stream);
    if (rc) return rc;
    // laserCloudOri / corr_normvect: the effective points in the caller's order (:547-561)
    int64_t n_ori = 0;
    if (want_ori && N > 0) {
        rc = launch_ori_flags(hp.dbg.sel, s->d_perm, N, D.flags, c->stream);
        if (!rc) rc = scan_u32(c, D.flags, D.pos, N);
        if (!rc) rc = launch_ori_scatter(s->pts, hp.dbg.normvec, hp.dbg.sel, s->d_perm, D.pos, N, D.ori, D.corr, c->stream);
        ScanCount cnt;
        if (!rc) rc = cnt.read(D.pos, D.flags, N, c->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        n_ori = cnt.sum();
        if (out->ori_xyz && n_ori > 0)
            HIP_TRY(hipMemcpyAsync(out->ori_xyz, D.ori, (size_t)n_ori * 12, hipMemcpyDeviceToHost, c->stream));
        if (out->corr_normvec && n_ori > 0)
            HIP_TRY(hipMemcpyAsync(out->corr_normvec, D.corr, (size_t)n_ori * 16, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_ori && out->n_ori) *out->n_ori = n_ori;
    // the last plane-pass block has reduced the sums into slot->red (hp.solve = 0)
    HIP_TRY(hipMemcpyAsync(c->h_slots, c->d_slots, sizeof(IekfSlot), hipMemcpyDeviceToHost, c->stream));
    std::vector<float> h_nv, h_w;
    std::vector<uint8_t> h_sel;
    if (N > 0 && out) {
        if (want_nv) {
            h_nv.resize((size_t)N * 4);
            HIP_TRY(hipMemcpyAsync(h_nv.data(), hp.dbg.normvec, (size_t)N * 16, hipMemcpyDeviceToHost, c->stream));
        }
        if (want_w) {
            h_w.resize((size_t)N * 3);
            HIP_TRY(hipMemcpyAsync(h_w.data(), hp.dbg.world, (size_t)N * 12, hipMemcpyDeviceToHost, c->stream));
        }
        if (want_sel) {
            h_sel.resize((size_t)N);
            HIP_TRY(hipMemcpyAsync(h_sel.data(), hp.dbg.sel, (size_t)N, hipMemcpyDeviceToHost, c->stream));
        }
    }
    std::vector<NNRec> recs;
    if (N > 0 && out && (out->nn_idx || out->nn_sqdist)) {
        recs.resize((size_t)N);
        HIP_TRY(hipMemcpyAsync(recs.data(), s->nn, (size_t)N * sizeof(NNRec), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (search_en) s->searched = true;
    const IekfSlot& hs = c->h_slots[0];
    const double* r = hs.red;
    std::memset(HTH, 0, 81 * sizeof(double));
    std::memset(HTL, 0, 9 * sizeof(double));
    int q = 0;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) {
            HTH[a * 9 + b] = r[q];
            HTH[b * 9 + a] = r[q];
            q++;
        }
    for (int a = 0; a < 6; a++) HTL[a] = r[21 + a];
    if (effct) *effct = (int64_t)r[28];
    if (out && out->visits) *out->visits = (int64_t)hs.visits[0];
    // per-point outputs come back in the caller's point order (stored order is Morton)
    if (host_perm(s)) return LIVO_E_HIP;
    for (int64_t k = 0; k < N; k++) {
        const int64_t i = s->perm[k];
        if (!h_nv.empty()) std::memcpy(out->normvec + 4 * i, &h_nv[4 * k], 16);
        if (!h_w.empty()) std::memcpy(out->world_xyz + 3 * i, &h_w[3 * k], 12);
        if (!h_sel.empty()) out->selected[i] = h_sel[k];
        if (!recs.empty())
            for (int j = 0; j < 5; j++) {
                if (out->nn_idx) out->nn_idx[i * 5 + j] = rec_host_idx(recs[k], j);
                if (out->nn_sqdist) out->nn_sqdist[i * 5 + j] = rec_host_sqdist(recs[k], j);
            }
    }
    return LIVO_OK;
}

// The batched iterated update of both formulations: the LaserMapping IEKF
// (states/priors/stats, model 0) or the IKFoM update (ik_states/ik_stats, model 1),
// in two halves over one batch lane: batch_enqueue puts the whole loop, and the
// copies of the slots back, on the lane's streams; batch_collect waits for them
// and unpacks the results.  Profiling (events, timings) on synchronous batches only.
static bool batch_fused(const livo_ctx* c, int model) {
    return c->fused && model == kModelLaserMapping && c->backend == LIVO_BACKEND_IKDTREE && c->knn_kind == 2;
}

// Slot b of a batch in its lane's staging area, host and device.  (A packed
// LaserMapping slot is addressed as an IekfSlot whose IKFoM block lies outside
// the buffer; the LaserMapping kernels never touch it.)
static IekfSlot& hslot(const BatchPlan& P, int32_t b) {
    return *reinterpret_cast<IekfSlot*>(P.stage->h + (size_t)b * P.stride);
}
static IekfSlot* dslot(const BatchPlan& P, int32_t b) {
    return reinterpret_cast<IekfSlot*>(P.stage->d + (size_t)b * P.stride);
}

// Profiling levels at which an event is recorded (bit k: livo_ctx_set_profiling level k).
enum { kProfL1 = 1 << 1, kProfL2 = 1 << 2, kProfAny = kProfL1 | kProfL2 };
// Records ev on st if the batch is profiled at one of `levels`; nothing otherwise.
static hipError_t prof_record(const BatchPlan& P, int levels, hipEvent_t ev, hipStream_t st) {
    return (levels >> P.prof) & 1 ? hipEventRecord(ev, st) : hipSuccess;
}

// What is refused is refused here, before any device work, so a refused batch
// leaves nothing queued.
static int batch_validate(livo_ctx* c, int L, int32_t n, const int32_t* ids, int model, bool sync) {
    if (!map_ready(c)) return LIVO_E_NOMAP;
    if (model == kModelIkfom && c->backend != LIVO_BACKEND_IKDTREE) return LIVO_E_INVALID;  // ikd-Tree h-model only
    for (int32_t b = 0; b < n; b++)
        if (!get_scan_q(c, ids[b])) return LIVO_E_NOSCAN;
    // a scan's neighbour records, plane cache and partials are per scan: the
    // same id twice in one batch would have two updates write them concurrently
    std::vector<int32_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return LIVO_E_INVALID;
    // nor may a scan be in two batches in flight
    for (int l = 0; l < LIVO_MAX_INFLIGHT; l++)
        if (l != L && c->lane[l].busy)
            for (int32_t id : c->lane[l].ids)
                if (std::binary_search(sorted.begin(), sorted.end(), id)) return LIVO_E_INVALID;
    // the unfused LaserMapping passes (iVox: per-context search scratch) run as
    // synchronous batches only; IKFoM batches keep their staging and replay
    // lists per lane
    if (!batch_fused(c, model) && model != kModelIkfom && (L != 0 || !sync)) return LIVO_E_INVALID;
    return LIVO_OK;
}

// The lane's plan for a batch of n: the path it takes and its stream groups.
// Returns the batch's points (the replay list's size).
static int64_t batch_plan(livo_ctx* c, int L, int32_t n, const int32_t* ids, int model, bool sync) {
    BatchLane& B = c->lane[L];
    BatchPlan& P = B.plan;
    P.model = model;
    P.n = n;
    P.fused = batch_fused(c, model);
    // LaserMapping slots: only the part before the IKFoM block, packed at
    // kLmStride; IKFoM slots whole.  The jobs lie behind the slots, so the
    // batch crosses PCIe in one copy each way.
    P.stage = &B.stage[model];
    P.stride = model == kModelIkfom ? sizeof(IekfSlot) : kLmStride;
    // kernel copies for submitted batches, which may queue behind another on the
    // shared streams (a DMA copy there waits on an engine hand-off); DMA copies
    // for synchronous ones (profiles/r03_ab_lanes.txt, r04_ab_block_order.txt)
    P.kcopy = !sync && P.stage->h_dev;
    // fused batches: the solve that stops a scan writes its slot into the
    // host-mapped staging copy itself (LIVO_SLOT_WB=0: copies after the batch)
    P.wb = P.fused && P.stage->h_dev && c->slot_wb;
    P.iv = c->backend == LIVO_BACKEND_IVOX && model != kModelIkfom;  // (synchronous batches only: lane 0)
    // synchronous batches only; 1: first-search events, 2: every evaluation, the batch span and the gap
    P.prof = sync && L == 0 && c->events_ready ? c->profiling : 0;
    // The batch in groups on separate streams: the latency-bound kernels of one
    // group (18x18 solve, tie replay, launch gaps, evaluations without a search)
    // overlap the throughput-bound k-NN / plane passes of the others.  Each group
    // keeps its own replay list.  Default: four groups, one per hardware queue
    // (round 4, 8 x 100k distinct scans, pipelined: 1 / 2 / 3 / 4 groups 18675 /
    // 21170 / 22350 / 22984 updates/s; 6 / 8 share the box's 4 queues and lose,
    // profiles/r04_ab_groups.txt; 8 x 200k on the 10M map: 4437 vs 3960 with two).
    // IKFoM four too (5.40k vs 5.13k with two); the iVox path two (1,520 vs 1,513 with four)
    const int auto_groups = (P.fused || model == kModelIkfom) ? 4 : 2;
    P.ngroups = std::max(1, std::min<int>(c->groups > 0 ? c->groups : auto_groups, n));
    int64_t off = 0;
    for (int gi = 0; gi < P.ngroups; gi++) {
        BatchPlan::Group& G = P.g[gi];
        G.first = (int32_t)((int64_t)n * gi / P.ngroups);
        G.count = (int32_t)((int64_t)n * (gi + 1) / P.ngroups) - G.first;
        G.max_nblk = 1;
        G.max_n = 1;
        G.off = off;
        G.st = B.st[gi];
        // a submitted fused batch's group of at most kInlineJobs scans: jobs, pose and control in
        // the launches' arguments, the slot through the first solve (a larger group: the copy kernel)
        // (P.wb: the jobs carry their slots' host-mapped addresses, HsJob::host_slot)
        G.inl = P.fused && P.kcopy && P.wb && !c->stage_copy && G.count <= kInlineJobs;
        for (int32_t b = G.first; b < G.first + G.count; b++) {
            const ScanBuf* s = get_scan_q(c, ids[b]);
            G.max_nblk = std::max(G.max_nblk, (int)s->nblk);
            G.max_n = std::max<int64_t>(G.max_n, s->n);
            off += s->n;
        }
    }
    return off;
}

// The host copies of the batch's slots and jobs.
static void batch_fill(livo_ctx* c, const BatchPlan& P, const int32_t* ids, const livo_state* states,
                       const livo_state* priors, const livo_ikfom_state* ik_states) {
    HsJob* const hjobs = reinterpret_cast<HsJob*>(P.stage->h + (size_t)P.n * P.stride);
    const int max_iter = c->params.max_iterations;
    for (int32_t b = 0; b < P.n; b++) {
        if (P.model == kModelIkfom) {
            init_slot_ik(hslot(P, b), ik_states[b], max_iter);
        } else if (P.dev_state) {
            std::memset(&hslot(P, b), 0, kSlotLmBytes);  // (the device writes its slot; this copy is the read-back's)
        } else {
            init_slot(hslot(P, b), states[b], priors ? priors[b] : states[b], max_iter, kSlotLmBytes);
        }
        fill_job(hjobs[b], *get_scan_q(c, ids[b]), dslot(P, b));
        if (P.wb) hjobs[b].host_slot = reinterpret_cast<uint4*>(P.stage->h_dev + (size_t)b * P.stride);
    }
}

// This lane's replay counters (one per group).
static unsigned* lane_rcount(livo_ctx* c, int L) { return c->d_replay_count + (size_t)L * kMaxGroups; }

// Each group stages its own slots and jobs on its own stream and starts from
// there: no fork from stream 0, so a group waits only for its own scans'
// uploads and, in a pipelined farm, for its own stream's previous batch (a
// queued batch's group g does not wait for the previous batch's group 0).
// prev: the batch whose every group this one waits for (LIVO_LANE_SERIAL=1).
static int stage_group(livo_ctx* c, int L, const BatchPlan& P, int gi, const int32_t* ids, const BatchLane* prev) {
    static_assert(sizeof(HsJob) % 16 == 0 && sizeof(IekfSlot) % 16 == 0 && kLmStride % 16 == 0, "16-B word copies");
    const BatchPlan::Group& G = P.g[gi];
    const hipStream_t st = G.st;
    for (int32_t b = G.first; b < G.first + G.count; b++) {
        ScanBuf* s = get_scan_q(c, ids[b]);
        // a scan whose asynchronous upload may still run: the group waits on the device
        if (s->pending) HIP_TRY(hipStreamWaitEvent(st, s->ready, 0));
        // IKFoM: its searches rewrite the neighbours without refitting the cached planes
        if (P.model == kModelIkfom && s->n > 0) HIP_TRY(hipMemsetAsync(s->pstate, 0, (size_t)s->n, st));
        // the unfused passes may read cached neighbours' coordinates (seeded rematch, IKFoM,
        // an iVox query with no candidate keeps its record)
        if (!P.fused) RC_TRY(ensure_nn_coords(c, s, st));
    }
    if (prev)
        for (int q = 0; q < prev->plan.ngroups; q++) HIP_TRY(hipStreamWaitEvent(st, prev->done[q], 0));
    const size_t s0 = (size_t)G.first * P.stride, sb = (size_t)G.count * P.stride;
    const size_t j0 = (size_t)P.n * P.stride + (size_t)G.first * sizeof(HsJob), jb = (size_t)G.count * sizeof(HsJob);
    if (G.inl) {
        // (nothing to copy: queue_fused puts the group's jobs and slot heads into its launches)
    } else if (P.kcopy) {
        RC_TRY(launch_copy_ranges(P.stage->h_dev, P.stage->d, s0, sb, j0, jb, st));
    } else {
        if (P.dev_state)
            RC_TRY(launch_lio_stage_slot(P.dev_state, dslot(P, G.first), c->params.max_iterations, st));
        else
            HIP_TRY(hipMemcpyAsync(P.stage->d + s0, P.stage->h + s0, sb, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(P.stage->d + j0, P.stage->h + j0, jb, hipMemcpyHostToDevice, st));
    }
    if (!P.fused) HIP_TRY(hipMemsetAsync(lane_rcount(c, L) + gi, 0, sizeof(unsigned), st));
    if (P.iv) HIP_TRY(hipMemsetAsync(c->d_replay_count2 + gi, 0, sizeof(unsigned), st));
    // profiling: each group's first search starts at ev[gi][0]
    HIP_TRY(prof_record(P, kProfAny, c->ev[gi][0], st));
    return LIVO_OK;
}

// A group's kernel parameters: its jobs and its slices of the lane's replay lists.
static void group_params(livo_ctx* c, int L, const BatchPlan& P, int gi, KnnParams& kp, HsParams& hp) {
    const BatchPlan::Group& G = P.g[gi];
    HsJob* const jobs = reinterpret_cast<HsJob*>(P.stage->d + (size_t)P.n * P.stride) + G.first;
    hp = make_hs_params(c);
    hp.jobs = jobs;
    kp = make_knn_params(c);
    kp.jobs = jobs;
    kp.replay_count = lane_rcount(c, L) + gi;
    kp.replay_list = c->d_replay_list + (size_t)L * c->replay_cap + G.off;
    kp.replay_count2 = P.iv ? c->d_replay_count2 + gi : nullptr;
    kp.replay_list2 = P.iv ? c->d_replay_list2 + G.off : nullptr;
    // the iVox overflow pass of each group has its own scratch slices (groups run concurrently)
    if (kp.iv.scratch) kp.iv.scratch += (int64_t)gi * c->iv.big_threads * c->iv.big_slice;
    // the last plane-pass block of each scan runs its solve (IKFoM: k_solve_ik, queue_unfused)
    hp.solve = P.model == kModelIkfom ? 0 : 1;
    hp.replay_count = kp.replay_count;
    hp.replay_count2 = kp.replay_count2;
}

// The fused loop: one launch per evaluation and group (a launch whose scans all stopped exits at once).
static int queue_fused(livo_ctx* c, const BatchPlan& P, const int32_t* ids, const KnnParams* kp, const HsParams* hp) {
    // (rec_compact: the ikd-Tree backend's run searches on a static map, the only writer of hot-only records)
    // (a new update replaces what an earlier one left to rebuild: batch_collect flags its own)
    for (int32_t b = 0; b < P.n; b++) {
        ScanBuf* s = get_scan_q(c, ids[b]);
        s->nn_lazy = false;
        if (kp[0].rec_compact) s->nn_compact = true;
    }
    const int evals = c->params.max_iterations + 1;
    // the groups staged inline: the host copies of their jobs, and for the first launch the
    // pose and control block of each slot and where its first solve finds the rest
    EvalInline inl[kMaxGroups];
    const HsJob* const hjobs = reinterpret_cast<const HsJob*>(P.stage->h + (size_t)P.n * P.stride);
    for (int gi = 0; gi < P.ngroups; gi++) {
        const BatchPlan::Group& G = P.g[gi];
        if (!G.inl) continue;
        EvalInline& I = inl[gi];
        std::memset(&I, 0, sizeof(I));
        I.n = G.count;
        for (int32_t k = 0; k < G.count; k++) {
            const IekfSlot& s = hslot(P, G.first + k);
            I.jobs[k] = hjobs[G.first + k];
            std::memcpy(I.head[k].rot, s.state.rot, sizeof(I.head[k].rot));
            std::memcpy(I.head[k].pos, s.state.pos, sizeof(I.head[k].pos));
            I.head[k].ctrl = s.ctrl;
        }
    }
    for (int e = 0; e < evals; e++)
        for (int gi = 0; gi < P.ngroups; gi++) {
            const BatchPlan::Group& G = P.g[gi];
            // level 2: ev[gi][e] before evaluation e, ev[gi][evals] after the last (finish_group)
            if (e > 0) HIP_TRY(prof_record(P, kProfL2, c->ev[gi][e], G.st));
            if (G.inl) inl[gi].first_in = e == 0;
            RC_TRY(launch_iekf_eval(kp[gi], hp[gi], G.count, G.max_n, e == 0, G.st, G.inl ? &inl[gi] : nullptr));
            if (e == 0) HIP_TRY(prof_record(P, kProfL1, c->ev[gi][1], G.st));
        }
    return LIVO_OK;
}

// The separate passes: per evaluation and group the search, the plane pass and the solve.
static int queue_unfused(livo_ctx* c, const BatchPlan& P, const KnnParams* kp, const HsParams* hp) {
    const int evals = c->params.max_iterations + 1;
    const bool ik = P.model == kModelIkfom;
    for (int e = 0; e < evals; e++)
        for (int gi = 0; gi < P.ngroups; gi++) {
            const BatchPlan::Group& G = P.g[gi];
            if (e > 0) HIP_TRY(prof_record(P, kProfL2, c->ev[gi][3 * e], G.st));
            // leaf-map search; rematch passes are bounded by the previous neighbours
            // (the group's replay count was zeroed before the batch / by the last k_solve)
            RC_TRY(backend_knn(c, kp[gi], G.count, G.max_n, e > 0, G.st));
            HIP_TRY(prof_record(P, e == 0 ? kProfAny : kProfL2, c->ev[gi][3 * e + 1], G.st));
            RC_TRY(ik ? launch_hshare_ik(hp[gi], G.count, G.max_nblk, e == 0, G.st)
                      : launch_hshare(hp[gi], G.count, G.max_nblk, e == 0, G.st));
            // IKFoM: the reduction, the measurement-free part of the update and the gain (k_solve_ik)
            if (ik) RC_TRY(launch_solve_ik(hp[gi], G.count, G.st));
        }
    return LIVO_OK;
}

// Each group copies its own slots back on its own stream (no cross-stream
// join before the copy) and records its end; the host then waits for every group.
static int finish_group(livo_ctx* c, BatchLane& B, const BatchPlan& P, int gi) {
    const BatchPlan::Group& G = P.g[gi];
    const int last_ev = P.fused ? c->params.max_iterations + 1 : 3 * LIVO_MAX_EVALS;
    HIP_TRY(prof_record(P, kProfL2, c->ev[gi][last_ev], G.st));
    if (P.wb) {
        // (written by the stopping solves)
    } else if (P.kcopy) {
        RC_TRY(launch_copy_words(dslot(P, G.first), P.stage->h_dev + (size_t)G.first * P.stride, P.stride * G.count,
                                 G.st));
    } else {
        HIP_TRY(hipMemcpyAsync(&hslot(P, G.first), dslot(P, G.first), P.stride * G.count, hipMemcpyDeviceToHost, G.st));
    }
    // this batch's end on the group's stream (another lane's batch may queue behind it)
    HIP_TRY(hipEventRecord(B.done[gi], G.st));
    return LIVO_OK;
}

// Profiling level 2, around the batch on the main stream: its start and the
// replay count of this batch only (every batch's replays add to the counter) ...
static int prof_batch_begin(livo_ctx* c, const BatchPlan& P) {
    if (P.prof < 2) return LIVO_OK;
    HIP_TRY(hipEventRecord(c->b_start, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_replay_total, 0, 8, c->stream));
    return LIVO_OK;
}
// ... and, once every group's searches have run (joined into the main stream),
// the counter's read-back and the batch's end.
static int prof_batch_end(livo_ctx* c, const BatchPlan& P) {
    if (P.prof < 2) return LIVO_OK;
    for (int gi = 1; gi < P.ngroups; gi++) {
        HIP_TRY(hipEventRecord(c->xjoin[gi - 1], P.g[gi].st));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->xjoin[gi - 1], 0));
    }
    HIP_TRY(hipMemcpyAsync(&c->last_replays, c->d_replay_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_replay_total, 0, 8, c->stream));
    HIP_TRY(hipEventRecord(c->b_end[c->b_par], c->stream));
    return LIVO_OK;
}

// A batch that was queued only in part, or whose end was not seen: its scans' neighbour
// records are no search's whole answer (the fused first search leaves the records that the
// second search rewrites unwritten, so some may still be an earlier update's).  They are
// searched again before anything reads them (livo_scan_neighbors: LIVO_E_NOSCAN).
static void batch_records_invalid(livo_ctx* c, int32_t n, const int32_t* ids) {
    for (int32_t b = 0; b < n; b++)
        if (ScanBuf* s = get_scan_q(c, ids[b])) s->searched = s->nn_lazy = false;
}

// dev_state (livo_lio_frame; one scan, synchronous, LaserMapping): the scan's state and prior on the device.
static int batch_enqueue(livo_ctx* c, int L, int32_t n, const int32_t* ids, int model, const livo_state* states,
                         const livo_state* priors, const livo_ikfom_state* ik_states, bool sync,
                         const livo_state* dev_state = nullptr) {
    if (!c || n < 0 || (n > 0 && (!ids || (model == kModelIkfom ? !ik_states : !states && !dev_state)))) return LIVO_E_INVALID;
    if (dev_state && (n != 1 || !sync || model != kModelLaserMapping)) return LIVO_E_INVALID;
    BatchLane& B = c->lane[L];
    if (B.busy) return LIVO_E_BUSY;
    B.n = 0;
    if (n == 0) return LIVO_OK;
    RC_TRY(batch_validate(c, L, n, ids, model, sync));
    if (set_device(c)) return LIVO_E_HIP;
    RC_TRY(lane_streams(c, L));
    RC_TRY(B.stage[model].ensure(stage_bytes(model, n)));
    const int64_t total_n = batch_plan(c, L, n, ids, model, sync);
    B.plan.dev_state = dev_state;
    const BatchPlan& P = B.plan;
    batch_fill(c, P, ids, states, priors, ik_states);
    RC_TRY(ensure_replay(c, total_n));
    RC_TRY(prof_batch_begin(c, P));
    // queued behind another lane's batch: with LIVO_LANE_SERIAL=1 start only once
    // all of its groups are done (default: each group as soon as its own stream frees)
    const BatchLane* prev = (c->lane_serial && c->last_lane >= 0 && c->last_lane != L && c->lane[c->last_lane].busy)
                                ? &c->lane[c->last_lane] : nullptr;
    c->last_lane = L;
    for (int gi = 0; gi < P.ngroups; gi++) RC_TRY(stage_group(c, L, P, gi, ids, prev));  // (copies: no record touched yet)
    const int rc = [&]() -> int {
        KnnParams kp[kMaxGroups];
        HsParams hp[kMaxGroups];
        for (int gi = 0; gi < P.ngroups; gi++) group_params(c, L, P, gi, kp[gi], hp[gi]);
        B.plan.lazy = P.fused && kp[0].rec_lazy != 0;
        RC_TRY(P.fused ? queue_fused(c, P, ids, kp, hp) : queue_unfused(c, P, kp, hp));
        for (int gi = 0; gi < P.ngroups; gi++) RC_TRY(finish_group(c, B, P, gi));
        return prof_batch_end(c, P);
    }();
    if (rc) {
        batch_records_invalid(c, n, ids);
        return rc;
    }
    B.busy = true;
    B.n = n;
    B.ids.assign(ids, ids + n);
    return LIVO_OK;
}

// The timings of a profiled batch from its events and slots (livo_last_timings).
static void batch_timings(livo_ctx* c, const BatchPlan& P, const int32_t* ids, unsigned long long replays) {
    const int32_t n = P.n;
    const int ngroups = P.ngroups, evals = c->params.max_iterations + 1;
    const bool full = P.prof >= 2;
    livo_timings t{};
    // first search of the whole batch: wall time from the earliest group's
    // start to the latest group's end (the groups start on their own streams)
    double lead = 0.0;  // how long before group 0 the earliest group started
    for (int gi = 0; gi < ngroups; gi++) {
        float ms = 0.f, m0 = 0.f;
        (void)hipEventElapsedTime(&ms, c->ev[0][0], c->ev[gi][1]);
        (void)hipEventElapsedTime(&m0, c->ev[0][0], c->ev[gi][0]);
        t.knn_ms = std::max(t.knn_ms, (double)ms);
        lead = std::max(lead, -(double)m0);
    }
    t.knn_ms += lead;
    t.knn_launches = 1;
    if (full && P.fused) {
        // every evaluation launch: max over the concurrent groups
        t.n_evals = std::min(evals, LIVO_MAX_EVALS);
        for (int e = 0; e < t.n_evals; e++) {
            // the evaluation's window over the concurrent groups (e = 0: the same
            // window as knn_ms above, from the earliest group's start)
            double m = 0.0;
            for (int gi = 0; gi < ngroups; gi++) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e == 0 ? c->ev[0][0] : c->ev[gi][e], c->ev[gi][e + 1]);
                m = std::max(m, (double)ms);
            }
            if (e == 0) m = t.knn_ms;
            t.eval_ms[e] = m;
            int searched = 0;
            for (int32_t b = 0; b < n; b++) searched += hslot(P, b).eval_search[e] != 0;
            t.eval_searched[e] = searched;
            if (e == 0) t.knn_ms = m;
            else if (searched) t.rematch_knn_ms += m;
            else t.plane_ms += m;
        }
    }
    if (full) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->b_start, c->b_end[c->b_par]);
        t.batch_ms = ms;
        if (c->b_prev) {
            (void)hipEventElapsedTime(&ms, c->b_end[c->b_par ^ 1], c->b_start);
            t.gap_ms = ms;
        }
        c->b_prev = true;
        c->b_par ^= 1;
    }
    for (int gi = 0; gi < ngroups && full && !P.fused; gi++)
        for (int e = 0; e < evals; e++) {
            float ms_k = 0.f, ms_h = 0.f;
            if (e > 0) (void)hipEventElapsedTime(&ms_k, c->ev[gi][3 * e], c->ev[gi][3 * e + 1]);
            const hipEvent_t end = (e + 1 < evals) ? c->ev[gi][3 * e + 3] : c->ev[gi][3 * LIVO_MAX_EVALS];
            (void)hipEventElapsedTime(&ms_h, c->ev[gi][3 * e + 1], end);
            t.rematch_knn_ms += ms_k;
            t.plane_ms += ms_h;  // plane pass + the solve run by its last block
        }
    // the first evaluation searches for every point of every scan
    for (int32_t b = 0; b < n; b++) {
        t.knn_visits += (int64_t)hslot(P, b).visits[0];
        t.knn_points += (int64_t)hslot(P, b).scanned[0];
        t.knn_queries += c->scans[ids[b]].n;
        t.effct_points += P.model == kModelIkfom ? hslot(P, b).ik.stats.effct_feat_num[0]
                                                 : hslot(P, b).stats.effct_feat_num[0];
    }
    t.knn_replays = (int64_t)replays;
    c->last = t;
}

static int batch_collect(livo_ctx* c, int L, livo_state* states, livo_iter_stats* stats,
                         livo_ikfom_state* ik_states, livo_ikfom_stats* ik_stats) {
    BatchLane& B = c->lane[L];
    if (B.n == 0) return LIVO_OK;
    if (!B.busy) return LIVO_E_INVALID;
    const BatchPlan& P = B.plan;
    const std::vector<int32_t> ids = std::move(B.ids);
    B.ids.clear();
    B.busy = false;  // collected (or failed): the lane is free either way
    B.n = 0;
    // wait by polling: the batch is short, and a blocking wait's wake-up
    // latency was a visible part of the gap between two batches
    const int rc = [&]() -> int {
        for (int gi = P.ngroups - 1; gi >= 0; gi--) HIP_TRY(event_wait(B.done[gi]));
        if (P.prof >= 2) HIP_TRY(stream_wait(c->stream));  // the replay counter's read-back and the batch-end event
        return LIVO_OK;
    }();
    if (rc) {
        batch_records_invalid(c, P.n, ids.data());
        return rc;
    }
    for (int32_t b = 0; b < P.n; b++) {
        const IekfSlot& s = hslot(P, b);
        if (P.model == kModelIkfom) {
            ik_states[b] = s.ik.x;
            if (ik_stats) ik_stats[b] = s.ik.stats;
        } else {
            states[b] = s.state;
            if (stats) stats[b] = s.stats;
        }
        ScanBuf& sc = c->scans[ids[b]];
        sc.searched = true;
        // a scan whose last search was not the loop's first left out the records no lane
        // read (k_iekf_eval<false>, rec_lazy): its pose stays with the scan, for ensure_nn_records
        int last = 0;
        for (int e = 0; e < std::min<int>(s.ctrl.n_evals, LIVO_MAX_EVALS); e++)
            if (s.eval_search[e]) last = e;
        sc.nn_lazy = P.lazy && last > 0;
        if (sc.nn_lazy) std::memcpy(sc.nn_pose, s.nn_pose, sizeof(sc.nn_pose));
    }
    if (P.prof) batch_timings(c, P, ids.data(), c->last_replays);
    return LIVO_OK;
}

// An enqueue that failed half-way: let the lane's queued work finish and free the lane.
static void lane_abort(BatchLane& B) {
    for (int k = 0; k < kMaxGroups && B.st[k]; k++) (void)hipStreamSynchronize(B.st[k]);
    B.busy = false;
    B.n = 0;
    B.ids.clear();
    B.ticket = -1;
}

static int batch_update(livo_ctx* c, int32_t n, const int32_t* ids, int model, livo_state* states,
                        const livo_state* priors, livo_iter_stats* stats, livo_ikfom_state* ik_states,
                        livo_ikfom_stats* ik_stats, const livo_state* dev_state = nullptr) {
    if (c && any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    const int rc = batch_enqueue(c, 0, n, ids, model, states, priors, ik_states, true, dev_state);
    if (rc) {
        if (c) lane_abort(c->lane[0]);
        return rc;
    }
    return batch_collect(c, 0, states, stats, ik_states, ik_stats);
}

int livo_iekf_update_batch(livo_ctx* c, int32_t n, const int32_t* ids, livo_state* states, const livo_state* priors,
                           livo_iter_stats* stats) {
    return batch_update(c, n, ids, kModelLaserMapping, states, priors, stats, nullptr, nullptr);
}

static int batch_submit(livo_ctx* c, int32_t n, const int32_t* ids, int model, const livo_state* states,
                        const livo_state* priors, const livo_ikfom_state* ik_states, int32_t* ticket) {
    if (!c || !ticket) return LIVO_E_INVALID;
    int L = -1;
    for (int l = 0; l < LIVO_MAX_INFLIGHT && L < 0; l++)
        if (!c->lane[l].busy) L = l;
    if (L < 0) return LIVO_E_BUSY;
    const int rc = batch_enqueue(c, L, n, ids, model, states, priors, ik_states, false);
    if (rc) {
        lane_abort(c->lane[L]);
        return rc;
    }
    c->lane[L].busy = true;  // (an empty batch too: its ticket is waited for like any other)
    c->lane_gen = (c->lane_gen + 1) & 0x3fffffff;
    c->lane[L].ticket = c->lane_gen * LIVO_MAX_INFLIGHT + L;
    *ticket = c->lane[L].ticket;
    return LIVO_OK;
}

int livo_iekf_update_batch_submit(livo_ctx* c, int32_t n, const int32_t* ids, const livo_state* states,
                                  const livo_state* priors, int32_t* ticket) {
    return batch_submit(c, n, ids, kModelLaserMapping, states, priors, nullptr, ticket);
}

static int batch_wait(livo_ctx* c, int32_t ticket, int model, livo_state* states, livo_iter_stats* stats,
                      livo_ikfom_state* ik_states, livo_ikfom_stats* ik_stats) {
    if (!c || ticket < 0) return LIVO_E_INVALID;
    const int L = ticket % LIVO_MAX_INFLIGHT;
    BatchLane& B = c->lane[L];
    if (!B.busy || B.ticket != ticket) return LIVO_E_INVALID;
    if (B.n > 0 && (B.plan.model != model || (model == kModelIkfom ? !ik_states : !states))) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    B.ticket = -1;
    if (B.n == 0) {
        B.busy = false;
        return LIVO_OK;
    }
    return batch_collect(c, L, states, stats, ik_states, ik_stats);
}

int livo_iekf_update_batch_wait(livo_ctx* c, int32_t ticket, livo_state* states, livo_iter_stats* stats) {
    return batch_wait(c, ticket, kModelLaserMapping, states, stats, nullptr, nullptr);
}

int livo_ikfom_update_batch_submit(livo_ctx* c, int32_t n, const int32_t* ids, const livo_ikfom_state* states,
                                   int32_t* ticket) {
    return batch_submit(c, n, ids, kModelIkfom, nullptr, nullptr, states, ticket);
}

int livo_ikfom_update_batch_wait(livo_ctx* c, int32_t ticket, livo_ikfom_state* states, livo_ikfom_stats* stats) {
    return batch_wait(c, ticket, kModelIkfom, nullptr, nullptr, states, stats);
}

int livo_iekf_update(livo_ctx* c, int32_t id, livo_state* state, const livo_state* prior, livo_iter_stats* stats) {
    if (!state) return LIVO_E_INVALID;
    return livo_iekf_update_batch(c, 1, &id, state, prior, stats);
}

int livo_ikfom_update_batch(livo_ctx* c, int32_t n, const int32_t* ids, livo_ikfom_state* states,
                            livo_ikfom_stats* stats) {
    return batch_update(c, n, ids, kModelIkfom, nullptr, nullptr, nullptr, states, stats);
}

int livo_ikfom_update(livo_ctx* c, int32_t id, livo_ikfom_state* state, livo_ikfom_stats* stats) {
    if (!state) return LIVO_E_INVALID;
    return livo_ikfom_update_batch(c, 1, &id, state, stats);
}

int livo_ctx_set_backend(livo_ctx* c, int backend) {
    if (!c || (backend != LIVO_BACKEND_IKDTREE && backend != LIVO_BACKEND_IVOX)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (backend != c->backend) {
        if (set_device(c)) return LIVO_E_HIP;
        if (int rc = fill_all_nn_coords(c)) return rc;
        for (auto& s : c->scans) s.searched = false;  // cached neighbours belong to the other map
    }
    c->backend = backend;
    return LIVO_OK;
}

int livo_ivox_params_default(livo_ivox_params* p) {
    if (!p) return LIVO_E_INVALID;
    p->resolution = 0.2f;   // ivox_grid_resolution default (laser_mapping.cpp:1021)
    p->nearby_type = 18;    // ivox_nearby_type default (laser_mapping.cpp:1022)
    p->capacity = 1000000;  // Options::capacity_ (ivox3d.h:57)
    return LIVO_OK;
}

int livo_ivox_init(livo_ctx* c, const livo_ivox_params* p) {
    if (!c) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    livo_ivox_params prm;
    livo_ivox_params_default(&prm);
    if (p) prm = *p;
    int nearby = 0;
    switch (prm.nearby_type) {
        case 0: nearby = 1; break;
        case 6: nearby = 7; break;
        case 18: nearby = 19; break;
        case 26: nearby = 27; break;
        default: return LIVO_E_INVALID;
    }
    if (!(prm.resolution > 0.f) || !std::isfinite(prm.resolution) || prm.capacity < 1) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    ivox_free(c->iv);
    IvoxDev& v = c->iv;
    v.prm = prm;
    v.inv_res = (float)(1.0 / (double)prm.resolution);  // options_.inv_resolution_ = 1.0 / resolution_
    v.nearby = nearby;
    if (const char* e = std::getenv("LIVO_IVOX_KIND"))  // (A/B and tests: force one search kernel)
        v.kind = std::strcmp(e, "thread") == 0 ? 0 : (std::strcmp(e, "wave") == 0 ? 1 : (std::strcmp(e, "team") == 0 ? 2 : -1));
    if (dev_alloc(&v.ctr, 5)) return LIVO_E_OOM;  // the counters of IvoxParams::ctr
    int rc = ivox_ensure_table(c, 1024);
    if (!rc) rc = ivox_ensure_big(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    v.ready = true;
    for (auto& s : c->scans) s.searched = false;
    return LIVO_OK;
}

int livo_ivox_add_points(livo_ctx* c, const float* xyz, int64_t n, int64_t stride_bytes) {
    if (!c || n < 0 || (n > 0 && !xyz)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (stride_bytes == 0) stride_bytes = 3 * sizeof(float);
    if (stride_bytes < (int64_t)(3 * sizeof(float))) return LIVO_E_INVALID;
    if (!c->iv.ready) return LIVO_E_NOMAP;
    if (n == 0) return LIVO_OK;
    if (set_device(c)) return LIVO_E_HIP;
    int rc = ivox_ensure_src(c, n);
    if (rc) return rc;
    std::vector<float> h((size_t)n * 4);
    const char* base = (const char*)xyz;
    for (int64_t i = 0; i < n; i++) {
        const float* p = (const float*)(base + i * stride_bytes);
        h[4 * i] = p[0]; h[4 * i + 1] = p[1]; h[4 * i + 2] = p[2]; h[4 * i + 3] = 0.f;
    }
    HIP_TRY(hipMemcpyAsync(c->iv.src, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return ivox_add_dev(c, n);
}

int livo_ivox_knn(livo_ctx* c, const float* q, int64_t n, int32_t max_num, double max_range, int32_t* idx,
                  float* d, int32_t* cnt) {
    if (!c || n < 0 || max_num < 1 || max_num > kNN || !(max_range >= 0.0) ||
        (n > 0 && (!q || !idx || !d || !cnt)))
        return LIVO_E_INVALID;
    if (!c->iv.ready) return LIVO_E_NOMAP;
    if (n == 0) return LIVO_OK;
    if (n > (int64_t)0x7FFFFFFF - kBlock) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    int rc = ensure_slot(c);
    if (rc) return rc;
    const size_t qb = (size_t)n * 4 * sizeof(float), rb = (size_t)n * sizeof(NNRec);
    rc = ensure_scratch(c, carve_bytes(knn_query_layout<NNRec>, (size_t)n));
    if (!rc) rc = ensure_replay(c, n);
    if (rc) return rc;
    Carve cv{(char*)c->scratch};
    const KnnQuery<NNRec> Q = knn_query_layout<NNRec>(cv, (size_t)n);
    std::vector<float> hq((size_t)n * 4);
    for (int64_t i = 0; i < n; i++) {
        hq[4 * i] = q[3 * i]; hq[4 * i + 1] = q[3 * i + 1]; hq[4 * i + 2] = q[3 * i + 2]; hq[4 * i + 3] = 0.f;
    }
    std::memset(&c->h_slots[0], 0, sizeof(IekfSlot));
    HsJob& j = c->h_jobs[0];
    j = HsJob{};
    j.pts = Q.q; j.nn = Q.rec; j.slot = c->d_slots; j.n = (int32_t)n; j.nblk = 0;
    HIP_TRY(hipMemcpyAsync(Q.q, hq.data(), qb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(Q.rec, 0xFF, rb, c->stream));  // cnt = -1: left alone = nothing found
    HIP_TRY(hipMemcpyAsync(c->d_slots, c->h_slots, sizeof(IekfSlot), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_jobs, c->h_jobs, sizeof(HsJob), hipMemcpyHostToDevice, c->stream));
    KnnParams kp = make_knn_params(c);
    kp.force = 1;
    kp.identity = 1;
    kp.iv.max_num = max_num;
    kp.iv.range2 = max_range * max_range;
    HIP_TRY(hipMemsetAsync(kp.replay_count, 0, sizeof(unsigned), c->stream));
    HIP_TRY(hipMemsetAsync(kp.replay_count2, 0, sizeof(unsigned), c->stream));
    rc = launch_ivox_knn(kp, 1, n, false, c->iv.big_threads, c->stream);
    if (rc) return rc;
    std::vector<NNRec> hr((size_t)n);
    HIP_TRY(hipMemcpyAsync(hr.data(), Q.rec, rb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; i++) {
        cnt[i] = rec_host_cnt(hr[i]);
        for (int t = 0; t < max_num; t++) {
            const bool has = rec_host_cnt(hr[i]) > t;
            idx[i * max_num + t] = has ? rec_host_idx(hr[i], t) : -1;
            d[i * max_num + t] = has ? rec_host_sqdist(hr[i], t) : INFINITY;
        }
    }
    return LIVO_OK;
}

int livo_ivox_get_info(livo_ctx* c, livo_ivox_info* out) {
    if (!c || !out) return LIVO_E_INVALID;
    if (!c->iv.ready) return LIVO_E_NOMAP;
    const IvoxDev& v = c->iv;
    out->num_points = v.npts;
    out->num_grids = v.ngrids;
    out->ids_issued = v.next_id;
    out->max_grid_points = v.max_grid;
    out->add_passes = v.add_passes;
    out->device_bytes = v.table * (int64_t)(sizeof(GridSlot) + 4 * sizeof(uint32_t)) +
                        (v.pts_cap[0] + v.pts_cap[1]) * 16 +
                        kMaxGroups * v.big_threads * v.big_slice * (int64_t)sizeof(SelElem);
    return LIVO_OK;
}

int livo_ivox_dump(livo_ctx* c, float* xyz, int32_t* ids, int32_t* keys, int64_t cap, int64_t* n) {
    if (!c || !n) return LIVO_E_INVALID;
    if (!c->iv.ready) return LIVO_E_NOMAP;
    const IvoxDev& v = c->iv;
    *n = v.npts;
    if (cap < v.npts) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    std::vector<GridSlot> slots((size_t)v.table);
    std::vector<unsigned long long> tl((size_t)v.table);
    std::vector<float> pts((size_t)v.npts * 4);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(slots.data(), v.slots, slots.size() * sizeof(GridSlot), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tl.data(), v.tlast, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (v.npts) HIP_TRY(hipMemcpy(pts.data(), v.pts[v.cur], pts.size() * sizeof(float), hipMemcpyDeviceToHost));
    // grids_cache_ order: most recently used first (the id of each grid's last added point)
    std::vector<int64_t> order;
    for (int64_t s2 = 0; s2 < v.table; s2++)
        if (slots[(size_t)s2].key != kGridEmpty) order.push_back(s2);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return tl[(size_t)a] > tl[(size_t)b]; });
    int64_t k = 0;
    for (const int64_t s2 : order) {
        const GridSlot& g = slots[(size_t)s2];
        const int kx = (int)(g.key & 0x1FFFFFull) - kIvBias, ky = (int)((g.key >> 21) & 0x1FFFFFull) - kIvBias,
                  kz = (int)((g.key >> 42) & 0x1FFFFFull) - kIvBias;
        for (uint32_t t = 0; t < g.count && k < v.npts; t++, k++) {
            const float* p = &pts[4 * (size_t)(g.start + t)];
            if (xyz) { xyz[3 * k] = p[0]; xyz[3 * k + 1] = p[1]; xyz[3 * k + 2] = p[2]; }
            if (ids) std::memcpy(&ids[k], &p[3], 4);
            if (keys) { keys[3 * k] = kx; keys[3 * k + 1] = ky; keys[3 * k + 2] = kz; }
        }
    }
    return k == v.npts ? LIVO_OK : LIVO_E_HIP;
}

// state: on the host, or dev_state: on the device (livo_lio_frame: the loop's slot or the propagated state).
static int map_incremental(livo_ctx* c, int32_t id, const livo_state* state, const livo_state* dev_state, double fs,
                           int ekf_inited, uint8_t* cat, int64_t counts[2]) {
    if (!c || (!state && !dev_state) || !(fs > 0.0)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (c->backend != LIVO_BACKEND_IVOX) return map_incremental_ikd(c, id, state, dev_state, fs, cat, counts);
    if (!c->iv.ready) return LIVO_E_NOMAP;
    ScanBuf* s = get_scan(c, id);
    if (!s) return LIVO_E_NOSCAN;
    if (set_device(c)) return LIVO_E_HIP;
    const int64_t N = s->n;
    if (counts) counts[0] = counts[1] = 0;
    if (N == 0) return LIVO_OK;
    int rc = ensure_slot(c);
    if (rc) return rc;
    rc = ensure_scratch(c, carve_bytes(map_incr_layout, (size_t)N));
    if (!rc) rc = ivox_ensure_src(c, N);
    if (rc) return rc;
    Carve cv{(char*)c->scratch};
    const MapIncr W = map_incr_layout(cv, (size_t)N);
    rc = ensure_nn_coords(c, s, c->stream);  // (first: rebuilding skipped records takes the staging slot)
    if (rc) return rc;
    if (!dev_state) {
        init_slot(c->h_slots[0], *state, *state, c->params.max_iterations);
        HIP_TRY(hipMemcpyAsync(c->d_slots, c->h_slots, sizeof(IekfSlot), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemsetAsync(W.flags, 0, (size_t)N * 8, c->stream));
    MapIncrParams mp{};
    mp.pts = s->pts;
    mp.nn = s->nn;
    mp.keypts = c->gpts;
    mp.perm = s->d_perm;
    mp.slot = c->d_slots;
    mp.pose = reinterpret_cast<const double*>(dev_state);  // (rot[9], pos[3] lead the state)
    std::memcpy(mp.R_LI, c->params.R_LI, sizeof(mp.R_LI));
    std::memcpy(mp.t_LI, c->params.t_LI, sizeof(mp.t_LI));
    mp.ordered = W.ordered;
    mp.flags = W.flags;
    mp.cat = cat ? W.cat : nullptr;
    mp.fs = fs;
    mp.n = (int32_t)N;
    mp.ekf_inited = ekf_inited ? 1 : 0;
    rc = launch_map_incr(mp, c->stream);
    if (!rc) rc = scan_u32(c, W.flags, W.pos, 2 * N);
    if (!rc) rc = launch_compact(W.ordered, W.flags, W.pos, 2 * N, c->iv.src, c->stream);
    ScanCount kept;
    if (!rc) rc = kept.read(W.pos, W.flags, 2 * N, c->stream);
    if (rc) return rc;
    uint32_t added = 0;  // pos[N]: the first half's count
    HIP_TRY(hipMemcpyAsync(&added, W.pos + N, 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> hcat;
    if (cat) {
        hcat.resize((size_t)N);
        HIP_TRY(hipMemcpyAsync(hcat.data(), W.cat, (size_t)N, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t total = kept.sum(), n_add = added;
    if (cat) {
        if (host_perm(s)) return LIVO_E_HIP;
        for (int64_t k = 0; k < N; k++) cat[s->perm[(size_t)k]] = hcat[(size_t)k];
    }
    rc = ivox_add_dev(c, total);
    if (rc) return rc;
    if (counts) {
        counts[0] = n_add;
        counts[1] = total - n_add;
    }
    return LIVO_OK;
}

int livo_map_incremental(livo_ctx* c, int32_t id, const livo_state* state, double fs, int ekf_inited, uint8_t* cat,
                         int64_t counts[2]) {
    if (!state) return LIVO_E_INVALID;
    return map_incremental(c, id, state, nullptr, fs, ekf_inited, cat, counts);
}

int livo_scan_inherit_neighbors(livo_ctx* c, int32_t dst, int32_t src) {
    if (!c) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    ScanBuf* d = get_scan(c, dst);
    ScanBuf* s = get_scan(c, src);
    if (!d || !s) return LIVO_E_NOSCAN;
    if (dst == src) return LIVO_OK;
    if (set_device(c)) return LIVO_E_HIP;
    if (d->n == 0) return LIVO_OK;
    int rc = s->searched ? ensure_nn_coords(c, s, c->stream) : LIVO_OK;  // (whole records are copied)
    if (rc) return rc;
    d->nn_compact = d->nn_lazy = false;
    rc = launch_inherit_nn(d->nn, d->d_perm, d->n, s->nn, s->d_iperm, s->searched ? s->n : 0, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d->pstate, 0, (size_t)d->n, c->stream));  // new neighbours: planes to refit
    HIP_TRY(hipStreamSynchronize(c->stream));
    d->searched = true;  // the cache now holds the inherited entries
    return LIVO_OK;
}

// ---- PCL VoxelGrid::applyFilter behind its bounds (livo_scan_preprocess, livo_cloud_publish) ----
// The filter's arrays for nb points; F.raw (the input), F.down (nb x 5) and the bounds are the caller's.
static void voxel_grid_layout(FrontParams& F, Carve& k, size_t nb) {
    F.keys = k.take<uint32_t>(nb);
    F.iota = k.take<uint32_t>(nb);
    F.skeys = k.take<uint32_t>(nb);
    F.svals = k.take<uint32_t>(nb);
    F.flags = k.take<uint32_t>(nb);
    F.vid = k.take<uint32_t>(nb);
    F.starts = k.take<uint32_t>(nb + 1);
}
// The bounds' words before the first atomic (launch_fe_minmax, launch_cloud_publish).
static int minmax_init(livo_ctx* c, unsigned* mm) {
    static const unsigned init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    return LIVO_OK;
}
// The F.n > 0 points of F.raw with their bounds in mm (device, written on c->stream):
// *n_vox centroids into F.down in ascending leaf order, or -1 where PCL returns its input.
static int voxel_grid(livo_ctx* c, FrontParams& F, const unsigned* mm, float leaf_size, int64_t* n_vox) {
    const int64_t n = F.n;
    *n_vox = -1;
    unsigned hm[6];
    HIP_TRY(hipMemcpyAsync(hm, mm, sizeof(hm), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float mn[3], mx[3];
    auto dec = [](unsigned o) {
        const unsigned u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    };
    for (int k = 0; k < 3; k++) {
        mn[k] = dec(hm[k]);
        mx[k] = dec(hm[3 + k]);
    }
    const float inv = 1.0f / leaf_size;  // inverse_leaf_size_
    const int64_t dx = static_cast<int64_t>((mx[0] - mn[0]) * inv) + 1;
    const int64_t dy = static_cast<int64_t>((mx[1] - mn[1]) * inv) + 1;
    const int64_t dz = static_cast<int64_t>((mx[2] - mn[2]) * inv) + 1;
    if ((dx * dy * dz) > static_cast<int64_t>(0x7FFFFFFF)) return LIVO_OK;  // PCL returns the input
    int max_b[3], div_b[3];
    for (int k = 0; k < 3; k++) {
        F.min_b[k] = static_cast<int>(std::floor(mn[k] * inv));
        max_b[k] = static_cast<int>(std::floor(mx[k] * inv));
        div_b[k] = max_b[k] - F.min_b[k] + 1;
    }
    F.divb_mul[0] = 1;
    F.divb_mul[1] = div_b[0];
    F.divb_mul[2] = div_b[0] * div_b[1];
    F.inv_leaf = inv;
    const int64_t cells = (int64_t)div_b[0] * div_b[1] * div_b[2];
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < cells) bits++;
    int rc = launch_fe_leaf(F, c->stream);
    if (!rc)
        rc = sort_u32(c, F.keys, const_cast<uint32_t*>(F.skeys), F.iota, const_cast<uint32_t*>(F.svals), n, bits);
    if (!rc) rc = launch_fe_runs(F, c->stream);
    if (!rc) rc = scan_u32(c, F.flags, F.vid, n);
    ScanCount vox;
    if (!rc) rc = vox.read(F.vid, F.flags, n, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = launch_fe_starts(F, c->stream);
    if (!rc) rc = launch_fe_centroid(F, vox.sum(), c->stream);
    if (rc) return rc;
    *n_vox = vox.sum();
    return LIVO_OK;
}

// livo_scan_preprocess and livo_scan_preprocess_imu: the Pose6D table comes from the host
// (poses, uploaded here) or lies on the device already (dev_poses, its order checked when
// it was made: dev_sorted).  The points come from the host or, with raw_dev, from the device
// (livo_frame_take: a range of the ingested frame).
static int scan_preprocess(livo_ctx* c, const livo_raw_point* raw, bool raw_dev, int64_t n, const livo_imu_pose* poses,
                           const double* dev_poses, bool dev_sorted, int32_t n_poses, const double rot_end[9],
                           const double pos_end[3], float leaf_size, int32_t* scan_id, livo_raw_point* undistorted,
                           livo_raw_point* down, int64_t down_cap, int64_t* n_down, const livo_state* end_dev = nullptr) {
    if (!c || !scan_id || n < 0 || (n > 0 && !raw) || n_poses < 0 || (n_poses > 0 && !poses && !dev_poses) ||
        !std::isfinite(leaf_size))
        return LIVO_E_INVALID;
    const bool deskew = n_poses >= 2 && n > 0;
    if (deskew && !end_dev && (!rot_end || !pos_end)) return LIVO_E_INVALID;
    if (dev_poses && !dev_sorted) return LIVO_E_INVALID;
    for (int32_t k = 1; k < n_poses && !dev_poses; k++)
        if (!(poses[k].offset_time >= poses[k - 1].offset_time)) return LIVO_E_INVALID;  // the walk needs sorted segments
    if (n > (int64_t)0x7FFFFFFF - kBlock) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    // the previous frame's feats_undistort is gone from here on (its buffer may be
    // freed or overwritten below): livo_frame_to_world(-1) sees no frame until this
    // one has been processed completely
    c->fe_raw = nullptr;
    c->fe_n = 0;
    FrontParams F{};
    double* d_poses;
    int32_t* seg;
    unsigned* mm;  // the bounds (launch_fe_minmax)
    const size_t nb = (size_t)std::max<int64_t>(n, 1);
    auto layout = [&](Carve k) {
        F.raw = k.take<float>(nb * 5);
        F.poses = d_poses = k.take<double>((size_t)std::max(dev_poses ? 0 : n_poses, 1) * 22);
        F.seg = seg = k.take<int32_t>(nb);
        F.seg_rev = k.take<int32_t>(nb);
        voxel_grid_layout(F, k, nb);
        F.down = k.take<float>(nb * 5);
        mm = k.take<unsigned>(6);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&c->fe_buf, &c->fe_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)c->fe_buf});
    F.n = n;
    F.np = n_poses;
    std::memcpy(F.R_LI, c->params.R_LI, sizeof(F.R_LI));
    std::memcpy(F.t_LI, c->params.t_LI, sizeof(F.t_LI));
    if (n > 0)
        HIP_TRY(hipMemcpyAsync(F.raw, raw, (size_t)n * 20, raw_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               c->stream));
    int rc = LIVO_OK;
    if (deskew) {
        // extR_Ri = R_LI^T rot_end^T, exrR_extT = R_LI^T t_LI (IMU_Processing.cpp:337-338)
        // (end_dev: the frame-end pose is on the device, fe_compensate forms extR_Ri and pos_end there)
        const double* RL = c->params.R_LI;
        F.end_dev = reinterpret_cast<const double*>(end_dev);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3 && !end_dev; j++) {
                double acc = RL[0 * 3 + i] * rot_end[j * 3 + 0];
                for (int l = 1; l < 3; l++) acc = acc + RL[l * 3 + i] * rot_end[j * 3 + l];
                F.extR_Ri[i * 3 + j] = acc;
            }
            F.exrR_extT[i] = (RL[0 * 3 + i] * c->params.t_LI[0] + RL[1 * 3 + i] * c->params.t_LI[1]) +
                             RL[2 * 3 + i] * c->params.t_LI[2];
            if (!end_dev) F.pos_end[i] = pos_end[i];
        }
        static_assert(sizeof(livo_imu_pose) == 22 * sizeof(double), "Pose6D row");
        if (dev_poses)
            F.poses = dev_poses;
        else
            HIP_TRY(hipMemcpyAsync(d_poses, poses, (size_t)n_poses * sizeof(livo_imu_pose), hipMemcpyHostToDevice,
                                   c->stream));
        rc = launch_fe_segment(F, c->stream);
        if (!rc) {
            size_t tb = 0;
            rc = prim_inclusive_min_scan_i32(nullptr, &tb, seg, F.seg_rev, n, c->stream);
            if (!rc) rc = ensure_prim(c, tb);
            tb = c->prim_bytes;
            if (!rc) rc = prim_inclusive_min_scan_i32(c->prim_tmp, &tb, seg, F.seg_rev, n, c->stream);
        }
        if (!rc) rc = launch_fe_undistort(F, c->stream);
        if (rc) return rc;
    }
    if (undistorted && n > 0)
        HIP_TRY(hipMemcpyAsync(undistorted, F.raw, (size_t)n * 20, hipMemcpyDeviceToHost, c->stream));
    // downSizeFilterSurf: PCL VoxelGrid::applyFilter
    const float* kept = F.raw;
    int64_t n_kept = n;
    if (leaf_size > 0.f && n > 0) {
        RC_TRY(minmax_init(c, mm));
        RC_TRY(launch_fe_minmax(F.raw, n, 5, mm, c->stream));
        int64_t n_vox;
        RC_TRY(voxel_grid(c, F, mm, leaf_size, &n_vox));
        if (n_vox >= 0) {
            kept = F.down;
            n_kept = n_vox;
        }
    }
    if (n_down) *n_down = n_kept;
    if (down) {
        if (down_cap < n_kept) return LIVO_E_RANGE;
        if (n_kept > 0) HIP_TRY(hipMemcpyAsync(down, kept, (size_t)n_kept * 20, hipMemcpyDeviceToHost, c->stream));
    }
    c->fe_raw = F.raw;  // feats_undistort stays resident until the next frame (livo_frame_to_world)
    c->fe_n = n;
    return scan_create_device(c, kept, 5, n_kept, scan_id);
}

int livo_scan_preprocess(livo_ctx* c, const livo_raw_point* raw, int64_t n, const livo_imu_pose* poses,
                         int32_t n_poses, const double rot_end[9], const double pos_end[3], float leaf_size,
                         int32_t* scan_id, livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap,
                         int64_t* n_down) {
    return scan_preprocess(c, raw, false, n, poses, nullptr, true, n_poses, rot_end, pos_end, leaf_size, scan_id,
                           undistorted, down, down_cap, n_down);
}

int livo_scan_preprocess_imu(livo_ctx* c, const livo_raw_point* raw, int64_t n, float leaf_size, int32_t* scan_id,
                             livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap, int64_t* n_down) {
    if (!c || !scan_id || n < 0 || (n > 0 && !raw) || !std::isfinite(leaf_size)) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (c->imu.rows <= 0) return LIVO_E_INVALID;  // no livo_imu_propagate yet
    return scan_preprocess(c, raw, false, n, nullptr, (const double*)c->imu.table, c->imu.sorted, c->imu.rows,
                           c->imu.rot_end, c->imu.pos_end, leaf_size, scan_id, undistorted, down, down_cap, n_down);
}

// ---- IMU initialisation and forward propagation (IMU_Processing.cpp:18-51, 92-197, 236-338) ----
int livo_imu_params_default(livo_imu_params* p) {
    if (!p) return LIVO_E_INVALID;
    for (int k = 0; k < 3; k++) p->cov_acc[k] = p->cov_gyr[k] = p->cov_bias_gyr[k] = p->cov_bias_acc[k] = 0.1;
    p->mean_acc[0] = p->mean_acc[1] = 0.0;
    p->mean_acc[2] = -1.0;
    return LIVO_OK;
}

int livo_imu_params_inited(livo_imu_params* p) {
    if (!p) return LIVO_E_INVALID;
    for (int k = 0; k < 3; k++) {
        p->cov_acc[k] = p->cov_gyr[k] = 0.01;
        p->cov_bias_gyr[k] = p->cov_bias_acc[k] = 0.0001;
    }
    return LIVO_OK;
}

static double norm3(const double* v) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

int livo_imu_init(livo_ctx*, const livo_imu_sample* imu, int32_t n, livo_imu_params* params, int32_t* init_iter_num,
                  double mean_gyr[3], livo_state* state, int32_t* status) {
    if (n < 0 || (n > 0 && !imu) || !params || !init_iter_num || !mean_gyr || !state || !status ||
        *init_iter_num < 1)
        return LIVO_E_INVALID;
    *status = LIVO_IMU_INIT_COLLECTING;
    if (n == 0) return LIVO_OK;  // Process2 returns before IMU_init on an empty meas.imu
    // detectZeroVelocity: running mean and covariance over the samples
    int N = *init_iter_num;
    double* ma = params->mean_acc;
    for (int32_t s = 0; s < n; s++) {
        const double* cur_acc = imu[s].acc;
        const double* cur_gyr = imu[s].gyr;
        for (int k = 0; k < 3; k++) {
            if (N == 1) {
                ma[k] = cur_acc[k];
                mean_gyr[k] = cur_gyr[k];
            }
            ma[k] += (cur_acc[k] - ma[k]) / N;
            mean_gyr[k] += (cur_gyr[k] - mean_gyr[k]) / N;
            const double da = cur_acc[k] - ma[k], dg = cur_gyr[k] - mean_gyr[k];
            params->cov_acc[k] = params->cov_acc[k] * (N - 1.0) / N + da * da * (N - 1.0) / (N * N);
            params->cov_gyr[k] = params->cov_gyr[k] * (N - 1.0) / N + dg * dg * (N - 1.0) / (N * N);
        }
        N++;
    }
    *init_iter_num = N;
    const double na = norm3(ma);
    const bool at_rest = std::fabs(na - 9.81) < 0.1 && std::fabs(norm3(mean_gyr)) < 0.1;
    if (!at_rest) {  // Reset()
        ma[0] = ma[1] = 0.0;
        ma[2] = -1.0;
        mean_gyr[0] = mean_gyr[1] = mean_gyr[2] = 0.0;
        *init_iter_num = 1;
        *status = LIVO_IMU_INIT_RESET;
        return LIVO_OK;
    }
    if (N < 50) return LIVO_OK;
    for (int k = 0; k < 3; k++) {
        state->gravity[k] = -ma[k] / na * 9.81;
        state->bias_g[k] = mean_gyr[k];
    }
    livo_imu_params_inited(params);
    *status = LIVO_IMU_INIT_DONE;
    return LIVO_OK;
}

// n jobs in one launch on the IMU stream.  table: job 0's rows go to the context's
// resident table (livo_imu_propagate) instead of the staging area.
static int imu_propagate(livo_ctx* c, int32_t n, const livo_imu_job* jobs, const livo_imu_params* params,
                         livo_imu_carry* carries, livo_state* states, livo_imu_pose* poses, int32_t pose_cap,
                         int32_t* n_poses, bool table, const livo_state** dev_state = nullptr) {
    if (!c || n < 0 || (n > 0 && (!jobs || !carries || !states)) || !params || pose_cap < 0)
        return LIVO_E_INVALID;
    int64_t total = 0;
    int32_t max_rows = 1;
    for (int32_t j = 0; j < n; j++) {
        if (jobs[j].n_imu < 0 || (jobs[j].n_imu > 0 && !jobs[j].imu)) return LIVO_E_INVALID;
        int32_t rows = 1;  // IMUpose[0], then one row per sample not skipped at :251
        for (int32_t s = 0; s < jobs[j].n_imu; s++)
            if (!(jobs[j].imu[s].stamp < carries[j].last_lidar_end_time)) rows++;
        if (poses && rows > pose_cap) return LIVO_E_RANGE;
        max_rows = std::max(max_rows, rows);
        total += jobs[j].n_imu;
    }
    if (total > (int64_t)0x7FFFFFFF) return LIVO_E_RANGE;
    if (hip_device_count() <= 0 || set_device(c)) return LIVO_E_HIP;
    if (n == 0) return LIVO_OK;
    ImuDev& D = c->imu;
    if (!lazy_stream(&D.st)) return LIVO_E_HIP;
    const bool want_rows = poses != nullptr || table;
    const int32_t dev_cap = want_rows ? max_rows : 0;
    ImuBatch B{};
    size_t io_bytes = 0, in_bytes = 0;  // states .. counts (copied back); .. samples (copied in)
    double* d_rows = nullptr;
    livo_state* h_states = nullptr;
    livo_imu_carry* h_carries = nullptr;
    int32_t* h_counts = nullptr;
    ImuJobDev* h_jobs = nullptr;
    livo_imu_sample* h_samples = nullptr;
    auto layout = [&](Carve k, bool host) {
        auto* s = k.take<livo_state>((size_t)n);
        auto* cy = k.take<livo_imu_carry>((size_t)n);
        auto* cnt = k.take<int32_t>((size_t)n);
        io_bytes = k.total();
        auto* jb = k.take<ImuJobDev>((size_t)n);
        auto* sm = k.take<livo_imu_sample>((size_t)std::max<int64_t>(total, 1));
        in_bytes = k.total();
        if (host) {
            h_states = s, h_carries = cy, h_counts = cnt, h_jobs = jb, h_samples = sm;
        } else {
            B.states = s, B.carries = cy, B.n_poses = cnt, B.jobs = jb, B.samples = sm;
            if (!table) d_rows = k.take<double>((size_t)n * (size_t)dev_cap * 22);
        }
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&D.buf, &D.bytes, layout(Carve{nullptr}, false)));
    layout(Carve{(char*)D.buf}, false);
    const size_t host_need = layout(Carve{nullptr}, true);
    if (host_need > D.pin_bytes) {
        if (D.pin) (void)hipHostFree(D.pin);
        D.pin = nullptr;
        D.pin_bytes = 0;
        if (hipHostMalloc(&D.pin, host_need, hipHostMallocDefault) != hipSuccess) {
            D.pin = nullptr;
            return LIVO_E_OOM;
        }
        D.pin_bytes = host_need;
    }
    layout(Carve{(char*)D.pin}, true);
    if (table) {
        D.rows = 0;  // no table until this call has succeeded
        RC_TRY(ensure_dev_bytes(&D.table, &D.table_bytes, (size_t)dev_cap * 22 * sizeof(double)));
        d_rows = (double*)D.table;
    }
    int64_t at = 0;
    for (int32_t j = 0; j < n; j++) {
        h_states[j] = states[j];
        h_carries[j] = carries[j];
        h_jobs[j] = ImuJobDev{at, jobs[j].n_imu, 0, jobs[j].pcl_beg_time, jobs[j].pcl_end_time};
        if (jobs[j].n_imu > 0) std::memcpy(h_samples + at, jobs[j].imu, (size_t)jobs[j].n_imu * sizeof(livo_imu_sample));
        at += jobs[j].n_imu;
    }
    bool sorted = true;  // job 0's offset times, as the kernel writes them
    if (table) {
        double prev = 0.0;
        for (int32_t s = 0; s < jobs[0].n_imu; s++) {
            if (jobs[0].imu[s].stamp < carries[0].last_lidar_end_time) continue;
            const double off = jobs[0].imu[s].stamp - jobs[0].pcl_beg_time;
            if (!(off >= prev)) sorted = false;
            prev = off;
        }
    }
    B.poses = want_rows ? d_rows : nullptr;
    B.pose_cap = dev_cap;
    std::memcpy(B.cov_acc, params->cov_acc, sizeof(B.cov_acc));
    std::memcpy(B.cov_gyr, params->cov_gyr, sizeof(B.cov_gyr));
    std::memcpy(B.cov_bias_gyr, params->cov_bias_gyr, sizeof(B.cov_bias_gyr));
    std::memcpy(B.cov_bias_acc, params->cov_bias_acc, sizeof(B.cov_bias_acc));
    B.acc_norm = norm3(params->mean_acc);
    HIP_TRY(hipMemcpyAsync(D.buf, D.pin, in_bytes, hipMemcpyHostToDevice, D.st));
    RC_TRY(launch_imu_propagate(B, n, D.st));
    // dev_state (livo_lio_frame, one job): the propagated state stays on the device, where the later
    // stages read it; the carry and the row count come back
    const size_t io_from = dev_state ? (size_t)((char*)B.carries - (char*)D.buf) : 0;
    HIP_TRY(hipMemcpyAsync((char*)D.pin + io_from, (char*)D.buf + io_from, io_bytes - io_from, hipMemcpyDeviceToHost,
                           D.st));
    if (poses)
        HIP_TRY(hipMemcpy2DAsync(poses, (size_t)pose_cap * sizeof(livo_imu_pose), d_rows,
                                 (size_t)dev_cap * sizeof(livo_imu_pose), (size_t)dev_cap * sizeof(livo_imu_pose),
                                 (size_t)n, hipMemcpyDeviceToHost, D.st));
    HIP_TRY(stream_wait(D.st));
    for (int32_t j = 0; j < n; j++) {
        if (!dev_state) states[j] = h_states[j];
        carries[j] = h_carries[j];
        if (n_poses) n_poses[j] = h_counts[j];
    }
    if (dev_state) *dev_state = B.states;
    if (table) {
        if (!dev_state) {  // (livo_lio_frame sets them from the one state copy at its end)
            std::memcpy(D.rot_end, states[0].rot, sizeof(D.rot_end));
            std::memcpy(D.pos_end, states[0].pos, sizeof(D.pos_end));
        }
        D.sorted = sorted;
        D.rows = h_counts[0];
    }
    return LIVO_OK;
}

int livo_imu_propagate_batch(livo_ctx* c, int32_t n, const livo_imu_job* jobs, const livo_imu_params* params,
                             livo_imu_carry* carries, livo_state* states, livo_imu_pose* poses, int32_t pose_cap,
                             int32_t* n_poses) {
    return imu_propagate(c, n, jobs, params, carries, states, poses, pose_cap, n_poses, false);
}

int livo_imu_propagate(livo_ctx* c, const livo_imu_job* job, const livo_imu_params* params, livo_imu_carry* carry,
                       livo_state* state, livo_imu_pose* poses, int32_t pose_cap, int32_t* n_poses) {
    if (!job || !carry || !state) return LIVO_E_INVALID;
    return imu_propagate(c, 1, job, params, carry, state, poses, pose_cap, n_poses, true);
}

// ---- Sensor handlers: the driver's message to the time-ordered frame (preprocess.cpp:82-116,
// laser_mapping.cpp:705, IMU_Processing.cpp:217-235) ----
int livo_ingest_params_default(livo_ingest_params* p) {
    if (!p) return LIVO_E_INVALID;
    p->lidar_type = LIVO_LIDAR_AVIA;  // laser_mapping.cpp:989-993
    p->n_scans = 16;
    p->point_filter_num = 2;
    p->reserved = 0;
    p->blind = 0.01;
    return LIVO_OK;
}

// The message of n records of rec bytes -> the context's frame.  L: the cloud's layout (null: Avia).
static int frame_ingest(livo_ctx* c, const livo_ingest_params* p, const void* data, int64_t n, int64_t rec,
                        const livo_cloud_layout* L, livo_ingest_info* info) {
    if (n > (int64_t)0x7FFFFFFF - kBlock) return LIVO_E_RANGE;
    IngestParams P{};
    P.n = n;
    P.lidar_type = p->lidar_type;
    P.n_scans = p->n_scans;
    P.filter_num = p->point_filter_num;
    P.blind = p->blind;
    if (L) P.L = *L;
    if (n > 0 && p->lidar_type == LIVO_LIDAR_VELO16) {
        float t;  // pl_orig.points[plsize - 1].time (:479)
        std::memcpy(&t, (const char*)data + (n - 1) * rec + L->off_time, 4);
        if (!(t > 0.f)) return LIVO_E_INVALID;  // given_offset_time == false: the times from yaw, not built
    }
    if (n > 0 && p->lidar_type == LIVO_LIDAR_XT32) std::memcpy(&P.time_head, (const char*)data + L->off_time, 8);
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (set_device(c)) return LIVO_E_HIP;
    IngestDev& D = c->ing;
    D.have = false;  // no frame until this call has succeeded
    const size_t nb = (size_t)std::max<int64_t>(n, 1);
    unsigned char* msg;
    uint32_t *pos, *skeys, *svals;
    float* frame;
    auto layout = [&](Carve k) {
        msg = k.take<unsigned char>(nb * (size_t)rec + 4);  // (k_ingest_cloud reads whole words)
        P.dec = k.take<float>(nb * 5);
        P.flags = k.take<uint32_t>(nb);
        pos = k.take<uint32_t>(nb);
        P.pts = k.take<float>(nb * 5);
        P.keys = k.take<uint32_t>(nb);
        P.iota = k.take<uint32_t>(nb);
        skeys = k.take<uint32_t>(nb);
        svals = k.take<uint32_t>(nb);
        frame = k.take<float>(nb * 5);
        P.ctr = k.take<unsigned>(kIngCtrN);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&D.buf, &D.bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)D.buf});
    P.msg = msg;
    P.pos = pos;
    livo_ingest_info I{};
    I.n_in = n;
    if (n > 0) {
        HIP_TRY(hipMemsetAsync(P.ctr, 0, kIngCtrN * sizeof(unsigned), c->stream));
        HIP_TRY(hipMemcpyAsync(msg, data, (size_t)n * (size_t)rec, hipMemcpyHostToDevice, c->stream));
        RC_TRY(launch_ingest_decode(P, c->stream));
        RC_TRY(scan_u32(c, P.flags, pos, n));
        RC_TRY(launch_ingest_emit(P, c->stream));
        unsigned h[3];
        HIP_TRY(hipMemcpyAsync(h, P.ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(stream_wait(c->stream));
        const int64_t total = h[kIngCtrTotal];
        I.n_kept = p->lidar_type == LIVO_LIDAR_AVIA ? total / p->point_filter_num : total;
        I.n_rejected = n - (int64_t)h[kIngCtrPass];
        I.n_decimated = (int64_t)h[kIngCtrPass] - I.n_kept;
        if (I.n_kept > 0) {
            const unsigned o = h[kIngCtrMaxKey], u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
            std::memcpy(&I.end_curvature, &u, 4);
            // the stable sort by time and its permutation applied: queued, the calls that read the frame follow
            RC_TRY(sort_u32(c, P.keys, skeys, P.iota, svals, I.n_kept, 32));
            RC_TRY(launch_ingest_gather(P.pts, svals, I.n_kept, frame, c->stream));
        }
    }
    D.frame = frame;
    D.skeys = skeys;
    D.ctr = P.ctr;
    D.info = I;
    D.have = true;
    if (info) *info = I;
    return LIVO_OK;
}

static bool ingest_params_ok(const livo_ingest_params* p) {
    return p && p->point_filter_num >= 1 && p->n_scans >= 0;
}

int livo_frame_ingest_livox(livo_ctx* c, const livo_ingest_params* p, const livo_livox_point* pts, int64_t n,
                            livo_ingest_info* info) {
    if (!c || !ingest_params_ok(p) || p->lidar_type != LIVO_LIDAR_AVIA || n < 0 || (n > 0 && !pts))
        return LIVO_E_INVALID;
    return frame_ingest(c, p, pts, n, sizeof(livo_livox_point), nullptr, info);
}

int livo_frame_ingest_cloud(livo_ctx* c, const livo_ingest_params* p, const void* data, int64_t n,
                            const livo_cloud_layout* L, livo_ingest_info* info) {
    if (!c || !ingest_params_ok(p) || !L || n < 0 || (n > 0 && !data)) return LIVO_E_INVALID;
    if (p->lidar_type != LIVO_LIDAR_VELO16 && p->lidar_type != LIVO_LIDAR_OUST64 && p->lidar_type != LIVO_LIDAR_XT32)
        return LIVO_E_INVALID;
    if (L->point_step < 1 || L->point_step > kIngestMaxStep) return LIVO_E_INVALID;
    const int32_t offs[5] = {L->off_x, L->off_y, L->off_z, L->off_intensity, L->off_time};
    for (int k = 0; k < 5; k++) {
        const int32_t width = (k == 4 && p->lidar_type == LIVO_LIDAR_XT32) ? 8 : 4;
        if (offs[k] < 0 || offs[k] > L->point_step - width) return LIVO_E_INVALID;
    }
    return frame_ingest(c, p, data, n, L->point_step, L, info);
}

int livo_frame_info(livo_ctx* c, livo_ingest_info* info) {
    if (!c || !info) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (!c->ing.have) return LIVO_E_INVALID;
    *info = c->ing.info;
    return LIVO_OK;
}

int livo_frame_dump(livo_ctx* c, livo_raw_point* out, int64_t cap, int64_t* n) {
    if (!c || !n) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (!c->ing.have) return LIVO_E_INVALID;
    const int64_t m = c->ing.info.n_kept;
    *n = m;
    if (!out || m == 0) return LIVO_OK;
    if (cap < m) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipMemcpyAsync(out, c->ing.frame, (size_t)m * 20, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(stream_wait(c->stream));
    return LIVO_OK;
}

// end_dev (livo_lio_frame): the frame-end pose of the de-skew on the device instead of c->imu.rot_end / pos_end.
static int frame_take(livo_ctx* c, double offset_limit_ms, int is_lidar_end, float leaf_size, int32_t* scan_id,
                      livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap, int64_t* n_down,
                      int64_t* n_taken, const livo_state* end_dev) {
    if (!c || !n_taken || (scan_id && !std::isfinite(leaf_size))) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    IngestDev& D = c->ing;
    if (!D.have) return LIVO_E_INVALID;
    if (scan_id && c->imu.rows <= 0) return LIVO_E_INVALID;  // no livo_imu_propagate yet
    if (set_device(c)) return LIVO_E_HIP;
    const int64_t from = D.info.cursor;
    unsigned cnt = 0;
    if (from < D.info.n_kept) {
        RC_TRY(launch_ingest_take_count(D.skeys, from, D.info.n_kept, offset_limit_ms, D.ctr + kIngCtrTake, c->stream));
        HIP_TRY(hipMemcpyAsync(&cnt, D.ctr + kIngCtrTake, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(stream_wait(c->stream));
    }
    if (scan_id) {
        if (cnt == 0) {  // an empty feats_undistort: no scan
            c->fe_raw = nullptr;
            c->fe_n = 0;
            *scan_id = -1;
            if (n_down) *n_down = 0;
        } else {
            RC_TRY(scan_preprocess(c, reinterpret_cast<const livo_raw_point*>(D.frame + 5 * from), true, (int64_t)cnt,
                                   nullptr, (const double*)c->imu.table, c->imu.sorted, c->imu.rows, c->imu.rot_end,
                                   c->imu.pos_end, leaf_size, scan_id, undistorted, down, down_cap, n_down, end_dev));
        }
    }
    D.info.cursor = is_lidar_end ? 0 : from + (int64_t)cnt;  // (:229, :232-235)
    *n_taken = (int64_t)cnt;
    return LIVO_OK;
}

int livo_frame_take(livo_ctx* c, double offset_limit_ms, int is_lidar_end, float leaf_size, int32_t* scan_id,
                    livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap, int64_t* n_down,
                    int64_t* n_taken) {
    return frame_take(c, offset_limit_ms, is_lidar_end, leaf_size, scan_id, undistorted, down, down_cap, n_down, n_taken,
                      nullptr);
}

int livo_vio_params_default(livo_vio_params* p) {
    if (!p) return LIVO_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    // camera_pinhole_resize.yaml
    p->cam.width = 640;
    p->cam.height = 512;
    p->cam.fx = 431.795259219;
    p->cam.fy = 431.550090267;
    p->cam.cx = 310.833037316;
    p->cam.cy = 266.985989326;
    p->cam.d[0] = -0.0944205499243979;
    p->cam.d[1] = 0.0946727677776504;
    p->cam.d[2] = -0.00807970960613932;
    p->cam.d[3] = 8.07461209775283e-05;
    p->R_ci[0] = p->R_ci[4] = p->R_ci[8] = 1.0;
    p->img_point_cov = 10.0;  // laser_mapping.cpp:976
    p->patch_size = 4;        // laser_mapping.cpp:1015
    p->max_iterations = 4;    // origin_laserMapping.cpp:1208 (NUM_MAX_ITERATIONS)
    return LIVO_OK;
}

// ---- livo_vio_update's body: the constants of p, the launches, the statistics ----
// (pos, levels, patches, partial, perr, slot, n and nblk are the caller's)
static VioParams update_params(const livo_vio_params* p, int32_t width, int32_t height) {
    VioParams P{};
    P.cam = cam_intrinsics(p->cam, width, height);
    P.ps = p->patch_size;
    std::memcpy(P.Rci, p->R_ci, sizeof(P.Rci));
    std::memcpy(P.Pci, p->P_ci, sizeof(P.Pci));
    // init() (lidar_selection.cpp:44-55): Jdphi_dR = Rci, Jdp_dR = -Rci [Pic]x, Pic = -Rci^T Pci
    std::memcpy(P.Jdphi_dR, p->R_ci, sizeof(P.Jdphi_dR));
    double Pic[3];
    for (int a = 0; a < 3; a++)
        Pic[a] = -((p->R_ci[0 * 3 + a] * p->P_ci[0] + p->R_ci[1 * 3 + a] * p->P_ci[1]) + p->R_ci[2 * 3 + a] * p->P_ci[2]);
    const double tmp[9] = {0.0, -Pic[2], Pic[1], Pic[2], 0.0, -Pic[0], -Pic[1], Pic[0], 0.0};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            P.Jdp_dR[a * 3 + b] = ((-p->R_ci[a * 3 + 0]) * tmp[0 * 3 + b] + (-p->R_ci[a * 3 + 1]) * tmp[1 * 3 + b]) +
                                  (-p->R_ci[a * 3 + 2]) * tmp[2 * 3 + b];
    P.img_cov = p->img_point_cov;
    P.max_iter = p->max_iterations;
    return P;
}
// Queues ComputeJ on c->stream: the slot holds state and prior, P.perr is cleared here.
static int update_queue(livo_ctx* c, VioParams P) {
    if (P.n > 0) HIP_TRY(hipMemsetAsync(P.perr, 0, (size_t)P.n * 4, c->stream));  // errors: 0 until an iteration runs
    int rc = LIVO_OK;
    for (int level = 2; level >= 0 && !rc; level--) {  // ComputeJ (:970-974)
        P.level = level;
        rc = launch_vio_begin(P, level, c->stream);
        for (int it = 0; it < P.max_iter && !rc; it++) rc = launch_vio_iter(P, c->stream);
    }
    if (!rc) rc = launch_vio_end(P, c->stream);
    return rc;
}
static void update_stats(const VioSlot& hs, livo_vio_stats* stats) {
    std::memset(stats, 0, sizeof(*stats));
    for (int k = 0; k < 3; k++) {
        stats->iterations[k] = hs.ctrl.iters[k];
        stats->updates[k] = hs.ctrl.updates[k];
        stats->last_error[k] = hs.ctrl.level_error[k];
    }
    stats->cov_updated = hs.ctrl.cov_updated;
    stats->n_meas = hs.ctrl.n_meas;
    stats->out_of_frame = (int64_t)hs.ctrl.oof;
}

int livo_vio_update(livo_ctx* c, const livo_vio_params* p, const uint8_t* image, int32_t width, int32_t height,
                    const double* pos, const int32_t* levels, const float* patches, int64_t n, livo_state* state,
                    const livo_state* prior, float* errors, livo_vio_stats* stats) {
    if (!c || !p || !state || n < 0 || width <= 0 || height <= 0 || !image ||
        (n > 0 && (!pos || !levels || !patches)) || p->patch_size < 1 || p->patch_size > 8 ||
        p->max_iterations < 0 || !(p->img_point_cov > 0.0))
        return LIVO_E_INVALID;
    for (int64_t i = 0; i < n; i++)
        if (levels[i] < 0 || levels[i] > 8) return LIVO_E_INVALID;
    if (n > (int64_t)0x7FFFFFFF - 256) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    const int pst = p->patch_size * p->patch_size;
    const int nblk = (int)std::max<int64_t>(1, (n + 255) / 256);
    uint8_t* d_img;
    double *d_pos, *d_par;
    int32_t* d_lev;
    float *d_pat, *d_err;
    VioSlot* d_slot;
    const size_t nb = (size_t)std::max<int64_t>(n, 1);
    auto layout = [&](Carve k) {
        d_img = k.take<uint8_t>((size_t)width * height);
        d_pos = k.take<double>(nb * 3);
        d_lev = k.take<int32_t>(nb);
        d_pat = k.take<float>(nb * 3 * pst);
        d_par = k.take<double>((size_t)nblk * kVioCols);
        d_err = k.take<float>(nb);
        d_slot = k.take<VioSlot>(1);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&c->vio_buf, &c->vio_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)c->vio_buf});
    VioSlot hs;
    std::memset(&hs, 0, sizeof(hs));
    hs.state = *state;
    hs.prior = prior ? *prior : *state;
    HIP_TRY(hipMemcpyAsync(d_img, image, (size_t)width * height, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(d_pos, pos, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_lev, levels, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_pat, patches, (size_t)n * 3 * pst * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(d_slot, &hs, sizeof(hs), hipMemcpyHostToDevice, c->stream));
    VioParams P = update_params(p, width, height);
    P.img = d_img;
    P.n = (int32_t)n;
    P.pos = d_pos;
    P.levels = d_lev;
    P.patches = d_pat;
    P.nblk = nblk;
    P.partial = d_par;
    P.perr = d_err;
    P.slot = d_slot;
    RC_TRY(update_queue(c, P));
    HIP_TRY(hipMemcpyAsync(&hs, d_slot, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
    if (errors && n > 0) HIP_TRY(hipMemcpyAsync(errors, d_err, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n > 0) *state = hs.state;
    if (stats) update_stats(hs, stats);
    return LIVO_OK;
}

int livo_map_add_points(livo_ctx* c, const float* xyz, int64_t n, int64_t stride_bytes, float ds, int downsample_on,
                        livo_map_add_stats* stats) {
    if (!c || n < 0 || (n > 0 && !xyz)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (downsample_on && !(ds > 0.f && std::isfinite(ds))) return LIVO_E_INVALID;
    if (stride_bytes == 0) stride_bytes = 3 * sizeof(float);
    if (stride_bytes < (int64_t)(3 * sizeof(float))) return LIVO_E_INVALID;
    if (!c->has_map) return LIVO_E_NOMAP;
    if (set_device(c)) return LIVO_E_HIP;
    int rc = dyn_activate(c);
    if (!rc) rc = dyn_add_scratch(c, std::max<int64_t>(n, 1));
    if (rc) return rc;
    if (n > 0) {
        std::vector<float> h((size_t)n * 4);
        const char* base = (const char*)xyz;
        for (int64_t i = 0; i < n; i++) {
            const float* p = (const float*)(base + i * stride_bytes);
            h[4 * i] = p[0]; h[4 * i + 1] = p[1]; h[4 * i + 2] = p[2]; h[4 * i + 3] = 0.f;
        }
        HIP_TRY(hipMemcpy(c->dyn.W, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return dyn_add(c, n, ds, downsample_on != 0, stats);
}

int livo_map_delete_boxes(livo_ctx* c, const float* boxes, int64_t nb, int64_t* deleted) {
    if (!c || nb < 0 || (nb > 0 && !boxes)) return LIVO_E_INVALID;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (!c->has_map) return LIVO_E_NOMAP;
    if (set_device(c)) return LIVO_E_HIP;
    if (deleted) *deleted = 0;
    int rc = dyn_activate(c);
    if (rc || nb == 0) return rc;
    DynDev& d = c->dyn;
    if (nb > d.box_cap) {
        dev_free(d.boxes);
        d.box_cap = 0;
        if (dev_alloc(&d.boxes, (size_t)nb * 6)) return LIVO_E_OOM;
        d.box_cap = nb;
    }
    HIP_TRY(hipMemcpyAsync(d.boxes, boxes, (size_t)nb * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d.ctr, 0, kDynCtrN * sizeof(unsigned long long), c->stream));
    rc = launch_dyn_delete_boxes(d.all, d.alive, d.n_ids, d.boxes, nb, d.ctr + kDynDeleted, c->stream);
    if (rc) return rc;
    unsigned long long cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, d.ctr + kDynDeleted, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    d.n_alive -= (int64_t)cnt;
    rc = dyn_rebuild(c);
    if (rc) return rc;
    if (deleted) *deleted = (int64_t)cnt;
    return LIVO_OK;
}

int livo_map_dump(livo_ctx* c, float* xyz, int32_t* ids, int64_t cap, int64_t* n) {
    if (!c || !n || cap < 0) return LIVO_E_INVALID;
    if (!c->has_map) return LIVO_E_NOMAP;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<float> p;
    std::vector<int32_t> id;
    if (c->dyn.active) {
        const DynDev& d = c->dyn;
        std::vector<float> all((size_t)d.n_ids * 4);
        std::vector<uint8_t> alive((size_t)d.n_ids);
        if (d.n_ids > 0) {
            HIP_TRY(hipMemcpy(all.data(), d.all, all.size() * sizeof(float), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(alive.data(), d.alive, alive.size(), hipMemcpyDeviceToHost));
        }
        for (int64_t k = 0; k < d.n_ids; k++)
            if (alive[(size_t)k]) {
                p.insert(p.end(), &all[(size_t)k * 4], &all[(size_t)k * 4] + 3);
                id.push_back((int32_t)k);
            }
    } else {  // the static map: its search structure's points (x, y, z, index) by index
        const int64_t M = c->map_points;
        const float* src = c->knn_kind >= 1 ? c->gpts : c->lpts;
        std::vector<float> pts((size_t)M * 4);
        if (M > 0) HIP_TRY(hipMemcpy(pts.data(), src, pts.size() * sizeof(float), hipMemcpyDeviceToHost));
        p.resize((size_t)M * 3);
        id.resize((size_t)M);
        for (int64_t k = 0; k < M; k++) {
            uint32_t ix;
            std::memcpy(&ix, &pts[(size_t)k * 4 + 3], 4);
            ix &= kIdxMask;
            if ((int64_t)ix >= M) return LIVO_E_HIP;
            std::memcpy(&p[(size_t)ix * 3], &pts[(size_t)k * 4], 12);
            id[ix] = (int32_t)ix;
        }
    }
    *n = (int64_t)id.size();
    if (!xyz && !ids) return LIVO_OK;
    if (cap < *n) return LIVO_E_RANGE;
    if (xyz && !p.empty()) std::memcpy(xyz, p.data(), p.size() * sizeof(float));
    if (ids && !id.empty()) std::memcpy(ids, id.data(), id.size() * sizeof(int32_t));
    return LIVO_OK;
}

int livo_map_last_add_stats(livo_ctx* c, livo_map_add_stats* out) {
    if (!c || !out) return LIVO_E_INVALID;
    *out = c->dyn.last;
    return LIVO_OK;
}

// The cloud of the frame stages: the last preprocessed frame at full resolution
// (scan_id < 0; n = 0 while there is none) or a resident scan, with the
// permutations between its stored order and the caller's point order.  The two
// LIVO_CLOUD_* ids: the published world cloud and pg_down, read as stored.
static bool is_cloud_id(int32_t scan_id) { return scan_id == LIVO_CLOUD_WORLD || scan_id == LIVO_CLOUD_WORLD_DOWN; }
static int frame_cloud(livo_ctx* c, int32_t scan_id, CloudSrc* S) {
    *S = CloudSrc{};
    if (is_cloud_id(scan_id)) {
        const WorldCloud& w = c->wcloud;
        const bool down = scan_id == LIVO_CLOUD_WORLD_DOWN;
        if (w.n < 0 || (down && w.n_down < 0)) return LIVO_E_NOSCAN;
        S->src = down ? w.down : w.world;
        S->n = down ? w.n_down : w.n;
        S->stride = 5;
        S->world = 1;
        return LIVO_OK;
    }
    if (scan_id < 0) {
        S->src = c->fe_raw;
        S->n = c->fe_raw ? c->fe_n : 0;
        S->stride = 5;
        return LIVO_OK;
    }
    ScanBuf* s = get_scan(c, scan_id);
    if (!s) return LIVO_E_NOSCAN;
    S->src = s->pts;
    S->perm = s->d_perm;
    S->iperm = s->d_iperm;
    S->n = s->n;
    S->stride = 4;
    return LIVO_OK;
}

static WorldParams world_params(const livo_ctx* c, const livo_state& state) {
    WorldParams W;
    std::memcpy(W.rot, state.rot, sizeof(W.rot));
    std::memcpy(W.pos, state.pos, sizeof(W.pos));
    std::memcpy(W.R_LI, c->params.R_LI, sizeof(W.R_LI));
    std::memcpy(W.t_LI, c->params.t_LI, sizeof(W.t_LI));
    return W;
}

int livo_frame_to_world(livo_ctx* c, int32_t scan_id, const livo_state* state, livo_raw_point* out, int64_t cap,
                        int64_t* n_out) {
    if (!c || !state || !n_out) return LIVO_E_INVALID;
    CloudSrc S;
    RC_TRY(frame_cloud(c, scan_id, &S));
    const int64_t n = S.n;
    *n_out = n;
    if (!out || n == 0) return LIVO_OK;
    if (cap < n) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    int rc = ensure_scratch(c, (size_t)n * 5 * sizeof(float));
    if (rc) return rc;
    float* d_out = (float*)c->scratch;
    rc = launch_to_world(S, world_params(c, *state), d_out, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LIVO_OK;
}

static void cloud_info(const WorldCloud& w, livo_cloud_info* out) {
    std::memset(out, 0, sizeof(*out));
    out->n = w.n;
    out->n_down = w.n_down;
    out->down_filtered = w.filtered ? 1 : 0;
    out->device_bytes = (int64_t)w.bytes;
}

// *pcl_wait_pub = *laserCloudWorld at the end of a LiDAR frame (laser_mapping.cpp:258-268) and the
// pg_down every detect until the next one filters out of it (lidar_selection.cpp:341-344).
// lio_state: on the host, or dev_state: on the device (livo_lio_frame).
static int cloud_publish(livo_ctx* c, int32_t src_scan_id, const livo_state* lio_state, const livo_state* dev_state,
                         float match_leaf, livo_cloud_info* info) {
    if (!c || (!lio_state && !dev_state) || !std::isfinite(match_leaf) || is_cloud_id(src_scan_id)) return LIVO_E_INVALID;
    CloudSrc S;
    RC_TRY(frame_cloud(c, src_scan_id, &S));
    const int64_t n = S.n;
    if (n > (int64_t)0x7FFFFFFF - kRgbBlock) return LIVO_E_RANGE;  // (the stages' bound)
    if (set_device(c)) return LIVO_E_HIP;
    const bool build_down = match_leaf > 0.f;
    const size_t nb = (size_t)std::max<int64_t>(n, 1);
    // the filter's arrays: scratch, not fe_buf (feats_undistort there is the source of src_scan_id < 0)
    FrontParams F{};
    unsigned* mm = nullptr;
    auto scratch = [&](Carve k) {
        voxel_grid_layout(F, k, nb);
        mm = k.take<unsigned>(6);
        return k.total();
    };
    if (build_down && n > 0) {
        RC_TRY(ensure_scratch(c, scratch(Carve{nullptr})));
        scratch(Carve{(char*)c->scratch});
    }
    float *d_world, *d_down;
    auto clouds = [&](Carve k) {
        d_world = k.take<float>(nb * 5);
        d_down = k.take<float>(build_down ? nb * 5 : 0);
        return k.total();
    };
    WorldCloud& w = c->wcloud;
    const size_t need = clouds(Carve{nullptr});
    if (need > w.bytes) {  // the new buffer first: an allocation that fails leaves the published cloud
        void* p = nullptr;
        if (hipMalloc(&p, need) != hipSuccess) return LIVO_E_OOM;
        if (w.buf) (void)hipFree(w.buf);  // (every call that read it has synchronised)
        w.buf = p;
        w.bytes = need;
        w.n = w.n_down = -1;
    }
    clouds(Carve{(char*)w.buf});
    // the previous cloud is gone from here on: no cloud until this one is complete
    w.n = w.n_down = -1;
    w.filtered = false;
    if (mm) RC_TRY(minmax_init(c, mm));
    {
        static const livo_state none{};  // (rot / pos unread with dev_state)
        RC_TRY(launch_cloud_publish(S, world_params(c, dev_state ? none : *lio_state), d_world, mm, c->stream,
                                    reinterpret_cast<const double*>(dev_state)));
    }
    int64_t n_down = build_down ? n : -1;
    const float* down = build_down ? d_world : nullptr;
    if (mm) {
        F.raw = d_world;
        F.n = n;
        F.down = d_down;
        int64_t n_vox;
        RC_TRY(voxel_grid(c, F, mm, match_leaf, &n_vox));
        if (n_vox >= 0) {
            w.filtered = true;
            n_down = n_vox;
            down = d_down;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    w.world = d_world;
    w.down = down;
    w.n = n;
    w.n_down = n_down;
    if (info) cloud_info(w, info);
    return LIVO_OK;
}

int livo_cloud_publish(livo_ctx* c, int32_t src_scan_id, const livo_state* lio_state, float match_leaf,
                       livo_cloud_info* info) {
    if (!lio_state) return LIVO_E_INVALID;
    return cloud_publish(c, src_scan_id, lio_state, nullptr, match_leaf, info);
}

int livo_cloud_info_get(livo_ctx* c, livo_cloud_info* out) {
    if (!c || !out) return LIVO_E_INVALID;
    if (c->wcloud.n < 0) return LIVO_E_NOSCAN;
    cloud_info(c->wcloud, out);
    return LIVO_OK;
}

int livo_cloud_colorize(livo_ctx* c, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                        const uint8_t* bgr, int32_t width, int32_t height, livo_rgb_point* out, int32_t* src_index,
                        int64_t cap, int64_t* n_out, livo_rgb_stats* stats) {
    if (!c || !state || !p || !n_out) return LIVO_E_INVALID;
    if (width <= 0 || height <= 0 || width != p->cam.width || height != p->cam.height) return LIVO_E_INVALID;
    if (!bgr && !image_reusable(c->bgr_img, width, height)) return LIVO_E_INVALID;
    RgbParams R{};
    RC_TRY(frame_cloud(c, scan_id, &R.cloud));  // in the caller's point order (iperm)
    const int64_t n = R.cloud.n;
    if (n > (int64_t)0x7FFFFFFF - kRgbBlock) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    if (bgr) RC_TRY(image_stage(c->bgr_img, bgr, (size_t)3 * (size_t)width * (size_t)height, c->stream));
    unsigned long long ctr[kRgbCtrN] = {0, 0, 0, 0};
    if (n > 0) {
        const bool compact = out || src_index;
        const int64_t nblk = (n + kRgbBlock - 1) / kRgbBlock;
        livo_rgb_point* d_out;
        int32_t* d_idx;
        uint32_t* d_off;
        auto layout = [&](Carve k) {
            R.rec = k.take<livo_rgb_point>((size_t)n);
            d_out = k.take<livo_rgb_point>((size_t)n);
            d_idx = k.take<int32_t>((size_t)n);
            R.keep = k.take<uint8_t>((size_t)n);
            R.blk_cnt = k.take<uint32_t>((size_t)nblk);
            R.blk_off = d_off = k.take<uint32_t>((size_t)nblk);
            R.ctr = k.take<unsigned long long>(kRgbCtrN);
            return k.total();
        };
        RC_TRY(ensure_scratch(c, layout(Carve{nullptr})));
        layout(Carve{(char*)c->scratch});
        R.W = world_params(c, *state);
        R.cam = frame_cam(*p, *state);  // once per call
        R.img = c->bgr_img.p;
        R.out = out ? d_out : nullptr;
        R.src_index = src_index ? d_idx : nullptr;
        HIP_TRY(hipMemsetAsync(R.ctr, 0, sizeof(ctr), c->stream));
        RC_TRY(launch_rgb_points(R, c->stream));
        if (compact) {
            RC_TRY(scan_u32(c, R.blk_cnt, d_off, nblk));
            RC_TRY(launch_rgb_scatter(R, c->stream));
        }
        HIP_TRY(hipMemcpyAsync(ctr, R.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bgr) {  // the upload is done: later calls may reuse it
        c->bgr_img.w = width;
        c->bgr_img.h = height;
    }
    const int64_t kept = (int64_t)ctr[kRgbCtrKept];
    *n_out = kept;
    if (stats) {
        stats->n_in = n;
        stats->n_out = kept;
        stats->behind = (int64_t)ctr[kRgbCtrBehind];
        stats->out_of_frame = (int64_t)ctr[kRgbCtrOutOfFrame];
        stats->edge_reads = (int64_t)ctr[kRgbCtrEdge];
    }
    if ((out || src_index) && cap < kept) return LIVO_E_RANGE;
    if (kept > 0 && (out || src_index)) {
        if (out)
            HIP_TRY(hipMemcpyAsync(out, R.out, (size_t)kept * sizeof(livo_rgb_point), hipMemcpyDeviceToHost, c->stream));
        if (src_index)
            HIP_TRY(hipMemcpyAsync(src_index, R.src_index, (size_t)kept * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return LIVO_OK;
}

// ---- livo_vio_select's body: the checks and the grid, the arrays, the launches, the statistics ----
struct SelectStage {
    VisParams V{};
    int64_t length = 0;
    int pst3 = 0;
};
// Everything of livo_vio_select that needs no device (image_ok: there is an image to read).
static int select_prepare(livo_ctx* c, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                          int32_t grid_size, int32_t width, int32_t height, bool image_ok, SelectStage* S) {
    if (grid_size < 1 || p->patch_size < 1 || p->patch_size > 8) return LIVO_E_INVALID;
    if (width <= 0 || height <= 0 || width != p->cam.width || height != p->cam.height) return LIVO_E_INVALID;
    VisParams& V = S->V;
    V.grid.ps = p->patch_size;
    V.grid.border = (p->patch_size / 2 + 1) * 8;
    V.grid.grid_size = grid_size;
    // one cell at least inside the border, in both directions
    if ((int64_t)width - 2 * V.grid.border < grid_size || (int64_t)height - 2 * V.grid.border < grid_size)
        return LIVO_E_INVALID;
    V.grid.grid_n_height = height / grid_size;
    const int64_t length = (int64_t)(width / grid_size) * V.grid.grid_n_height;
    if (length > (int64_t)0x7FFFFFFF - kVisBlock) return LIVO_E_RANGE;
    V.grid.length = (int32_t)length;
    if (!image_ok) return LIVO_E_INVALID;
    RC_TRY(frame_cloud(c, scan_id, &V.cloud));  // in the caller's point order (iperm)
    if (V.cloud.n > (int64_t)0x7FFFFFFF - kVisBlock) return LIVO_E_RANGE;
    S->length = length;
    S->pst3 = 3 * p->patch_size * p->patch_size;
    V.W = world_params(c, *state);
    V.cam = frame_cam(*p, *state);  // once per call
    return LIVO_OK;
}
static void select_layout(SelectStage& S, Carve& k) {
    VisParams& V = S.V;
    const size_t length = (size_t)S.length;
    V.table = k.take<unsigned long long>(length);
    V.ctr = k.take<unsigned long long>(kVisCtrN);  // (behind the table: one clear for both)
    V.flag = k.take<uint32_t>(length);
    V.slot = k.take<uint32_t>(length);
    V.out = k.take<livo_vis_point>(length);
    V.patches = k.take<float>(length * S.pst3);
}
// Queues the selection of img on c->stream; emit: the records and patches too (V.ctr holds the counts).
static int select_queue(livo_ctx* c, SelectStage& S, const uint8_t* img, bool emit) {
    VisParams& V = S.V;
    V.img = img;
    if (V.cloud.n <= 0) return LIVO_OK;
    HIP_TRY(hipMemsetAsync(V.table, 0, (size_t)((char*)(V.ctr + kVisCtrN) - (char*)V.table), c->stream));
    RC_TRY(launch_vis_score(V, c->stream));
    RC_TRY(launch_vis_flags(V, c->stream));
    if (emit) {  // (the table bounds the result: the records are written before their count is known)
        RC_TRY(scan_u32(c, V.flag, const_cast<uint32_t*>(V.slot), S.length));
        RC_TRY(launch_vis_emit(V, c->stream));
    }
    return LIVO_OK;
}
static void select_stats(const SelectStage& S, const unsigned long long* ctr, livo_vis_stats* stats) {
    stats->n_in = S.V.cloud.n;
    stats->in_frame = (int64_t)ctr[kVisCtrInFrame];
    stats->behind_in_frame = (int64_t)ctr[kVisCtrBehind];
    stats->cell_overflow = (int64_t)ctr[kVisCtrOverflow];
    stats->n_out = (int64_t)ctr[kVisCtrOut];
    stats->n_cells = S.length;
}

int livo_vio_select(livo_ctx* c, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                    int32_t grid_size, const uint8_t* gray, int32_t width, int32_t height, livo_vis_point* out,
                    float* patches, int64_t cap, int64_t* n_out, livo_vis_stats* stats) {
    if (!c || !state || !p || !n_out) return LIVO_E_INVALID;
    if (cap < 0 || (out ? !patches : cap != 0)) return LIVO_E_INVALID;
    SelectStage S;
    RC_TRY(select_prepare(c, scan_id, state, p, grid_size, width, height,
                          gray || image_reusable(c->gray_img, width, height), &S));
    VisParams& V = S.V;
    const int64_t n = V.cloud.n;
    if (set_device(c)) return LIVO_E_HIP;
    if (gray) RC_TRY(image_stage(c->gray_img, gray, (size_t)width * (size_t)height, c->stream));
    const int pst3 = S.pst3;
    auto layout = [&](Carve k) {
        select_layout(S, k);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&c->vis_buf, &c->vis_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)c->vis_buf});
    unsigned long long ctr[kVisCtrN] = {0, 0, 0, 0};
    RC_TRY(select_queue(c, S, c->gray_img.p, out != nullptr));
    if (n > 0) HIP_TRY(hipMemcpyAsync(ctr, V.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (gray) {  // the upload is done: later calls may reuse it
        c->gray_img.w = width;
        c->gray_img.h = height;
    }
    const int64_t sel = (int64_t)ctr[kVisCtrOut];
    *n_out = sel;
    if (stats) select_stats(S, ctr, stats);
    if (out && cap < sel) return LIVO_E_CAPACITY;
    if (out && sel > 0) {
        HIP_TRY(hipMemcpyAsync(out, V.out, (size_t)sel * sizeof(livo_vis_point), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(patches, V.patches, (size_t)sel * pst3 * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return LIVO_OK;
}

int livo_vmap_reset(livo_ctx* c, int64_t max_points, int64_t max_frames, int32_t patch_size) {
    if (!c || max_points < 1 || max_frames < 1 || patch_size < 1 || patch_size > 8) return LIVO_E_INVALID;
    if (max_points > (int64_t)0x7FFFFFFF / kVmMaxObs || max_frames > (int64_t)0x7FFFFFFF - kVmBlock)
        return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    VmapDev& m = c->vmap;
    m.ready = false;
    const size_t pst3 = (size_t)3 * patch_size * patch_size;
    VmStore D{};
    VmFrame* frame;
    auto layout = [&](Carve k) {
        D.pt = k.take<VmPoint>((size_t)max_points);
        D.obs = k.take<VmObs>((size_t)max_points * kVmMaxObs);
        D.patch = k.take<float>((size_t)max_points * kVmMaxObs * pst3);
        D.frame = frame = k.take<VmFrame>((size_t)max_frames);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&m.buf, &m.bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)m.buf});
    (void)frame;
    D.img = (const uint8_t*)m.img;
    m.dev = D;
    m.max_points = max_points;
    m.max_frames = max_frames;
    m.ps = patch_size;
    m.w = m.h = 0;
    m.n_obs = 0;
    m.count.clear();
    m.frames.clear();
    m.free_slots.clear();
    m.ready = true;
    return LIVO_OK;
}

static int vmap_frame_slot(const VmapDev& m, int32_t frame_id) {
    if (frame_id < 0) return -1;  // (a released slot holds id -1)
    for (size_t k = 0; k < m.frames.size(); k++)
        if (m.frames[k].id == frame_id) return (int)k;
    return -1;
}

// livo_vmap_add_frame's checks (cam = frame_cam(p, state): only its intrinsics are tested).
static int frame_check(const VmapDev& m, const FrameCam& cam, int32_t width, int32_t height) {
    if (cam.distortion) return LIVO_E_INVALID;
    if (!m.frames.empty() && (width != m.w || height != m.h || cam.fx != m.K.fx || cam.fy != m.K.fy ||
                              cam.cx != m.K.cx || cam.cy != m.K.cy))
        return LIVO_E_INVALID;
    return LIVO_OK;
}
// The slot the next frame takes (a released one before a fresh one) and, before the first
// frame, the image store sized by it.  The caller has checked the capacity.
static int frame_take_slot(livo_ctx* c, const FrameCam& cam, int32_t width, int32_t height, int* slot) {
    VmapDev& m = c->vmap;
    if (m.frames.empty()) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        RC_TRY(ensure_dev_bytes(&m.img, &m.img_bytes, (size_t)width * (size_t)height * (size_t)m.max_frames));
        m.dev.img = (const uint8_t*)m.img;
        m.w = width;
        m.h = height;
        m.K = cam;
    }
    *slot = m.free_slots.empty() ? (int)m.frames.size() : m.free_slots.back();
    return LIVO_OK;
}
// The host's copy after the frame's image and VmFrame are in `slot`.
static void frame_commit(VmapDev& m, int slot, const VmFrame& f) {
    if (slot == (int)m.frames.size()) {
        m.frames.push_back(f);
    } else {
        m.free_slots.pop_back();
        m.frames[(size_t)slot] = f;
    }
    m.dev.n_frames = (int32_t)m.frames.size();
}

int livo_vmap_add_frame(livo_ctx* c, int32_t frame_id, const livo_state* state, const livo_vio_params* p,
                        const uint8_t* gray, int32_t width, int32_t height) {
    if (!c || !state || !p || frame_id < 0 || width <= 0 || height <= 0) return LIVO_E_INVALID;
    VmapDev& m = c->vmap;
    if (!m.ready || width != p->cam.width || height != p->cam.height) return LIVO_E_INVALID;
    const FrameCam cam = frame_cam(*p, *state);
    RC_TRY(frame_check(m, cam, width, height));
    if (!gray && !image_reusable(c->gray_img, width, height)) return LIVO_E_INVALID;
    if (vmap_frame_slot(m, frame_id) >= 0) return LIVO_E_INVALID;
    if (m.live_frames() >= m.max_frames) return LIVO_E_CAPACITY;
    if (set_device(c)) return LIVO_E_HIP;
    const size_t bytes = (size_t)width * (size_t)height;
    int slot;
    RC_TRY(frame_take_slot(c, cam, width, height, &slot));
    const VmFrame f = vm_make_frame(frame_id, cam);
    uint8_t* dst = (uint8_t*)m.img + (size_t)slot * bytes;
    HIP_TRY(hipMemcpyAsync(dst, gray ? gray : c->gray_img.p, bytes, gray ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync((VmFrame*)m.dev.frame + slot, &f, sizeof(f), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    frame_commit(m, slot, f);
    return LIVO_OK;
}

int livo_vmap_add(livo_ctx* c, int32_t frame_id, int64_t n, const int32_t* point_ids, const livo_vis_point* pts,
                  const int32_t* levels, const float* patches, int32_t* ids_out) {
    if (!c || n < 0 || (n > 0 && (!pts || !patches))) return LIVO_E_INVALID;
    VmapDev& m = c->vmap;
    if (!m.ready) return LIVO_E_INVALID;
    const int slot = vmap_frame_slot(m, frame_id);
    if (slot < 0) return LIVO_E_INVALID;
    if (n == 0) return LIVO_OK;
    const int64_t np0 = (int64_t)m.count.size();
    if (levels)
        for (int64_t i = 0; i < n; i++)
            if (levels[i] < 0 || levels[i] > 8) return LIVO_E_INVALID;
    // the place of every observation, on a copy of the counts: nothing is written on an error
    std::vector<int32_t> count = m.count, point((size_t)n), index((size_t)n), after((size_t)n);
    if (!point_ids) {
        if (np0 + n > m.max_points) return LIVO_E_CAPACITY;
        count.resize((size_t)(np0 + n), 0);
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t id = point_ids ? (int64_t)point_ids[i] : np0 + i;
        if (id < 0 || id >= (int64_t)count.size()) return LIVO_E_INVALID;
        if (count[(size_t)id] >= kVmMaxObs) return LIVO_E_CAPACITY;
        point[(size_t)i] = (int32_t)id;
        index[(size_t)i] = count[(size_t)id]++;
    }
    for (int64_t i = 0; i < n; i++) after[(size_t)i] = count[(size_t)point[(size_t)i]];
    std::vector<VmObs> obs((size_t)n);
    std::vector<VmPoint> fresh(point_ids ? 0 : (size_t)n);
    for (int64_t i = 0; i < n; i++) {
        obs[(size_t)i] = vm_make_obs(m.K, frame_id, slot, point_ids && levels ? levels[i] : 0, pts[i].u, pts[i].v);
        if (!point_ids) fresh[(size_t)i] = vm_make_point(pts[i]);
    }
    if (set_device(c)) return LIVO_E_HIP;
    const int pst3 = 3 * m.ps * m.ps;
    VmPutParams P{};
    VmObs* d_obs;
    float* d_pat;
    int32_t *d_point, *d_index, *d_count;
    auto layout = [&](Carve k) {
        d_obs = k.take<VmObs>((size_t)n);
        d_pat = k.take<float>((size_t)n * pst3);
        d_point = k.take<int32_t>((size_t)n);
        d_index = k.take<int32_t>((size_t)n);
        d_count = k.take<int32_t>((size_t)n);
        return k.total();
    };
    RC_TRY(ensure_scratch(c, layout(Carve{nullptr})));
    layout(Carve{(char*)c->scratch});
    HIP_TRY(hipMemcpyAsync(d_obs, obs.data(), (size_t)n * sizeof(VmObs), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_pat, patches, (size_t)n * pst3 * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_point, point.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_index, index.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_count, after.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (!point_ids)
        HIP_TRY(hipMemcpyAsync(m.dev.pt + np0, fresh.data(), (size_t)n * sizeof(VmPoint), hipMemcpyHostToDevice,
                               c->stream));
    P.map = m.dev;
    P.n = (int32_t)n;
    P.pst3 = pst3;
    P.obs = d_obs;
    P.patches = d_pat;
    P.point = d_point;
    P.index = d_index;
    P.count = d_count;
    RC_TRY(launch_vm_put(P, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.count.swap(count);
    m.n_obs += n;
    m.dev.n_points = (int32_t)m.count.size();
    if (ids_out && !point_ids)
        for (int64_t i = 0; i < n; i++) ids_out[i] = (int32_t)(np0 + i);
    return LIVO_OK;
}

int livo_vmap_info(livo_ctx* c, livo_vmap_counts* info) {
    if (!c || !info) return LIVO_E_INVALID;
    const VmapDev& m = c->vmap;
    if (!m.ready) return LIVO_E_INVALID;
    std::memset(info, 0, sizeof(*info));
    info->n_points = (int64_t)m.count.size();
    info->n_obs = m.n_obs;
    info->n_frames = m.live_frames();
    info->max_points = m.max_points;
    info->max_frames = m.max_frames;
    info->patch_size = m.ps;
    info->width = m.w;
    info->height = m.h;
    return LIVO_OK;
}

int livo_vmap_dump(livo_ctx* c, livo_vmap_point* points, int64_t cap_points, livo_vmap_obs* obs, float* patches,
                   int64_t cap_obs, int64_t* n_points, int64_t* n_obs) {
    if (!c || !n_points || !n_obs || cap_points < 0 || cap_obs < 0) return LIVO_E_INVALID;
    const VmapDev& m = c->vmap;
    if (!m.ready) return LIVO_E_INVALID;
    const int64_t np = (int64_t)m.count.size();
    *n_points = np;
    *n_obs = m.n_obs;
    if (!points && !obs && !patches) return LIVO_OK;
    if ((points && cap_points < np) || ((obs || patches) && cap_obs < m.n_obs)) return LIVO_E_RANGE;
    if (np == 0) return LIVO_OK;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t pst3 = (size_t)3 * m.ps * m.ps;
    std::vector<VmPoint> pt((size_t)np);
    std::vector<VmObs> ob((size_t)np * kVmMaxObs);
    HIP_TRY(hipMemcpy(pt.data(), m.dev.pt, pt.size() * sizeof(VmPoint), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ob.data(), m.dev.obs, ob.size() * sizeof(VmObs), hipMemcpyDeviceToHost));
    int64_t at = 0;
    for (int64_t i = 0; i < np; i++) {
        const int cnt = m.count[(size_t)i];
        if (pt[(size_t)i].n_obs != cnt) return LIVO_E_HIP;
        if (points) {
            livo_vmap_point& q = points[i];
            std::memset(&q, 0, sizeof(q));
            std::memcpy(q.pos, pt[(size_t)i].pos, sizeof(q.pos));
            q.value = pt[(size_t)i].value;
            q.n_obs = cnt;
            std::memcpy(q.voxel, pt[(size_t)i].voxel, sizeof(q.voxel));
            q.first_obs = at;
        }
        for (int k = 0; k < cnt; k++) {
            if (obs) {
                const VmObs& o = ob[(size_t)i * kVmMaxObs + k];
                livo_vmap_obs& r = obs[at + k];
                std::memset(&r, 0, sizeof(r));
                r.frame_id = o.frame_id;
                r.level = o.level;
                std::memcpy(r.px, o.px, sizeof(r.px));
                std::memcpy(r.f, o.f, sizeof(r.f));
            }
        }
        if (patches && cnt > 0)  // a point's observations lie together
            HIP_TRY(hipMemcpy(patches + (size_t)at * pst3, m.dev.patch + (size_t)i * kVmMaxObs * pst3,
                              (size_t)cnt * pst3 * 4, hipMemcpyDeviceToHost));
        at += cnt;
    }
    return LIVO_OK;
}

// ---- livo_vio_match's body: the checks and the grid, the arrays, the launches, the statistics ----
struct MatchStage {
    VmatchParams V{};
    int64_t length = 0, np = 0;
    int pst3 = 0;
    char* clear_end = nullptr;
};
// Everything of livo_vio_match that needs no device (image_ok: there is an image to read).
static int match_prepare(livo_ctx* c, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                         int32_t grid_size, int32_t ncc_en, double ncc_thre, double outlier_threshold, int32_t width,
                         int32_t height, bool image_ok, MatchStage* M) {
    if (grid_size < 1 || p->patch_size < 2 || p->patch_size > 8 || p->patch_size % 2) return LIVO_E_INVALID;
    if (width <= 0 || height <= 0 || width != p->cam.width || height != p->cam.height) return LIVO_E_INVALID;
    VmapDev& m = c->vmap;
    if (!m.ready || p->patch_size != m.ps) return LIVO_E_INVALID;
    VmatchParams& V = M->V;
    V.cam = frame_cam(*p, *state);  // once per call
    if (V.cam.distortion) return LIVO_E_INVALID;
    if (!m.frames.empty() && (width != m.w || height != m.h)) return LIVO_E_INVALID;
    V.grid.ps = p->patch_size;
    V.grid.border = (p->patch_size / 2 + 1) * 8;
    V.grid.grid_size = grid_size;
    if ((int64_t)width - 2 * V.grid.border < grid_size || (int64_t)height - 2 * V.grid.border < grid_size)
        return LIVO_E_INVALID;
    V.grid.grid_n_height = height / grid_size;
    const int64_t length = (int64_t)(width / grid_size) * V.grid.grid_n_height;
    if (length > (int64_t)0x7FFFFFFF - kVmBlock) return LIVO_E_RANGE;
    V.grid.length = (int32_t)length;
    if (!image_ok) return LIVO_E_INVALID;
    RC_TRY(frame_cloud(c, scan_id, &V.cloud));  // in the caller's point order (iperm)
    const int64_t n = V.cloud.n;
    if (n > ((int64_t)1 << 30)) return LIVO_E_RANGE;
    M->length = length;
    M->np = (int64_t)m.count.size();
    M->pst3 = 3 * p->patch_size * p->patch_size;
    int log2 = 6;  // two slots per cloud point at least: a probe always ends
    while (((int64_t)1 << log2) < 2 * n) log2++;
    V.vset_log2 = log2;
    V.W = world_params(c, *state);
    vm_frame_pos(V.cam.Rcw, V.cam.Pcw, V.fpos);
    V.map = m.dev;
    V.ncc_en = ncc_en ? 1 : 0;
    V.ncc_thre = ncc_thre;
    V.err_thre = outlier_threshold * (double)(p->patch_size * p->patch_size);
    return LIVO_OK;
}
static void match_layout(MatchStage& M, Carve& k, int64_t max_frames) {
    VmatchParams& V = M.V;
    const size_t length = (size_t)M.length, npix = (size_t)V.cam.w * (size_t)V.cam.h;
    // cleared to 0xFF: the set, the bids, the warp owners
    V.vset = k.take<unsigned long long>((size_t)1 << V.vset_log2);
    V.bid = k.take<unsigned long long>(length);
    V.owner = k.take<uint32_t>((size_t)max_frames);
    M.clear_end = (char*)k.take<char>(0);
    // cleared to 0: the depth image, the counters
    V.depth = k.take<uint32_t>(npix);
    V.ctr = k.take<unsigned long long>(kVmCtrN);
    V.cand = k.take<int32_t>(length);
    V.keep = k.take<uint32_t>(length);
    V.slot = k.take<uint32_t>(length);
    V.rec = k.take<livo_vmatch_point>(length);
    V.cpatch = k.take<float>(length * M.pst3);
    V.out = k.take<livo_vmatch_point>(length);
    V.pos = k.take<double>(length * 3);
    V.levels = k.take<int32_t>(length);
    V.patches = k.take<float>(length * M.pst3);
}
// Queues the match of img on c->stream; store: the warped patches into the map and the
// survivors' arrays (V.ctr holds the counts).  Nothing runs on an empty map (:334).
static int match_queue(livo_ctx* c, MatchStage& M, const uint8_t* img, bool store) {
    VmatchParams& V = M.V;
    V.img = img;
    V.store = store ? 1 : 0;
    if (M.np <= 0) return LIVO_OK;
    HIP_TRY(hipMemsetAsync(V.vset, 0xFF, (size_t)(M.clear_end - (char*)V.vset), c->stream));
    HIP_TRY(hipMemsetAsync(V.depth, 0, (size_t)((char*)(V.ctr + kVmCtrN) - (char*)V.depth), c->stream));
    RC_TRY(launch_vm_cloud(V, c->stream));
    RC_TRY(launch_vm_map(V, c->stream));
    RC_TRY(launch_vm_cell(V, c->stream));
    RC_TRY(launch_vm_warp(V, c->stream));
    if (store) {  // (the cells bound the result: the survivors are written before their count is known)
        RC_TRY(scan_u32(c, V.keep, const_cast<uint32_t*>(V.slot), M.length));
        RC_TRY(launch_vm_scatter(V, c->stream));
    }
    return LIVO_OK;
}
static void match_stats(const MatchStage& M, const unsigned long long* ctr, livo_vmatch_stats* stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->n_in = M.V.cloud.n;
    stats->n_voxels = (int64_t)ctr[kVmCtrVoxels];
    stats->map_tested = (int64_t)ctr[kVmCtrTested];
    stats->in_frame = (int64_t)ctr[kVmCtrInFrame];
    stats->cell_overflow = (int64_t)ctr[kVmCtrOverflow];
    stats->cells_marked = (int64_t)ctr[kVmCtrMarked];
    stats->depth_rejected = (int64_t)ctr[kVmCtrDepth];
    stats->view_rejected = (int64_t)ctr[kVmCtrView];
    stats->ncc_rejected = (int64_t)ctr[kVmCtrNcc];
    stats->error_rejected = (int64_t)ctr[kVmCtrError];
    stats->warp_shared = (int64_t)ctr[kVmCtrShared];
    stats->warp_nan = (int64_t)ctr[kVmCtrNan];
    stats->n_out = (int64_t)ctr[kVmCtrOut];
}

int livo_vio_match(livo_ctx* c, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                   int32_t grid_size, int32_t ncc_en, double ncc_thre, double outlier_threshold,
                   const uint8_t* gray, int32_t width, int32_t height, livo_vmatch_point* out, double* pos,
                   int32_t* search_levels, float* patches, int64_t cap, int64_t* n_out, livo_vmatch_stats* stats) {
    if (!c || !state || !p || !n_out) return LIVO_E_INVALID;
    if (cap < 0 || (out ? !(pos && search_levels && patches) : cap != 0)) return LIVO_E_INVALID;
    MatchStage M;
    RC_TRY(match_prepare(c, scan_id, state, p, grid_size, ncc_en, ncc_thre, outlier_threshold, width, height,
                         gray || image_reusable(c->match_img, width, height), &M));
    VmatchParams& V = M.V;
    if (set_device(c)) return LIVO_E_HIP;
    if (gray) RC_TRY(image_stage(c->match_img, gray, (size_t)width * (size_t)height, c->stream));
    const int pst3 = M.pst3;
    auto layout = [&](Carve k) {
        match_layout(M, k, c->vmap.max_frames);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&c->vm_buf, &c->vm_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)c->vm_buf});
    unsigned long long ctr[kVmCtrN] = {};
    RC_TRY(match_queue(c, M, c->match_img.p, out != nullptr));
    if (M.np > 0) HIP_TRY(hipMemcpyAsync(ctr, V.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (gray) {  // the upload is done: later calls may reuse it
        c->match_img.w = width;
        c->match_img.h = height;
    }
    const int64_t sel = (int64_t)ctr[kVmCtrOut];
    *n_out = sel;
    if (stats) match_stats(M, ctr, stats);
    if (out && cap < sel) return LIVO_E_CAPACITY;
    if (out && sel > 0) {
        HIP_TRY(hipMemcpyAsync(out, V.out, (size_t)sel * sizeof(livo_vmatch_point), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(pos, V.pos, (size_t)sel * 24, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(search_levels, V.levels, (size_t)sel * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(patches, V.patches, (size_t)sel * pst3 * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return LIVO_OK;
}

// ---- livo_vio_observe's body: the parameter block, the host's counts, the statistics ----
// (the frame's pose, the ids and levels, rec and ctr are the caller's)
static VmObserveParams observe_params(const VmapDev& m, int slot, int32_t frame_id, int64_t n) {
    VmObserveParams P{};
    static_cast<CamIntrinsics&>(P.cam) = m.K;
    P.map = m.dev;
    P.n = (int32_t)n;
    P.ps = m.ps;
    P.border = (m.ps / 2 + 1) * 8;
    P.slot = slot;
    P.frame_id = frame_id;
    return P;
}
// The device decided the counts: the host's copy follows.
static void observe_follow(VmapDev& m, const livo_vobs_point* rec, int64_t n) {
    for (int64_t i = 0; i < n; i++) {
        int32_t& cnt = m.count[(size_t)rec[i].point_id];
        m.n_obs += (int64_t)rec[i].n_obs - cnt;
        cnt = rec[i].n_obs;
    }
}
static void observe_stats(const VmapDev& m, const unsigned long long* ctr, int64_t n, livo_vobs_stats* stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->n_in = n;
    stats->behind = (int64_t)ctr[kVoCtrBehind];
    stats->out_of_frame = (int64_t)ctr[kVoCtrOutOfFrame];
    stats->pose_flagged = (int64_t)ctr[kVoCtrPose];
    stats->pixel_flagged = (int64_t)ctr[kVoCtrPixel];
    stats->added = (int64_t)ctr[kVoCtrAdded];
    stats->deleted = (int64_t)ctr[kVoCtrDeleted];
    stats->deleted_without_add = (int64_t)ctr[kVoCtrBare];
    stats->n_obs_total = m.n_obs;
}

int livo_vio_observe(livo_ctx* c, int32_t frame_id, int64_t n, const int32_t* point_ids, const int32_t* search_levels,
                     livo_vobs_point* out, livo_vobs_stats* stats) {
    if (!c || n < 0 || (n > 0 && !point_ids)) return LIVO_E_INVALID;
    VmapDev& m = c->vmap;
    if (!m.ready) return LIVO_E_INVALID;
    const int slot = vmap_frame_slot(m, frame_id);
    if (slot < 0) return LIVO_E_INVALID;
    const int64_t np = (int64_t)m.count.size();
    if (n > np) return LIVO_E_INVALID;  // (an id twice, or one outside the map)
    std::vector<int32_t> level((size_t)n, 0);
    std::vector<uint8_t> listed((size_t)np, 0);
    for (int64_t i = 0; i < n; i++) {
        const int64_t id = point_ids[i];
        if (id < 0 || id >= np || listed[(size_t)id]) return LIVO_E_INVALID;
        listed[(size_t)id] = 1;
        if (search_levels) {
            if (search_levels[i] < 0 || search_levels[i] > 8) return LIVO_E_INVALID;
            level[(size_t)i] = search_levels[i];
        }
    }
    std::vector<livo_vobs_point> rec((size_t)n);
    unsigned long long ctr[kVoCtrN] = {};
    if (n > 0) {
        if (set_device(c)) return LIVO_E_HIP;
        VmObserveParams P = observe_params(m, slot, frame_id, n);
        const VmFrame& f = m.frames[(size_t)slot];
        std::memcpy(P.cam.Rcw, f.Rcw, sizeof(f.Rcw));
        std::memcpy(P.cam.Pcw, f.Pcw, sizeof(f.Pcw));
        std::memcpy(P.cpos, f.pos, sizeof(f.pos));
        int32_t *d_point, *d_level;
        auto layout = [&](Carve k) {
            P.ctr = k.take<unsigned long long>(kVoCtrN);
            P.rec = k.take<livo_vobs_point>((size_t)n);
            P.point = d_point = k.take<int32_t>((size_t)n);
            P.level = d_level = k.take<int32_t>((size_t)n);
            return k.total();
        };
        RC_TRY(ensure_scratch(c, layout(Carve{nullptr})));
        layout(Carve{(char*)c->scratch});
        HIP_TRY(hipMemsetAsync(P.ctr, 0, sizeof(ctr), c->stream));
        HIP_TRY(hipMemcpyAsync(d_point, point_ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_level, level.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        RC_TRY(launch_vm_observe(P, c->stream));
        HIP_TRY(hipMemcpyAsync(ctr, P.ctr, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rec.data(), P.rec, (size_t)n * sizeof(livo_vobs_point), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        observe_follow(m, rec.data(), n);
        if (out) std::memcpy(out, rec.data(), (size_t)n * sizeof(livo_vobs_point));
    }
    if (stats) observe_stats(m, ctr, n, stats);
    return LIVO_OK;
}

// LidarSelector::detect (src/lidar_selection.cpp:1024-1073) behind the image conversion: the
// stage bodies above in the order match, select, update, frame, observe, new points, over one
// carve of c->det_buf and one uploaded image.  What the host reads: the counters behind the
// select (the survivor and selected counts size the later launches), and at the end the
// update's slot, the observe's counters and records and the stored VmFrame.
int livo_vio_detect(livo_ctx* c, int32_t scan_id, int32_t frame_id, livo_state* state, const livo_state* prior,
                    const livo_vio_params* p, const livo_vdetect_params* d, const uint8_t* gray, int32_t width,
                    int32_t height, livo_vdetect_stats* stats) {
    if (!c || !state || !p || !d || !gray || frame_id < 0) return LIVO_E_INVALID;
    if (p->max_iterations < 0 || !(p->img_point_cov > 0.0)) return LIVO_E_INVALID;  // (livo_vio_update's)
    VmapDev& m = c->vmap;
    MatchStage M;
    SelectStage S;
    // addFromSparseMap reads pg_down, addSparseMap the full cloud (lidar_selection.cpp:341-344, 140)
    const int32_t match_id =
        scan_id == LIVO_CLOUD_WORLD && c->wcloud.n >= 0 && c->wcloud.n_down >= 0 ? LIVO_CLOUD_WORLD_DOWN : scan_id;
    RC_TRY(match_prepare(c, match_id, state, p, d->grid_size, d->ncc_en, d->ncc_thre, d->outlier_threshold, width,
                         height, true, &M));
    RC_TRY(select_prepare(c, scan_id, state, p, d->grid_size, width, height, true, &S));
    RC_TRY(frame_check(m, M.V.cam, width, height));
    if (vmap_frame_slot(m, frame_id) >= 0) return LIVO_E_INVALID;
    if (m.live_frames() >= m.max_frames) return LIVO_E_CAPACITY;
    if (M.length > (int64_t)0x7FFFFFFF - 256) return LIVO_E_RANGE;  // (the update's block count)
    if (set_device(c)) return LIVO_E_HIP;
    const size_t bytes = (size_t)width * (size_t)height;
    int slot;
    RC_TRY(frame_take_slot(c, M.V.cam, width, height, &slot));
    RC_TRY(image_stage(c->det_img, gray, bytes, c->stream));
    const int pst3 = M.pst3;
    const size_t cells = (size_t)M.length;  // bounds the survivors and, as S.length, the selected
    VioParams U = update_params(p, width, height);
    VmObserveParams O = observe_params(m, slot, frame_id, 0);
    auto layout = [&](Carve k) {
        match_layout(M, k, m.max_frames);
        select_layout(S, k);
        U.partial = k.take<double>((cells + 255) / 256 * kVioCols + kVioCols);
        U.perr = k.take<float>(cells);
        U.slot = k.take<VioSlot>(1);
        O.ctr = k.take<unsigned long long>(kVoCtrN);
        O.rec = k.take<livo_vobs_point>(cells);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&c->det_buf, &c->det_bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)c->det_buf});
    VioSlot hs;
    std::memset(&hs, 0, sizeof(hs));
    hs.state = *state;
    hs.prior = prior ? *prior : *state;
    HIP_TRY(hipMemcpyAsync(U.slot, &hs, sizeof(hs), hipMemcpyHostToDevice, c->stream));
    // 1, 2: the match and the select at the state given, on the one image
    RC_TRY(match_queue(c, M, c->det_img.p, true));
    RC_TRY(select_queue(c, S, c->det_img.p, true));
    unsigned long long mctr[kVmCtrN] = {}, sctr[kVisCtrN] = {}, octr[kVoCtrN] = {};
    if (M.np > 0) HIP_TRY(hipMemcpyAsync(mctr, M.V.ctr, sizeof(mctr), hipMemcpyDeviceToHost, c->stream));
    if (S.V.cloud.n > 0) HIP_TRY(hipMemcpyAsync(sctr, S.V.ctr, sizeof(sctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int64_t n_s = (int64_t)mctr[kVmCtrOut], n_new = (int64_t)sctr[kVisCtrOut], np0 = M.np;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        match_stats(M, mctr, &stats->match);
        select_stats(S, sctr, &stats->select);
        stats->n_matched = n_s;
        stats->n_new = n_new;
        stats->first_new_id = n_new > 0 ? (int32_t)np0 : -1;
    }
    if (np0 + n_new > m.max_points) {  // (livo_vmap_add's; the match has rewarped)
        if (m.frames.empty()) m.w = m.h = 0;  // no first frame after all
        return LIVO_E_CAPACITY;
    }
    // 3: the update on the survivors where the scatter left them
    U.img = c->det_img.p;
    U.n = (int32_t)n_s;
    U.pos = M.V.pos;
    U.levels = M.V.levels;
    U.patches = M.V.patches;
    U.nblk = (int)std::max<int64_t>(1, (n_s + 255) / 256);
    RC_TRY(update_queue(c, U));
    // 4: the frame of the updated state (the state given if nothing matched: the update leaves it)
    VmFrame* d_frame = (VmFrame*)m.dev.frame + slot;
    VmFrameParams F{};
    F.dst = d_frame;
    F.state = &U.slot->state;
    F.vio = *p;
    F.frame_id = frame_id;
    RC_TRY(launch_vm_frame(F, c->stream));
    HIP_TRY(hipMemcpyAsync((uint8_t*)m.img + (size_t)slot * bytes, c->det_img.p, bytes, hipMemcpyDeviceToDevice,
                           c->stream));
    // 5: the observe on the match's records (one point per cell, ids from the map: no id twice)
    std::vector<livo_vobs_point> rec((size_t)n_s);
    if (n_s > 0) {
        O.n = (int32_t)n_s;
        O.match = M.V.out;
        HIP_TRY(hipMemsetAsync(O.ctr, 0, sizeof(octr), c->stream));
        RC_TRY(launch_vm_observe_resident(O, c->stream));
        HIP_TRY(hipMemcpyAsync(octr, O.ctr, sizeof(octr), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(rec.data(), O.rec, (size_t)n_s * sizeof(livo_vobs_point), hipMemcpyDeviceToHost,
                               c->stream));
    }
    // 6: the selected points, behind the observe: their ids are beyond those it was given
    if (n_new > 0) {
        VmFreshParams N{};
        N.map = m.dev;
        N.K = m.K;
        N.n = (int32_t)n_new;
        N.pst3 = pst3;
        N.frame_id = frame_id;
        N.slot = slot;
        N.base = (int32_t)np0;
        N.pts = S.V.out;
        N.patches = S.V.patches;
        RC_TRY(launch_vm_fresh(N, c->stream));
    }
    VmFrame f;
    HIP_TRY(hipMemcpyAsync(&hs, U.slot, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&f, d_frame, sizeof(f), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_s > 0) *state = hs.state;
    frame_commit(m, slot, f);
    observe_follow(m, rec.data(), n_s);
    if (stats) {
        update_stats(hs, &stats->update);
        observe_stats(m, octr, n_s, &stats->observe);
    }
    m.count.resize((size_t)(np0 + n_new), 1);
    m.n_obs += n_new;
    m.dev.n_points = (int32_t)m.count.size();
    return LIVO_OK;
}

// The frames no observation names are released: their slots go to the next frames stored.
int livo_vmap_release_frames(livo_ctx* c, int32_t* released, int64_t cap, int64_t* n_out) {
    if (!c || !n_out || cap < 0 || (!released && cap != 0)) return LIVO_E_INVALID;
    VmapDev& m = c->vmap;
    if (!m.ready) return LIVO_E_INVALID;
    *n_out = 0;
    const size_t n_slots = m.frames.size();
    if (n_slots == 0) return LIVO_OK;
    if (n_slots > (size_t)65535 * kVmRefTile) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    RC_TRY(ensure_scratch(c, n_slots * sizeof(uint32_t)));
    uint32_t* d_refs = (uint32_t*)c->scratch;
    std::vector<uint32_t> refs(n_slots);
    HIP_TRY(hipMemsetAsync(d_refs, 0, n_slots * sizeof(uint32_t), c->stream));
    RC_TRY(launch_vm_frame_refs(m.dev, (int32_t)n_slots, d_refs, c->stream));
    HIP_TRY(hipMemcpyAsync(refs.data(), d_refs, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<std::pair<int32_t, int32_t>> idle;  // (frame id, slot)
    for (size_t k = 0; k < n_slots; k++)
        if (m.frames[k].id >= 0 && refs[k] == 0u) idle.emplace_back(m.frames[k].id, (int32_t)k);
    std::sort(idle.begin(), idle.end());
    *n_out = (int64_t)idle.size();
    if (!released) return LIVO_OK;  // the sizing form
    if (cap < (int64_t)idle.size()) return LIVO_E_CAPACITY;
    for (size_t i = 0; i < idle.size(); i++) {
        released[i] = idle[i].first;
        m.frames[(size_t)idle[i].second].id = -1;
        m.free_slots.push_back(idle[i].second);
    }
    std::sort(m.free_slots.begin(), m.free_slots.end(), std::greater<int32_t>());
    return LIVO_OK;
}

// ---- One LiDAR frame in one call (laser_mapping.cpp:37-284, the LIO half of Run()) ----
// The stages are the entry points' own internals with the state on the device: dst is the propagated
// state where k_imu_propagate left it (the IMU staging), then the loop's slot.  Host syncs that remain:
// the propagation's (carry, row count), the take count, the VoxelGrid bounds and voxel count (twice:
// downSizeFilterSurf, pg_down), the scan build, the loop's end (its slot comes back: the one copy of
// the state), map_incremental's counts, the publish.
int livo_lio_frame(livo_ctx* c, const livo_imu_job* job, const livo_imu_params* imu, livo_imu_carry* carry,
                   double offset_limit_ms, const livo_lio_params* p, livo_state* state, livo_state* state_propagat,
                   livo_lio_stats* stats) {
    if (!c || !job || !imu || !carry || !p || !state || !state_propagat) return LIVO_E_INVALID;
    if (job->n_imu < 0 || (job->n_imu > 0 && !job->imu)) return LIVO_E_INVALID;
    if (!std::isfinite(p->filter_size_surf) || !std::isfinite(p->match_leaf) || !(p->filter_size_map_min > 0.0))
        return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (any_inflight(c)) return LIVO_E_BUSY;  // submitted batches are collected first
    if (!c->ing.have) return LIVO_E_INVALID;
    const bool ivox = c->backend == LIVO_BACKEND_IVOX;
    if (ivox ? !c->iv.ready : (!p->first_scan && !c->has_map)) return LIVO_E_NOMAP;
    if (p->prev_scan_id >= 0 && !get_scan_q(c, p->prev_scan_id)) return LIVO_E_NOSCAN;
    livo_lio_stats S;
    std::memset(&S, 0, sizeof(S));
    S.stage = LIVO_LIO_EMPTY;
    S.scan_id = -1;
    // 1. the forward propagation; the state stays in the IMU staging
    const livo_state* dst = nullptr;
    RC_TRY(imu_propagate(c, 1, job, imu, carry, state, nullptr, 0, nullptr, true, &dst));
    // The one copy of a frame that runs no loop: the propagated state, for both outputs.
    auto finish = [&](int rc) -> int {
        if (rc) {
            c->imu.rows = 0;  // (the table's end pose never reached the host: no table)
            return rc;
        }
        std::memcpy(c->imu.rot_end, state_propagat->rot, sizeof(c->imu.rot_end));
        std::memcpy(c->imu.pos_end, state_propagat->pos, sizeof(c->imu.pos_end));
        if (stats) *stats = S;
        return LIVO_OK;
    };
    auto fetch_propagated = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(state, dst, sizeof(livo_state), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(stream_wait(c->stream));
        *state_propagat = *state;
        return LIVO_OK;
    };
    // 2. the slice, the de-skew against the device's end pose, downSizeFilterSurf
    std::vector<livo_raw_point> down;
    int32_t id = -1;
    {
        const int64_t left = c->ing.info.n_kept - c->ing.info.cursor;
        if (p->first_scan) down.resize((size_t)std::max<int64_t>(left, 1));
        const int rc = frame_take(c, offset_limit_ms, 1, p->filter_size_surf, &id, nullptr,
                                  p->first_scan ? down.data() : nullptr, (int64_t)down.size(), &S.n_down, &S.n_taken, dst);
        if (rc) return finish(rc);
    }
    S.scan_id = id;
    if (S.n_taken == 0) return finish(fetch_propagated());
    // 3. the first scan builds / fills the map (through the host: once per session)
    if (p->first_scan) {
        S.stage = LIVO_LIO_FIRST_SCAN;
        int rc = fetch_propagated();  // (also the wait for `down`)
        if (!rc && S.n_down > 5) {
            const float* xyz = reinterpret_cast<const float*>(down.data());
            rc = ivox ? livo_ivox_add_points(c, xyz, S.n_down, sizeof(livo_raw_point))
                      : livo_map_build(c, xyz, S.n_down, sizeof(livo_raw_point));
            if (!rc) S.map_built = 1;
        }
        return finish(rc);
    }
    // 4. the facade's adopt_scan
    if (p->prev_scan_id >= 0) {
        int rc = ivox ? livo_scan_inherit_neighbors(c, id, p->prev_scan_id) : LIVO_OK;
        if (!rc) rc = livo_scan_release(c, p->prev_scan_id);
        if (rc) return finish(rc);
    }
    // 5. the IEKF loop: its slot staged from dst on the device, its end the one copy of the state
    if (p->ekf_inited) {
        const int rc = batch_update(c, 1, &id, kModelLaserMapping, state, nullptr, &S.iter, nullptr, nullptr, dst);
        if (rc) return finish(rc);
        const BatchPlan& P = c->lane[0].plan;
        if (hslot(P, 0).ctrl.n_evals > 0) {
            *state_propagat = hslot(P, 0).prior;
            dst = &dslot(P, 0)->state;
        } else {
            // no evaluation ran (an empty scan: not reachable with n_taken > 0), so nothing wrote the slot
            // back: the chain returns its input, the propagated state
            const int rc2 = fetch_propagated();
            if (rc2) return finish(rc2);
            std::memset(&S.iter, 0, sizeof(S.iter));
        }
    }
    // 6. map_incremental and 7. the publish at the state on the device
    int rc = map_incremental(c, id, nullptr, dst, p->filter_size_map_min, p->ekf_inited, nullptr, S.map_counts);
    if (!rc) rc = cloud_publish(c, p->dense_map_en ? -1 : id, nullptr, dst, p->match_leaf, &S.cloud);
    if (!rc && !p->ekf_inited) rc = fetch_propagated();
    if (rc) return finish(rc);
    S.stage = LIVO_LIO_UPDATED;
    return finish(LIVO_OK);
}

// ---- Loop search: the resident STD database and SearchLoop (include/STD/STDesc.cpp:299-374, :960-1280) ----
int livo_std_params_default(livo_std_params* p) {
    if (!p) return LIVO_E_INVALID;
    p->skip_near_num = 50;  // read_parameters, STDesc.cpp:83-93
    p->candidate_num = 50;
    p->rough_dis_threshold = 0.01;
    p->vertex_diff_threshold = 0.5;
    p->icp_threshold = 0.5;
    p->normal_threshold = 0.2;
    p->dis_threshold = 0.5;
    return LIVO_OK;
}

static bool std_params_ok(const livo_std_params* p) {
    if (!p || p->skip_near_num < 0 || p->candidate_num < 0 || p->candidate_num > LIVO_STD_MAX_CANDIDATES) return false;
    const double t[5] = {p->rough_dis_threshold, p->vertex_diff_threshold, p->icp_threshold, p->normal_threshold,
                         p->dis_threshold};
    for (double v : t)
        if (!std::isfinite(v) || v < 0.0) return false;
    return true;
}

constexpr int64_t kStdMaxCount = (int64_t)0x7FFFFFFF - 1024;

int livo_std_reset(livo_ctx* c, const livo_std_params* p, int64_t max_descs, int64_t max_frames, int64_t max_planes) {
    if (!c || !std_params_ok(p) || max_descs < 1 || max_frames < 1 || max_planes < 1) return LIVO_E_INVALID;
    if (max_frames > LIVO_STD_MAX_FRAMES || max_descs > kStdMaxCount || max_planes > kStdMaxCount) return LIVO_E_RANGE;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (set_device(c)) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    HIP_TRY(stream_wait(c->stream));  // a commit may still be writing the arrays this replaces
    D.ready = D.staged = D.searched = false;
    StdParams& P = D.P;
    P = StdParams{};
    const size_t nd = (size_t)max_descs, nf = (size_t)max_frames;
    auto layout = [&](Carve k) {
        D.hot = k.take<StdHot>(nd);
        D.verts = k.take<StdVerts>(nd);
        for (int b = 0; b < 2; b++) {
            D.skey[b] = k.take<unsigned long long>(nd);
            D.sseq[b] = k.take<uint32_t>(nd);
        }
        D.planes = k.take<livo_std_plane>((size_t)max_planes);
        D.d_plane_off = k.take<uint32_t>(nf + 1);
        P.votes = k.take<uint32_t>(nf);
        P.cand_of_frame = k.take<int32_t>(nf);
        P.coff = k.take<uint32_t>(LIVO_STD_MAX_CANDIDATES + 1);
        P.cands = k.take<livo_std_candidate>(LIVO_STD_MAX_CANDIDATES);
        P.vote_list = k.take<uint32_t>((size_t)LIVO_STD_MAX_CANDIDATES * kStdSamples);
        P.sample_rt = k.take<double>((size_t)LIVO_STD_MAX_CANDIDATES * kStdSamples * 12);
        P.n_succ = k.take<uint32_t>(LIVO_STD_MAX_CANDIDATES);
        P.ctr = k.take<unsigned>(kStdCtrN);
        P.result = k.take<livo_std_result>(1);
        return k.total();
    };
    RC_TRY(ensure_dev_bytes(&D.buf, &D.bytes, layout(Carve{nullptr})));
    layout(Carve{(char*)D.buf});
    HIP_TRY(hipMemsetAsync(D.d_plane_off, 0, 4, c->stream));
    D.prm = *p;
    D.max_descs = max_descs;
    D.max_frames = max_frames;
    D.max_planes = max_planes;
    D.n_descs = D.n_planes = D.cells = 0;
    D.n_frames = 0;
    D.cur = 0;
    D.cells_known = true;
    D.plane_off.assign(1, 0u);
    D.n_cand = 0;
    D.n_matches = 0;
    D.ready = true;
    return LIVO_OK;
}

// The staged frame's buffers for n descriptors and m planes (livo_std_stage, livo_std_generate).
static int std_stage_layout(livo_ctx* c, int64_t n, int64_t m) {
    StdDev& D = c->stdb;
    const size_t nn = (size_t)std::max<int64_t>(n, 1), mm = (size_t)std::max<int64_t>(m, 1);
    auto layout = [&](Carve k) {
        D.src = k.take<livo_std_desc>(nn);
        D.src_planes = k.take<livo_std_plane>(mm);
        D.nkey = k.take<unsigned long long>(nn);
        D.snkey = k.take<unsigned long long>(nn);
        D.nseq = k.take<uint32_t>(nn);
        D.snseq = k.take<uint32_t>(nn);
        D.P.cnt = k.take<uint32_t>(nn);
        D.P.off = k.take<uint32_t>(nn);
        return k.total();
    };
    const size_t need = layout(Carve{nullptr});
    if (need > D.stage_bytes) HIP_TRY(stream_wait(c->stream));  // (a commit may still read the frame it replaces)
    RC_TRY(ensure_dev_bytes(&D.stage, &D.stage_bytes, need));
    layout(Carve{(char*)D.stage});
    return LIVO_OK;
}

int livo_std_stage(livo_ctx* c, const livo_std_desc* descs, int64_t n, const livo_std_plane* planes, int64_t m) {
    if (!c || n < 0 || m < 0 || (n > 0 && !descs) || (m > 0 && !planes)) return LIVO_E_INVALID;
    if (n > kStdMaxCount || m > kStdMaxCount) return LIVO_E_RANGE;
    uint32_t id_min = 0xFFFFFFFFu, id_max = 0u;
    for (int64_t i = 0; i < n; i++) {
        const double* v = descs[i].side_length;  // the six vectors lie one behind the other
        for (int k = 0; k < 18; k++)
            if (!std::isfinite(v[k])) return LIVO_E_INVALID;
        for (int k = 0; k < 3; k++)
            if (std::fabs(v[k]) >= (double)(kStdCellBias - 2)) return LIVO_E_RANGE;
        id_min = std::min(id_min, descs[i].frame_id);
        id_max = std::max(id_max, descs[i].frame_id);
    }
    for (int64_t i = 0; i < m; i++)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(planes[i].xyz[k]) || !std::isfinite(planes[i].normal[k])) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    D.staged = D.searched = false;
    RC_TRY(std_stage_layout(c, n, m));
    if (n > 0) HIP_TRY(hipMemcpyAsync(D.src, descs, (size_t)n * sizeof(livo_std_desc), hipMemcpyHostToDevice, c->stream));
    if (m > 0)
        HIP_TRY(hipMemcpyAsync(D.src_planes, planes, (size_t)m * sizeof(livo_std_plane), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(stream_wait(c->stream));  // host pointers are read before return
    D.n_src = n;
    D.n_src_planes = m;
    D.id_min = id_min;
    D.id_max = id_max;
    D.staged = true;
    c->sgen.have = false;
    return LIVO_OK;
}

// The search's parameter block over the database as it stands.
static StdParams std_search_params(StdDev& D) {
    StdParams P = D.P;
    P.prm = D.prm;
    P.hot = D.hot;
    P.verts = D.verts;
    P.skey = D.skey[D.cur];
    P.sseq = D.sseq[D.cur];
    P.n_db = D.n_descs;
    P.n_frames = D.n_frames;
    P.planes = D.planes;
    P.plane_off = D.d_plane_off;
    P.src = D.src;
    P.n_src = (int32_t)D.n_src;
    P.src_planes = D.src_planes;
    P.n_src_planes = (int32_t)D.n_src_planes;
    return P;
}

int livo_std_search(livo_ctx* c, livo_std_result* out, livo_std_pair* pairs, int64_t cap, int64_t* n_pairs) {
    if (!c || !out || cap < 0) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready || !D.staged) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    D.searched = false;
    D.n_cand = 0;
    D.n_matches = 0;
    livo_std_result R{};
    R.frame = R.candidate = -1;
    R.rot[0] = R.rot[4] = R.rot[8] = 1.0;
    if (n_pairs) *n_pairs = 0;
    if (D.n_src > 0 && D.n_frames > 0) {  // (:304: no descriptors, no search; an empty database holds no match)
        StdParams P = std_search_params(D);
        const size_t nf = (size_t)D.n_frames;
        HIP_TRY(hipMemsetAsync(P.votes, 0, nf * 4, c->stream));
        HIP_TRY(hipMemsetAsync(P.cand_of_frame, 0xFF, nf * 4, c->stream));
        RC_TRY(launch_std_match(P, false, c->stream));
        RC_TRY(scan_u32(c, P.cnt, P.off, D.n_src));
        RC_TRY(launch_std_rank(P, c->stream));
        unsigned h[2];
        HIP_TRY(hipMemcpyAsync(h, P.ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(stream_wait(c->stream));  // wait 1: the match total sizes the arrays and launches below
        const int64_t total = h[kStdCtrTotal];
        const int32_t n_cand = (int32_t)h[kStdCtrCands];
        R.n_candidates = n_cand;
        if (n_cand > 0) {
            uint32_t *smkey, *smval;
            auto layout = [&](Carve k) {
                P.matches = k.take<livo_std_pair>((size_t)total);
                P.mkey = k.take<uint32_t>((size_t)total);
                P.mval = k.take<uint32_t>((size_t)total);
                smkey = k.take<uint32_t>((size_t)total);
                smval = k.take<uint32_t>((size_t)total);
                P.succ = k.take<livo_std_pair>((size_t)total);
                return k.total();
            };
            RC_TRY(ensure_dev_bytes(&D.mbuf, &D.mbytes, layout(Carve{nullptr})));
            layout(Carve{(char*)D.mbuf});
            P.sval = smval;
            RC_TRY(launch_std_match(P, true, c->stream));
            RC_TRY(launch_std_keys(P, total, c->stream));
            RC_TRY(sort_u32(c, P.mkey, smkey, P.mval, smval, total, 7));
            RC_TRY(launch_std_verify(P, n_cand, c->stream));
            D.cands.resize((size_t)n_cand);
            D.coff.resize((size_t)n_cand + 1);
            HIP_TRY(hipMemcpyAsync(&R, P.result, sizeof(R), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(D.cands.data(), P.cands, (size_t)n_cand * sizeof(livo_std_candidate),
                                   hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(D.coff.data(), P.coff, ((size_t)n_cand + 1) * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(stream_wait(c->stream));  // wait 2: the result
            D.P.matches = P.matches;
            D.P.sval = P.sval;
            D.n_matches = total;
            D.n_cand = n_cand;
            if (R.frame >= 0 && pairs && R.n_pairs > 0) {
                const int64_t k = std::min<int64_t>(cap, R.n_pairs);
                if (k > 0) {
                    HIP_TRY(hipMemcpyAsync(pairs, P.succ + D.coff[(size_t)R.candidate], (size_t)k * sizeof(livo_std_pair),
                                           hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(stream_wait(c->stream));  // wait 3, only with a loop whose pairs are asked for
                }
            }
        }
    }
    if (n_pairs) *n_pairs = R.n_pairs;
    *out = R;
    D.searched = true;
    return LIVO_OK;
}

int livo_std_commit(livo_ctx* c, int32_t* frame) {
    if (!c) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready || !D.staged) return LIVO_E_INVALID;
    if (D.n_src > 0 && (D.id_min != D.id_max || D.id_min != (uint32_t)D.n_frames)) return LIVO_E_INVALID;
    if (D.n_frames + 1 > D.max_frames || D.n_descs + D.n_src > D.max_descs || D.n_planes + D.n_src_planes > D.max_planes)
        return LIVO_E_CAPACITY;
    if (set_device(c)) return LIVO_E_HIP;
    StdCommit K{};
    K.src = D.src;
    K.n = D.n_src;
    K.n0 = D.n_descs;
    K.src_planes = D.src_planes;
    K.m = D.n_src_planes;
    K.p0 = D.n_planes;
    K.frame = D.n_frames;
    K.hot = D.hot;
    K.verts = D.verts;
    K.planes = D.planes;
    K.plane_off = D.d_plane_off;
    K.nkey = D.nkey;
    K.nseq = D.nseq;
    RC_TRY(launch_std_commit(K, c->stream));
    if (D.n_src > 0) {
        RC_TRY(sort_u64(c, D.nkey, D.snkey, D.nseq, D.snseq, D.n_src));
        RC_TRY(launch_std_merge(D.skey[D.cur], D.sseq[D.cur], D.n_descs, D.snkey, D.snseq, D.n_src, D.skey[1 - D.cur],
                                D.sseq[1 - D.cur], c->stream));
        D.cur = 1 - D.cur;
        D.cells_known = false;
    }
    D.n_descs += D.n_src;
    D.n_planes += D.n_src_planes;
    D.plane_off.push_back((uint32_t)D.n_planes);
    if (frame) *frame = D.n_frames;
    D.n_frames++;
    D.searched = false;  // (the last search's lists index the arrays of the index before the merge)
    return LIVO_OK;
}

int livo_std_candidates(livo_ctx* c, livo_std_candidate* out, int64_t cap, int64_t* n) {
    if (!c || !n || cap < 0) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready || !D.searched) return LIVO_E_INVALID;
    *n = D.n_cand;
    if (!out) return LIVO_OK;
    if (cap < D.n_cand) return LIVO_E_RANGE;
    for (int32_t k = 0; k < D.n_cand; k++) out[k] = D.cands[(size_t)k];
    return LIVO_OK;
}

int livo_std_matches(livo_ctx* c, int32_t candidate, livo_std_pair* pairs, int64_t cap, int64_t* n) {
    if (!c || !n || cap < 0) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready || !D.searched || candidate < 0 || candidate >= D.n_cand) return LIVO_E_INVALID;
    const int64_t len = D.cands[(size_t)candidate].votes;
    *n = len;
    if (!pairs) return LIVO_OK;
    if (cap < len) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    std::vector<uint32_t> order((size_t)len);
    std::vector<livo_std_pair> all((size_t)D.n_matches);
    HIP_TRY(hipMemcpyAsync(order.data(), D.P.sval + D.coff[(size_t)candidate], (size_t)len * 4, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(all.data(), D.P.matches, (size_t)D.n_matches * sizeof(livo_std_pair), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(stream_wait(c->stream));
    for (int64_t j = 0; j < len; j++) pairs[j] = all[order[(size_t)j]];
    return LIVO_OK;
}

int livo_std_info_get(livo_ctx* c, livo_std_info* info) {
    if (!c || !info) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready) return LIVO_E_INVALID;
    if (!D.cells_known) {
        if (set_device(c)) return LIVO_E_HIP;
        unsigned cells = 0;
        HIP_TRY(hipMemsetAsync(D.P.ctr + kStdCtrCells, 0, 4, c->stream));
        RC_TRY(launch_std_count_cells(D.skey[D.cur], D.n_descs, D.P.ctr, c->stream));
        HIP_TRY(hipMemcpyAsync(&cells, D.P.ctr + kStdCtrCells, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(stream_wait(c->stream));
        D.cells = cells;
        D.cells_known = true;
    }
    info->frames = D.n_frames;
    info->descs = D.n_descs;
    info->planes = D.n_planes;
    info->cells = D.cells;
    info->max_descs = D.max_descs;
    info->max_frames = D.max_frames;
    info->max_planes = D.max_planes;
    info->staged_descs = D.staged ? D.n_src : -1;
    info->staged_planes = D.staged ? D.n_src_planes : -1;
    return LIVO_OK;
}

int livo_std_dump(livo_ctx* c, livo_std_desc* descs, int64_t desc_cap, int64_t* n_descs, int32_t frame,
                  livo_std_plane* planes, int64_t plane_cap, int64_t* n_planes) {
    if (!c || desc_cap < 0 || plane_cap < 0) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready || frame >= D.n_frames) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    if (n_descs) *n_descs = D.n_descs;
    if (descs && D.n_descs > 0) {
        if (desc_cap < D.n_descs) return LIVO_E_RANGE;
        RC_TRY(ensure_scratch(c, (size_t)D.n_descs * sizeof(livo_std_desc)));
        RC_TRY(launch_std_unpack(D.hot, D.verts, D.n_descs, (livo_std_desc*)c->scratch, c->stream));
        HIP_TRY(hipMemcpyAsync(descs, c->scratch, (size_t)D.n_descs * sizeof(livo_std_desc), hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(stream_wait(c->stream));
    }
    if (frame >= 0) {
        const int64_t p0 = D.plane_off[(size_t)frame], np = (int64_t)D.plane_off[(size_t)frame + 1] - p0;
        if (n_planes) *n_planes = np;
        if (planes && np > 0) {
            if (plane_cap < np) return LIVO_E_RANGE;
            HIP_TRY(hipMemcpyAsync(planes, D.planes + p0, (size_t)np * sizeof(livo_std_plane), hipMemcpyDeviceToHost,
                                   c->stream));
            HIP_TRY(stream_wait(c->stream));
        }
    }
    return LIVO_OK;
}

// ---- GenerateSTDescs on the device (include/STD/STDesc.cpp:264-297, :376-958, :1367-1415) ----
int livo_std_gen_params_default(livo_std_gen_params* p) {
    if (!p) return LIVO_E_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->voxel_size = 2.0;  // read_parameters, STDesc.cpp:57-81
    p->voxel_init_num = 10;
    p->plane_detection_thre = 0.01;
    p->plane_merge_normal_thre = 0.1;
    p->proj_image_resolution = 0.5;
    p->proj_dis_min = 0.0;
    p->proj_dis_max = 2.0;
    p->corner_thre = 10.0;
    p->maximum_corner_num = 100;
    p->non_max_suppression_radius = 2.0;
    p->descriptor_near_num = 10;
    p->descriptor_min_len = 2.0;
    p->descriptor_max_len = 50.0;
    p->std_side_resolution = 0.2;
    return LIVO_OK;
}

// LIVO_OK, or the refusal of a parameter set (livo.h lists them).
static int std_gen_params_check(const livo_std_gen_params* p) {
    if (!p) return LIVO_E_INVALID;
    const double t[11] = {p->voxel_size, p->plane_detection_thre, p->plane_merge_normal_thre, p->proj_image_resolution,
                          p->proj_dis_min, p->proj_dis_max, p->corner_thre, p->non_max_suppression_radius,
                          p->descriptor_min_len, p->descriptor_max_len, p->std_side_resolution};
    for (double v : t)
        if (!std::isfinite(v) || v < 0.0) return LIVO_E_INVALID;
    if (!(p->voxel_size > 0.0) || !(p->proj_image_resolution > 0.0) || !(p->std_side_resolution > 0.0)) return LIVO_E_INVALID;
    if (p->voxel_init_num < 0 || p->maximum_corner_num < 1) return LIVO_E_INVALID;
    if (p->descriptor_near_num < 3 || p->descriptor_near_num > LIVO_STD_GEN_MAX_NEAR) return LIVO_E_INVALID;
    const double reach = p->voxel_size * std::sqrt(17.0);
    if (reach >= 10.0) return LIVO_E_RANGE;
    if (2.0 * reach / p->proj_image_resolution + 5.0 > (double)LIVO_STD_GEN_MAX_IMAGE) return LIVO_E_RANGE;
    if (p->descriptor_max_len * 1000.0 >= (double)((1 << 21) - 1)) return LIVO_E_RANGE;
    if (p->descriptor_max_len / p->std_side_resolution >= (double)(kStdCellBias - 2)) return LIVO_E_RANGE;
    return LIVO_OK;
}

// Room for n more points behind the key cloud's; a larger allocation takes the old points over.
static int std_key_room(livo_ctx* c, int64_t n) {
    StdGenDev& G = c->sgen;
    if (G.n_key + n > kStdMaxCount) return LIVO_E_RANGE;
    const size_t need = (size_t)(G.n_key + n) * 3 * sizeof(float);
    if (need <= G.key_bytes) return LIVO_OK;
    const size_t want = std::max(need, G.key_bytes * 2);
    float* fresh = nullptr;
    if (hipMalloc((void**)&fresh, want) != hipSuccess) return LIVO_E_OOM;
    hipError_t e = hipSuccess;
    if (G.n_key > 0)
        e = hipMemcpyAsync(fresh, G.key, (size_t)G.n_key * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = stream_wait(c->stream);  // (a generate may still read the old points)
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        return LIVO_E_HIP;
    }
    if (G.key) (void)hipFree(G.key);
    G.key = fresh;
    G.key_bytes = want;
    return LIVO_OK;
}

int livo_std_key_add(livo_ctx* c, int32_t scan_id) {
    if (!c) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    CloudSrc S;
    RC_TRY(frame_cloud(c, scan_id, &S));
    if (S.n <= 0) return LIVO_OK;
    if (set_device(c)) return LIVO_E_HIP;
    RC_TRY(std_key_room(c, S.n));
    StdGenDev& G = c->sgen;
    RC_TRY(launch_std_gen_append(S.src, S.n, S.stride, G.key + G.n_key * 3, c->stream));
    G.n_key += S.n;
    return LIVO_OK;
}

int livo_std_key_add_host(livo_ctx* c, const float* xyz, int64_t n, int64_t stride_bytes) {
    if (!c || n < 0 || (n > 0 && !xyz) || stride_bytes < 12 || stride_bytes % 4 != 0) return LIVO_E_INVALID;
    const int64_t stride = stride_bytes / 4;
    for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(xyz[i * stride + k])) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    if (n == 0) return LIVO_OK;
    if (set_device(c)) return LIVO_E_HIP;
    RC_TRY(std_key_room(c, n));
    StdGenDev& G = c->sgen;
    float* dst = G.key + G.n_key * 3;
    if (stride == 3) {
        HIP_TRY(hipMemcpyAsync(dst, xyz, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    } else {
        HIP_TRY(hipMemcpy2DAsync(dst, 12, xyz, (size_t)stride_bytes, 12, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(stream_wait(c->stream));  // host pointers are read before return
    G.n_key += n;
    return LIVO_OK;
}

int livo_std_key_clear(livo_ctx* c) {
    if (!c) return LIVO_E_INVALID;
    c->sgen.n_key = 0;
    return LIVO_OK;
}

int livo_std_key_count(livo_ctx* c, int64_t* n) {
    if (!c || !n) return LIVO_E_INVALID;
    *n = c->sgen.n_key;
    return LIVO_OK;
}

int livo_std_generate(livo_ctx* c, const livo_std_gen_params* p, livo_std_gen_stats* stats) {
    if (!c) return LIVO_E_INVALID;
    RC_TRY(std_gen_params_check(p));
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    StdGenDev& G = c->sgen;
    if (!D.ready) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    hipStream_t st = c->stream;
    livo_std_gen_stats S{};
    StdGen g{};
    g.prm = *p;
    g.frame_id = (uint32_t)D.n_frames;
    g.pts = G.key;
    g.n = G.n_key;
    S.points = g.n;
    const double reach = p->voxel_size * std::sqrt(17.0);
    const int seg_side = (int)(2.0 * reach / (5.0 * p->proj_image_resolution) + 1.0);
    g.seg_max = seg_side * seg_side;  // (<= 256: the image side is at most LIVO_STD_GEN_MAX_IMAGE)
    auto grow = [&](int which, size_t need) -> int {
        if (need > G.bytes[which]) HIP_TRY(stream_wait(st));
        return ensure_dev_bytes(&G.buf[which], &G.bytes[which], need);
    };
    // 1. voxel keys, the stable sort by (key, input index), the voxels' runs
    {
        const size_t n = (size_t)std::max<int64_t>(g.n, 1);
        auto layout = [&](Carve k) {
            g.ctr = k.take<unsigned>(kGenCtrN);
            g.pkey = k.take<unsigned long long>(n);
            g.skey = k.take<unsigned long long>(n);
            g.piota = k.take<uint32_t>(n);
            g.sidx = k.take<uint32_t>(n);
            g.spts = k.take<float>(n * 3);
            g.head = k.take<uint32_t>(n);
            g.hpos = k.take<uint32_t>(n);
            return k.total();
        };
        G.have = false;  // (the last generate's corner list lies in the arrays this one writes)
        RC_TRY(grow(0, layout(Carve{nullptr})));
        layout(Carve{(char*)G.buf[0]});
    }
    HIP_TRY(hipMemsetAsync(g.ctr, 0, kGenCtrN * sizeof(unsigned), st));
    ScanCount heads, planes, jobs, corners, alive, survivors;
    if (g.n > 0) {
        RC_TRY(launch_std_gen_keys(g, st));
        RC_TRY(sort_u64(c, g.pkey, g.skey, g.piota, g.sidx, g.n));
        RC_TRY(launch_std_gen_heads(g, st));
        RC_TRY(scan_u32(c, g.head, g.hpos, g.n));
        RC_TRY(heads.read(g.hpos, g.head, g.n, st));
        unsigned err = 0;
        HIP_TRY(hipMemcpyAsync(&err, g.ctr + kGenCtrErr, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(stream_wait(st));
        if (err & 1u) return LIVO_E_INVALID;
        if (err & 2u) return LIVO_E_RANGE;
        g.nv = heads.sum();
    }
    S.voxels = g.nv;
    // 2.-4. planes, connections and the jobs' counts, per voxel
    if (g.nv > 0) {
        const size_t nv = (size_t)g.nv;
        auto layout = [&](Carve k) {
            g.vkey = k.take<unsigned long long>(nv);
            g.vstart = k.take<uint32_t>(nv + 1);
            g.vfirst = k.take<uint32_t>(nv);
            g.viota = k.take<uint32_t>(nv);
            g.ofirst = k.take<uint32_t>(nv);
            g.order = k.take<uint32_t>(nv);
            g.rank = k.take<uint32_t>(nv);
            g.vplane = k.take<uint32_t>(nv);
            g.vnorm = k.take<double>(nv * 3);
            g.vcen = k.take<double>(nv * 3);
            g.pflag = k.take<uint32_t>(nv);
            g.ppos = k.take<uint32_t>(nv);
            g.conn = k.take<uint32_t>(nv);
            g.cidx = k.take<uint32_t>(nv * 6);
            g.jcnt = k.take<uint32_t>(nv);
            g.jpos = k.take<uint32_t>(nv);
            return k.total();
        };
        RC_TRY(grow(1, layout(Carve{nullptr})));
        layout(Carve{(char*)G.buf[1]});
        RC_TRY(launch_std_gen_voxels(g, st));
        RC_TRY(sort_u32(c, g.vfirst, g.ofirst, g.viota, g.order, g.nv, 32));  // pin 1: the order of first appearance
        RC_TRY(launch_std_gen_planes(g, st));
        RC_TRY(scan_u32(c, g.pflag, g.ppos, g.nv));
        RC_TRY(scan_u32(c, g.jcnt, g.jpos, g.nv));
        RC_TRY(planes.read(g.ppos, g.pflag, g.nv, st));
        RC_TRY(jobs.read(g.jpos, g.jcnt, g.nv, st));
        HIP_TRY(stream_wait(st));
        S.plane_voxels = planes.sum();
        g.nj = jobs.sum();
    }
    S.jobs = g.nj;
    // 5. the jobs, their members and corners
    if (g.nj > 0) {
        const size_t nj = (size_t)g.nj;
        auto layout = [&](Carve k) {
            g.job_v = k.take<uint32_t>(nj);
            g.job_c = k.take<uint32_t>(nj);
            g.jslot = k.take<uint32_t>(nj * 27);
            g.jpts = k.take<uint32_t>(nj);
            g.ccnt = k.take<uint32_t>(nj);
            g.cpos = k.take<uint32_t>(nj);
            g.cbuf = k.take<livo_std_corner>(nj * (size_t)g.seg_max);
            return k.total();
        };
        RC_TRY(grow(2, layout(Carve{nullptr})));
        layout(Carve{(char*)G.buf[2]});
        HIP_TRY(hipMemsetAsync(g.jslot, 0, nj * 27 * 4, st));
        RC_TRY(launch_std_gen_jobs(g, st));
        RC_TRY(scan_u32(c, g.ccnt, g.cpos, g.nj));
        RC_TRY(corners.read(g.cpos, g.ccnt, g.nj, st));
        unsigned err = 0;
        HIP_TRY(hipMemcpyAsync(&err, g.ctr + kGenCtrErr, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(stream_wait(st));
        if (err & 4u) return LIVO_E_RANGE;  // (not reachable: the parameter check bounds the image)
        g.m = corners.sum();
    }
    S.corners_raw = g.m;
    // 6. suppression and the cut
    int64_t n_sup = 0;
    if (g.m > 0) {
        const size_t m = (size_t)g.m;
        auto layout = [&](Carve k) {
            g.call = k.take<livo_std_corner>(m);
            g.csup = k.take<livo_std_corner>(m);
            g.cfin = k.take<livo_std_corner>(m);
            g.alive = k.take<uint32_t>(m);
            g.apos = k.take<uint32_t>(m);
            g.cutkey = k.take<uint32_t>(m);
            g.cutval = k.take<uint32_t>(m);
            g.scutkey = k.take<uint32_t>(m);
            g.scutval = k.take<uint32_t>(m);
            g.knn = k.take<uint32_t>(m * LIVO_STD_GEN_MAX_NEAR);
            return k.total();
        };
        RC_TRY(grow(3, layout(Carve{nullptr})));
        layout(Carve{(char*)G.buf[3]});
        RC_TRY(launch_std_gen_corners(g, st));
        RC_TRY(scan_u32(c, g.alive, g.apos, g.m));
        RC_TRY(alive.read(g.apos, g.alive, g.m, st));
        RC_TRY(launch_std_gen_keep(g, st));
        HIP_TRY(stream_wait(st));
        n_sup = alive.sum();
        if ((int64_t)p->maximum_corner_num > n_sup) {  // (:603: the suppressed list as it is)
            g.k = n_sup;
            g.cfin = g.csup;
        } else {
            g.k = p->maximum_corner_num;
            RC_TRY(sort_u32(c, g.cutkey, g.scutkey, g.cutval, g.scutval, n_sup, 32));
            RC_TRY(launch_std_gen_pick(g, st));
        }
    }
    S.corners_suppressed = n_sup;
    S.corners = g.k;
    // 7. the triangles
    int64_t n_descs = 0;
    g.kf = (int32_t)std::min<int64_t>(p->descriptor_near_num, g.k);
    g.pairs = (p->descriptor_near_num - 1) * (p->descriptor_near_num - 2) / 2;
    if (g.kf >= 3) {
        g.nc = g.k * g.pairs;
        if (g.nc > kStdMaxCount) return LIVO_E_RANGE;
        S.triangles_tried = g.k * ((int64_t)(g.kf - 1) * (g.kf - 2) / 2);
        const size_t nc = (size_t)g.nc;
        auto layout = [&](Carve k) {
            g.ckey = k.take<unsigned long long>(nc);
            g.sckey = k.take<unsigned long long>(nc);
            g.cval = k.take<uint32_t>(nc);
            g.scval = k.take<uint32_t>(nc);
            g.surv = k.take<uint32_t>(nc);
            g.spos = k.take<uint32_t>(nc);
            return k.total();
        };
        RC_TRY(grow(4, layout(Carve{nullptr})));
        layout(Carve{(char*)G.buf[4]});
        RC_TRY(launch_std_gen_cands(g, st));
        RC_TRY(sort_u64(c, g.ckey, g.sckey, g.cval, g.scval, g.nc));
        RC_TRY(launch_std_gen_surv(g, st));
        RC_TRY(scan_u32(c, g.surv, g.spos, g.nc));
        RC_TRY(survivors.read(g.spos, g.surv, g.nc, st));
        HIP_TRY(stream_wait(st));
        n_descs = survivors.sum();
    } else {
        g.nc = 0;
    }
    S.descs = n_descs;
    // the products become the staged frame
    D.staged = D.searched = false;
    G.have = false;
    RC_TRY(std_stage_layout(c, n_descs, S.plane_voxels));
    g.descs_out = D.src;
    g.planes_out = D.src_planes;
    if (S.plane_voxels > 0) RC_TRY(launch_std_gen_planes_out(g, st));
    if (n_descs > 0) RC_TRY(launch_std_gen_emit(g, st));
    D.n_src = n_descs;
    D.n_src_planes = S.plane_voxels;
    D.id_min = D.id_max = g.frame_id;
    D.staged = true;
    G.last = g;
    G.have = true;
    G.n_key = 0;  // laser_mapping.cpp:1249
    if (stats) *stats = S;
    return LIVO_OK;
}

int livo_std_staged(livo_ctx* c, livo_std_desc* descs, int64_t desc_cap, int64_t* n_descs, livo_std_plane* planes,
                    int64_t plane_cap, int64_t* n_planes, livo_std_corner* corners, int64_t corner_cap,
                    int64_t* n_corners) {
    if (!c || desc_cap < 0 || plane_cap < 0 || corner_cap < 0) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    StdDev& D = c->stdb;
    if (!D.ready || !D.staged) return LIVO_E_INVALID;
    const StdGenDev& G = c->sgen;
    const int64_t nk = G.have ? G.last.k : 0;
    if (n_descs) *n_descs = D.n_src;
    if (n_planes) *n_planes = D.n_src_planes;
    if (n_corners) *n_corners = nk;
    if ((descs && desc_cap < D.n_src) || (planes && plane_cap < D.n_src_planes) || (corners && corner_cap < nk))
        return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    if (descs && D.n_src > 0)
        HIP_TRY(hipMemcpyAsync(descs, D.src, (size_t)D.n_src * sizeof(livo_std_desc), hipMemcpyDeviceToHost, c->stream));
    if (planes && D.n_src_planes > 0)
        HIP_TRY(hipMemcpyAsync(planes, D.src_planes, (size_t)D.n_src_planes * sizeof(livo_std_plane), hipMemcpyDeviceToHost,
                               c->stream));
    if (corners && nk > 0)
        HIP_TRY(hipMemcpyAsync(corners, G.last.cfin, (size_t)nk * sizeof(livo_std_corner), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(stream_wait(c->stream));
    return LIVO_OK;
}

int livo_std_gen_debug(livo_ctx* c, int32_t* voxels, int64_t voxel_cap, int64_t* n_voxels, int32_t* jobs, int64_t job_cap,
                       int64_t* n_jobs) {
    if (!c || voxel_cap < 0 || job_cap < 0) return LIVO_E_INVALID;
    if (hip_device_count() <= 0) return LIVO_E_HIP;
    const StdGenDev& G = c->sgen;
    if (!G.have) return LIVO_E_INVALID;
    const StdGen& g = G.last;
    if (n_voxels) *n_voxels = g.nv;
    if (n_jobs) *n_jobs = g.nj;
    if ((voxels && voxel_cap < g.nv) || (jobs && job_cap < g.nj)) return LIVO_E_RANGE;
    if (set_device(c)) return LIVO_E_HIP;
    const size_t nv = (size_t)g.nv, nj = (size_t)g.nj;
    std::vector<uint32_t> order(nv), rank(nv), vstart(nv + 1), vfirst(nv), vplane(nv), job_v(nj), job_c(nj), jpts(nj),
        jslot(nj * 27);
    auto down = [&](std::vector<uint32_t>& h, const uint32_t* d) {
        return h.empty() ? hipSuccess : hipMemcpyAsync(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost, c->stream);
    };
    if (nv > 0) {
        HIP_TRY(down(order, g.order));
        HIP_TRY(down(rank, g.rank));
        HIP_TRY(down(vstart, g.vstart));
        HIP_TRY(down(vfirst, g.vfirst));
        HIP_TRY(down(vplane, g.vplane));
    }
    if (nj > 0) {
        HIP_TRY(down(job_v, g.job_v));
        HIP_TRY(down(job_c, g.job_c));
        HIP_TRY(down(jpts, g.jpts));
        HIP_TRY(down(jslot, g.jslot));
    }
    HIP_TRY(stream_wait(c->stream));
    if (voxels)
        for (size_t r = 0; r < nv; r++) {
            const uint32_t v = order[r];
            voxels[r * 3] = (int32_t)vfirst[v];
            voxels[r * 3 + 1] = (int32_t)(vstart[v + 1] - vstart[v]);
            voxels[r * 3 + 2] = (int32_t)vplane[v];
        }
    if (jobs)
        for (size_t j = 0; j < nj; j++) {
            jobs[j * 30] = (int32_t)rank[job_v[j]];
            jobs[j * 30 + 1] = (int32_t)rank[job_c[j]];
            jobs[j * 30 + 2] = (int32_t)jpts[j];
            for (int s = 0; s < 27; s++) {
                const uint32_t w = jslot[j * 27 + s];
                jobs[j * 30 + 3 + s] = w ? (int32_t)rank[w - 1] + 1 : 0;
            }
        }
    return LIVO_OK;
}

int livo_sync(livo_ctx* c) {
    if (!c) return LIVO_E_INVALID;
    if (set_device(c)) return LIVO_E_HIP;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const BatchLane& B : c->lane)  // submitted batches run on their lanes' streams
        for (int k = 0; k < kMaxGroups && B.st[k]; k++) HIP_TRY(hipStreamSynchronize(B.st[k]));
    return c->up.drain();  // asynchronous uploads
}

}  // extern "C"

extern "C" int livo_debug_map_rebuilds(livo_ctx* c, int64_t out[4]) {
    if (!c || !out) return LIVO_E_INVALID;
    out[0] = c->dyn.rebuilds_sorted;
    out[1] = c->dyn.rebuilds_merged;
    out[2] = c->dyn.wide_redos;
    out[3] = c->dyn.rebuilds_fused;
    return LIVO_OK;
}
