/*
 * livo.h — C ABI of the MI355X-native LIO scan-to-map IEKF hot path.
 *
 * Drop-in boundary for FAST-LIVO's scan-to-map update.  The
 * reference has no function boundary of its own for this path: the work lives
 * in private members of LaserMapping with implicit state.  Each entry point
 * below replaces one of them (reference paths under snowflakezzz/FAST-LIVO-noted):
 *
 *   livo_map_build      ← KD_TREE::Build            include/ikd-Tree/ikd_Tree.cpp:337-348
 *                         (called at src/laser_mapping.cpp:134-142 for the first scan)
 *   livo_knn            ← KD_TREE::Nearest_Search   include/ikd-Tree/ikd_Tree.cpp:350-380
 *   livo_scan_upload    ← feats_down_body handed to h_share_model
 *                                                   src/laser_mapping.cpp:129-131
 *   livo_h_share        ← LaserMapping::h_share_model(MatrixXd&, VectorXd&)
 *                                                   include/laser_mapping.h:83,
 *                                                   src/laser_mapping.cpp:485-644
 *   livo_iekf_update    ← the IEKF loop inlined in LaserMapping::Run
 *                                                   src/laser_mapping.cpp:171-238
 *   livo_iekf_update_batch ← the same for independent scans (scan farm, §8e)
 *   livo_ivox_*         ← faster_lio::IVox, the compiled default k-NN backend
 *                                                   include/ivox3d/ivox3d.h:37-305
 *   livo_map_incremental ← LaserMapping::map_incremental (iVox and ikd-Tree branches)
 *                                                   src/laser_mapping.cpp:329-389
 *   livo_map_add_points / livo_map_delete_boxes ← KD_TREE::Add_Points / Delete_Point_Boxes
 *                                                   include/ikd-Tree/ikd_Tree.cpp:382-457, 501-521
 *   livo_vio_update     ← LidarSelector::ComputeJ / UpdateState (VIO photometric update)
 *                                                   src/lidar_selection.cpp:748-978
 *   livo_scan_preprocess ← ImuProcess::UndistortPcl (per point) + downSizeFilterSurf
 *                                                   src/IMU_Processing.cpp:340-378,
 *                                                   src/laser_mapping.cpp:129-130
 *   livo_cloud_colorize ← LaserMapping::publish_frame_world_rgb (the coloured cloud)
 *                                                   src/laser_mapping.cpp:1351-1381
 *   livo_vio_select     ← LidarSelector::addSparseMap (a frame's new visual map points)
 *   livo_vmap_*         ← feat_map, imgs_ and the features' T_f_w_ (the resident visual map)
 *   livo_vio_match      ← LidarSelector::addFromSparseMap (the visual map matched into a frame)
 *                                                   src/lidar_selection.cpp:117-221
 *   livo_std_*          ← STDescManager::SearchLoop / AddSTDescs (the loop search) and
 *                         GenerateSTDescs (livo_std_key_*, livo_std_generate)
 *                                                   include/STD/STDesc.cpp:299-374, 960-1280
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross the ABI;
 *   - every function returns int: LIVO_OK (0) or a negative LIVO_E_* code;
 *     nothing throws across the ABI (livo_error_string() explains a code);
 *   - matrices are row-major doubles (the C++ facade in
 *     fast-livo-noted_amd/host/ converts to/from Eigen-style column-major);
 *   - host pointers are read/written synchronously before return;
 *   - a livo_ctx owns one HIP stream, the device-resident map and scans, and
 *     scratch; calls on one ctx are NOT thread-safe (use one ctx per host
 *     thread / GPU, as the reference uses one LaserMapping per process).
 *   - there is no CPU fallback: every compute entry point runs on the GPU and
 *     fails with LIVO_E_HIP if no device is usable.
 */
#ifndef LIVO_H
#define LIVO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9: the resident visual map (livo_vmap_*) and livo_vio_match added (nothing else changed).
 *    livo_cloud_publish, livo_cloud_info_get and the two LIVO_CLOUD_* ids added the same way.
 *    livo_imu_* (params, init, propagate, propagate_batch) and livo_scan_preprocess_imu too.
 *    livo_ingest_params_default, livo_frame_ingest_livox / _cloud, livo_frame_info / _dump / _take too.
 *    livo_std_* (the loop search) too.
 * 8: livo_vio_select added (nothing else changed).
 * 7: livo_cloud_colorize added (nothing else changed).
 * 5: livo_ivox_info grew add_passes (round 4).
 * 4: livo_timings grew the per-evaluation fields (eval_ms ... gap_ms), LIVO_E_BUSY
 *    and the submit / wait pair were added (round 3); a binary built against 3
 *    passes a smaller livo_timings. */
#define LIVO_ABI_VERSION 9
#define LIVO_DIM_STATE 18        /* DIM_STATE, include/common_lib.h:32 */
#define LIVO_NUM_MATCH_POINTS 5  /* NUM_MATCH_POINTS, include/common_lib.h:37 */
#define LIVO_MAX_EVALS 16        /* max h_share/solve evaluations per scan update */

enum {
    LIVO_OK = 0,
    LIVO_E_INVALID = -1,   /* bad argument (null pointer, negative size, ...) */
    LIVO_E_HIP = -2,       /* HIP runtime error (no device, launch failure) */
    LIVO_E_NOMAP = -3,     /* map not built */
    LIVO_E_NOSCAN = -4,    /* unknown / released scan id */
    LIVO_E_OOM = -5,       /* device allocation failed */
    LIVO_E_RANGE = -6,     /* size beyond the supported range */
    LIVO_E_CAPACITY = -7,  /* capacity exceeded (livo_vio_select: cap below the result) */
    LIVO_E_BUSY = -8       /* batches in flight (livo_iekf_update_batch_submit) */
};

typedef struct livo_ctx livo_ctx;

/* Hot-path parameters (defaults = reference defaults, src/laser_mapping.cpp:945-1116). */
typedef struct livo_params {
    double laser_point_cov;  /* LASER_POINT_COV, laser_mapping.cpp:975 (0.001)          */
    double R_LI[9];          /* Lidar_rot_to_IMU (row-major), default identity          */
    double t_LI[3];          /* Lidar_offset_to_IMU, default 0                           */
    double max_residual;     /* compaction gate |pd2| <= 2.0, laser_mapping.cpp:552      */
    float plane_threshold;   /* esti_plane threshold 0.1f, laser_mapping.cpp:530         */
    float max_nn_sqdist;     /* k-NN gate sqdis[4] > 5 => reject, laser_mapping.cpp:518  */
    int32_t max_iterations;  /* NUM_MAX_ITERATIONS (max_iteration, default 4, :968)      */
    int32_t flags;           /* reserved, must be 0                                      */
} livo_params;

/* StatesGroup (include/common_lib.h:518-603), row-major. */
typedef struct livo_state {
    double rot[9];      /* rot_end (IMU->world)  */
    double pos[3];      /* pos_end               */
    double vel[3];      /* vel_end               */
    double bias_g[3];
    double bias_a[3];
    double gravity[3];
    double cov[LIVO_DIM_STATE * LIVO_DIM_STATE];
} livo_state;

/* Per-scan-update statistics (the reference logs these ad hoc, laser_mapping.cpp:164-238). */
typedef struct livo_iter_stats {
    int32_t iterations;   /* h_share + solve evaluations performed            */
    int32_t knn_passes;   /* evaluations with nearest_search_en               */
    int32_t converged;    /* flg_EKF_converged at exit                        */
    int32_t rematch_num;
    int64_t effct_feat_num[LIVO_MAX_EVALS];
    double solution[LIVO_MAX_EVALS][LIVO_DIM_STATE]; /* state delta per evaluation */
    double res_mean[LIVO_MAX_EVALS];                 /* res_mean_last per evaluation */
} livo_iter_stats;

typedef struct livo_map_info {
    int64_t num_points;   /* M                                                    */
    int32_t depth;        /* tree levels                                          */
    int32_t ball_chunks;  /* anchor chunks the ball runs were built in (0: none)  */
    int64_t num_slots;    /* heap-ordered node slots (2^depth - 1)                */
    int64_t device_bytes; /* HBM bytes held by the map                            */
    int64_t ball_entries; /* entries of the ball runs (0: the cell runs only)     */
} livo_map_info;

/* Optional per-point outputs of livo_h_share (any pointer may be NULL). */
typedef struct livo_point_out {
    float* normvec;       /* N*4: plane n.x,n.y,n.z and pd2 (normvec->points[i], :537-541)      */
    uint8_t* selected;    /* N:   point_selected_surf[i] && res_last[i] <= 2.0 (:552)            */
    int32_t* nn_idx;      /* N*5: map indices (input order of livo_map_build), -1 pad           */
    float* nn_sqdist;     /* N*5: squared distances (pointSearchSqDis), +inf pad                */
    float* world_xyz;     /* N*3: feats_down_world (pointBodyToWorld, :508)                      */
    int64_t* visits;      /* 1:   k-NN nodes visited over all points (the V_ref yardstick)       */
    /* laserCloudOri / corr_normvect (:547-561): the effective points (selected and
     * |pd2| <= 2), compacted in the caller's point order; capacity N each. */
    float* ori_xyz;       /* n_ori*3: body points (laserCloudOri)                                */
    float* corr_normvec;  /* n_ori*4: their plane normal and pd2 (corr_normvect)                 */
    int64_t* n_ori;       /* 1:   effct_feat_num                                                 */
} livo_point_out;

/* Device time of the kernels of the last livo_iekf_update* call (profiling mode only).
 * knn_* describe the first evaluation's k-NN of the whole batch (pilot pass +
 * pilot-seeded pass + their tie replays, both streams), in which every point of
 * every scan is searched: the dominant kernels.  The other times are summed
 * over the streams (they overlap). */
typedef struct livo_timings {
    double knn_ms;         /* first-evaluation k-NN of the batch, device wall time     */
    double rematch_knn_ms; /* k-NN launches of later evaluations (rematch)             */
    double plane_ms;       /* plane fit + Jacobian + reduction + 18x18 solve (fused)   */
    double solve_ms;       /* 0: the solve runs in the plane pass's last block         */
    int64_t knn_launches;  /* first-evaluation k-NN phases timed (1 per call)          */
    int64_t knn_visits;    /* tree nodes those searches visited (pilot-seeded: < V_ref) */
    int64_t knn_queries;   /* points those launches processed                          */
    int64_t effct_points;  /* effective points of the first evaluation                 */
    int64_t knn_replays;   /* queries recomputed by the exact tie-order replay (all passes) */
    int64_t knn_points;    /* map points those launches read (cell grid; 0 for tree passes) */
    /* level 2, fused evaluation: device time of each evaluation launch (max over
     * the stream groups) and the scans that searched in it; the batch from its
     * first copy to its last, and the device idle time since the previous
     * batch ended (host time between calls; 0 for the first profiled batch).
     * Then knn_ms = eval_ms[0], rematch_knn_ms = the evaluations after the
     * first that searched, plane_ms = those that did not. */
    double eval_ms[LIVO_MAX_EVALS];
    int32_t eval_searched[LIVO_MAX_EVALS];
    int32_t n_evals;
    int32_t reserved_;
    double batch_ms;
    double gap_ms;
} livo_timings;

int livo_abi_version(void);
const char* livo_error_string(int code);
int livo_params_default(livo_params* p);

int livo_ctx_create(int device, const livo_params* p, livo_ctx** out);
int livo_ctx_destroy(livo_ctx* ctx);
int livo_ctx_set_params(livo_ctx* ctx, const livo_params* p);
/* Device timing of livo_iekf_update* (livo_last_timings): 0 off; 1 the first
 * search of the batch only (two events per stream group); 2 also every
 * evaluation's k-NN / plane / solve stages (costs ~10% of throughput). */
int livo_ctx_set_profiling(livo_ctx* ctx, int level);
int livo_last_timings(livo_ctx* ctx, livo_timings* out);

/* Build the device map from M host points (x,y,z floats at xyz + i*stride_bytes).
 * Same tree as KD_TREE::Build on the same input order. Replaces any previous map. */
int livo_map_build(livo_ctx* ctx, const float* xyz, int64_t M, int64_t stride_bytes);
int livo_map_get_info(livo_ctx* ctx, livo_map_info* out);

/* Exact k-NN (k <= 5) of n host queries; idx/sqdist are n*k, ascending. */
int livo_knn(livo_ctx* ctx, const float* q_xyz, int64_t n, int32_t k, int32_t* idx, float* sqdist);

/* Copy a body-frame scan (feats_down_body) to HBM; it stays resident until released. */
int livo_scan_upload(livo_ctx* ctx, const float* xyz, int64_t N, int64_t stride_bytes, int32_t* scan_id);
/* livo_scan_upload without waiting for the device: the points are packed into a
 * pinned staging buffer (xyz is free again on return), then copied and ordered
 * on the context's upload stream beside the batches in flight.  A batch using
 * the scan waits for that on the device; any other call on it, on the host.
 * (The reference hands each frame's feats_down_body to h_share_model,
 * src/laser_mapping.cpp:129-131: the upload of frame k+1 can run under frame k.) */
int livo_scan_upload_async(livo_ctx* ctx, const float* xyz, int64_t N, int64_t stride_bytes, int32_t* scan_id);
/* livo_scan_upload_async for n scans in one pass (xyz[b]: N[b] points at
 * stride_bytes, scan_ids[b] out): one staging copy, then one bounds pass, one
 * key pass, one stable sort of the whole batch and one gather on the upload
 * stream; each scan is stored exactly as livo_scan_upload stores it.  From
 * page-locked memory (livo_host_register) with stride 12 the copy engine reads
 * the caller's arrays directly (no host copy): keep them unchanged until a batch
 * that uses the scans returns (or livo_sync); otherwise they are free on return. */
int livo_scan_upload_batch_async(livo_ctx* ctx, const float* const* xyz, const int64_t* N, int32_t n,
                                 int64_t stride_bytes, int32_t* scan_ids);
/* Page-lock (hipHostRegister) / release a caller's host buffer, e.g. the point
 * arrays a scan farm uploads from; unregister waits for the device first. */
int livo_host_register(livo_ctx* ctx, void* p, size_t bytes);
int livo_host_unregister(livo_ctx* ctx, void* p);
/* Release a resident scan: LIVO_E_BUSY while a submitted batch that holds it is
 * not collected; other batches may be in flight. */
int livo_scan_release(livo_ctx* ctx, int32_t scan_id);

/* The neighbour cache of a resident scan: the k = 5 nearest map points of each
 * point from the last search on it (Nearest_Points, laser_mapping.h:165, in
 * Nearest_Search's ascending PointType_CMP order, ikd_Tree.cpp:350-380).
 * idx: N x 5 map indices (-1 pad); sqdist: N x 5 (+inf pad); either may be NULL.
 * LIVO_E_NOSCAN if the scan was never searched, or if the last batched update
 * on it failed with LIVO_E_HIP after some of its launches were queued (its
 * records are then no single search's answer, see livo_iekf_update_batch).
 * Cost: after a batched update on a static map (livo_map_build, no point added or
 * deleted since) the loop's last search has stored only the records the loop itself
 * read.  The first call that reads a scan's records afterwards -- this one,
 * livo_h_share, livo_scan_inherit_neighbors, livo_map_incremental, an unfused,
 * iVox or IKFoM update of the scan, or a change of the map or backend, which
 * does it for every such scan -- runs that scan's search once more, at the pose
 * of its last search, and leaves the same records a stored search would have;
 * later calls cost nothing.  LIVO_REC_LAZY=0 (read when the context is created)
 * stores them in the loop instead. */
int livo_scan_neighbors(livo_ctx* ctx, int32_t scan_id, int32_t* idx, float* sqdist);

/* One h_share_model evaluation on a resident scan at the given state.
 * nearest_search_en != 0 runs the k-NN; otherwise the neighbours cached by the
 * last search on this scan are reused (Nearest_Points, laser_mapping.h:165).
 * HTH (9x9, row-major) and HTL (9) as HPH/HPL of the reference. */
int livo_h_share(livo_ctx* ctx, int32_t scan_id, const livo_state* state, int nearest_search_en,
                 double HTH[81], double HTL[9], int64_t* effct_feat_num, const livo_point_out* out);

/* Full iterated update of one scan (laser_mapping.cpp:171-238): state in/out,
 * prior = state_propagat (NULL: prior = input state). stats may be NULL. */
int livo_iekf_update(livo_ctx* ctx, int32_t scan_id, livo_state* state, const livo_state* prior,
                     livo_iter_stats* stats);

/* n independent scan updates in one batched pass (states/priors/stats arrays of n).
 * The ids must be distinct (LIVO_E_INVALID otherwise): a scan's neighbour cache
 * belongs to one update at a time.  An update that fails on the device side
 * (LIVO_E_HIP from a launch, a copy or the wait for its end; submit / wait
 * alike) leaves its scans without a neighbour cache, as if never searched:
 * the first search of an update stores only the records that the update's
 * second search does not rewrite.  An update refused before anything is
 * queued (bad arguments, LIVO_E_BUSY) leaves the caches as they were. */
int livo_iekf_update_batch(livo_ctx* ctx, int32_t n, const int32_t* scan_ids, livo_state* states,
                           const livo_state* priors, livo_iter_stats* stats);

/* The same batched update, split into enqueue and collect, so a scan farm keeps
 * the next batch queued on the device while the host collects the last one
 * (no replacement in the reference, which updates one scan per frame in
 * LaserMapping::Run; this is the farm of SURVEY.md §8e).  submit copies
 * states / priors (NULL: prior = state) at the call and returns a ticket;
 * wait(ticket) blocks until that batch is done and writes its states and
 * stats (may be NULL).  At most LIVO_MAX_INFLIGHT batches per context are
 * submitted and not yet waited for (LIVO_E_BUSY beyond), and a scan may be in
 * one of them only (LIVO_E_INVALID).  While a batch is in flight its scans
 * may not be released, and the map may not be rebuilt or changed (LIVO_E_BUSY),
 * and livo_scan_neighbors of one of its scans returns LIVO_E_BUSY.  submit
 * needs the fused ikd-Tree path (the default: LIVO_BACKEND_IKDTREE, no
 * LIVO_FUSED=0 / LIVO_KNN_KIND override): otherwise it returns LIVO_E_INVALID
 * before queuing anything, and livo_iekf_update_batch does the same update
 * synchronously. */
#define LIVO_MAX_INFLIGHT 2
int livo_iekf_update_batch_submit(livo_ctx* ctx, int32_t n, const int32_t* scan_ids, const livo_state* states,
                                  const livo_state* priors, int32_t* ticket);
int livo_iekf_update_batch_wait(livo_ctx* ctx, int32_t ticket, livo_state* states, livo_iter_stats* stats);

/* ------------------------------------------------------------------------
 * IKFoM formulation (the "solve in use-ikfom.hpp"):
 *   state_ikfom                         include/use-ikfom.hpp:12-21 (23 DOF)
 *   h_share_model (legacy h-model)      src/origin_laserMapping.cpp:916-1048
 *   esekf::update_iterated_dyn_share_modified
 *                                       include/IKFoM_toolkit/esekfom/esekfom.hpp:1619-1928
 * The same map, scans and k-NN as above; 12-wide measurement rows [n, A, B, C]
 * (extrinsic estimation on), the manifold (SO3 / S2) Jacobian corrections,
 * per-DOF convergence |dx_i| <= 0.001 (origin_laserMapping.cpp:1231-1233),
 * R = params.laser_point_cov, maximum_iter = params.max_iterations.
 * ------------------------------------------------------------------------ */
#define LIVO_IKFOM_DOF 23

/* state_ikfom: quaternions (w, x, y, z) for rot and offset_R_L_I, the S2
 * gravity as its 3-vector (length 98090/10000), cov = P_ (23x23 row-major). */
typedef struct livo_ikfom_state {
    double pos[3];
    double rot[4];
    double offset_R[4];
    double offset_T[3];
    double vel[3];
    double bg[3];
    double ba[3];
    double grav[3];
    double cov[LIVO_IKFOM_DOF * LIVO_IKFOM_DOF];
} livo_ikfom_state;

typedef struct livo_ikfom_stats {
    int32_t iterations;   /* h_dyn_share + update evaluations                    */
    int32_t knn_passes;   /* evaluations with dyn_share.converge (k-NN search)   */
    int32_t converged;    /* dyn_share.converge at exit                          */
    int32_t t;            /* converged-iteration counter t at exit               */
    int64_t effct_feat_num[LIVO_MAX_EVALS];
    double dx[LIVO_MAX_EVALS][LIVO_IKFOM_DOF];  /* dx_ applied per evaluation */
    double res_mean[LIVO_MAX_EVALS];
} livo_ikfom_stats;

/* The IKFoM iterated update of n resident scans, each starting from its state
 * (x_propagated = the input state, P_propagated = its cov).  stats may be NULL. */
int livo_ikfom_update_batch(livo_ctx* ctx, int32_t n, const int32_t* scan_ids, livo_ikfom_state* states,
                            livo_ikfom_stats* stats);
int livo_ikfom_update(livo_ctx* ctx, int32_t scan_id, livo_ikfom_state* state, livo_ikfom_stats* stats);
/* The IKFoM batch split into enqueue and collect, as livo_iekf_update_batch_submit
 * / _wait (the same LIVO_MAX_INFLIGHT lanes and tickets; a ticket is collected
 * with the wait of its own model). */
int livo_ikfom_update_batch_submit(livo_ctx* ctx, int32_t n, const int32_t* scan_ids, const livo_ikfom_state* states,
                                   int32_t* ticket);
int livo_ikfom_update_batch_wait(livo_ctx* ctx, int32_t ticket, livo_ikfom_state* states, livo_ikfom_stats* stats);

/* ------------------------------------------------------------------------
 * iVox backend: faster_lio::IVox<3, DEFAULT, PointType>
 * (include/laser_mapping.h:65), the k-NN backend of the reference's default
 * build (CMakeLists.txt:15 leaves USE_ikdtree undefined).  With
 * livo_ctx_set_backend(ctx, LIVO_BACKEND_IVOX), livo_h_share and
 * livo_iekf_update[_batch] search the iVox map with
 * GetClosestPoint(point_world, points_near, 5) (laser_mapping.cpp:520): no
 * sqdist gate, a point is matched iff 5 neighbours within 5 m were found
 * (:525), the neighbours are in the order the reference's std::nth_element
 * leaves them, and a point with no candidate keeps its previous
 * Nearest_Points entry (ivox3d.h:165-167).
 * ------------------------------------------------------------------------ */
#define LIVO_BACKEND_IKDTREE 0  /* -DUSE_ikdtree build (CMakeLists.txt:15)            */
#define LIVO_BACKEND_IVOX 1     /* the default build: IVox (laser_mapping.cpp:519-521) */

typedef struct livo_ivox_params {
    float resolution;     /* ivox_grid_resolution (0.2, laser_mapping.cpp:1021)          */
    int32_t nearby_type;  /* ivox_nearby_type: 0 CENTER, 6, 18 (default, :1022-1035), 26 */
    int64_t capacity;     /* Options::capacity_ (1000000, ivox3d.h:57)                   */
} livo_ivox_params;

typedef struct livo_ivox_info {
    int64_t num_points;      /* points held (IVox::NumPoints)                       */
    int64_t num_grids;       /* IVox::NumValidGrids (ivox3d.h:206-209)              */
    int64_t ids_issued;      /* points ever added = the id of the next point        */
    int64_t max_grid_points; /* largest grid                                        */
    int64_t device_bytes;    /* HBM held by the iVox map                            */
    int64_t add_passes;      /* device passes AddPoints took since init: one per    */
                             /* call, more when an LRU victim is re-touched         */
} livo_ivox_info;

int livo_ctx_set_backend(livo_ctx* ctx, int backend);
int livo_ivox_params_default(livo_ivox_params* p);
/* IVox(Options) (ivox3d.h:64-67, laser_mapping.cpp:776): an empty map. */
int livo_ivox_init(livo_ctx* ctx, const livo_ivox_params* p);
/* IVox::AddPoints (ivox3d.h:256-281) of n host points, in order (the first
 * scan's feats_down_body, laser_mapping.cpp:147), with the LRU grid cache:
 * once a new grid takes the grid count to capacity, the grid whose last added
 * point is the oldest is evicted with its points (:270-274).  Point ids
 * continue from ids_issued.  LIVO_E_RANGE (a key beyond the supported cell
 * range) leaves the map unchanged. */
int livo_ivox_add_points(livo_ctx* ctx, const float* xyz, int64_t n, int64_t stride_bytes);
/* IVox::GetClosestPoint(pt, closest_pt, max_num, max_range) (ivox3d.h:132-204)
 * for n host queries: idx / sqdist n*max_num in the reference's order (the
 * nearest first), cnt[i] = neighbours found, -1 when there was no candidate
 * (the reference returns false and leaves its output vector alone). */
int livo_ivox_knn(livo_ctx* ctx, const float* q_xyz, int64_t n, int32_t max_num, double max_range, int32_t* idx,
                  float* sqdist, int32_t* cnt);
int livo_ivox_get_info(livo_ctx* ctx, livo_ivox_info* out);
/* Every point, grid by grid in grids_cache_ order (most recently used grid
 * first, insertion order inside a grid): xyz n*3, ids n, keys n*3 (the grid
 * of each point); any may be NULL.
 * *n = points; LIVO_E_RANGE if cap < *n (nothing written). */
int livo_ivox_dump(livo_ctx* ctx, float* xyz, int32_t* ids, int32_t* keys, int64_t cap, int64_t* n);

/* LaserMapping::map_incremental, iVox branch (laser_mapping.cpp:329-389): the
 * scan's points at `state` (the updated state), the add / no-downsample / skip
 * decision from the scan's neighbour cache, then AddPoints(points_to_add) and
 * AddPoints(point_no_need_downsample) on the device.  cat (may be NULL): per
 * point 0 skipped, 1 added, 2 added without downsampling; counts[2] = the two
 * batch sizes.  ekf_inited = flg_EKF_inited.  iVox backend only. */
int livo_map_incremental(livo_ctx* ctx, int32_t scan_id, const livo_state* state, double filter_size_map_min,
                         int ekf_inited, uint8_t* cat, int64_t counts[2]);
/* Nearest_Points.resize(N) between scans (laser_mapping.cpp:165) keeps the
 * entries of the previous scan's points: dst's point i starts with src's
 * point i's cache (empty for i >= src's size). */
int livo_scan_inherit_neighbors(livo_ctx* ctx, int32_t dst_scan, int32_t src_scan);

/* ------------------------------------------------------------------------
 * Scan front-end: from the raw frame to the resident
 * feats_down_body on the device.
 *   ImuProcess::UndistortPcl, per-point backward propagation
 *                                       src/IMU_Processing.cpp:340-378
 *   downSizeFilterSurf.filter (PCL VoxelGrid)  src/laser_mapping.cpp:129-130
 * ------------------------------------------------------------------------ */
/* The PointXYZINormal fields the front-end reads; curvature = the point's
 * offset time in ms (preprocess.cpp:346). */
typedef struct livo_raw_point {
    float x, y, z, intensity, curvature;
} livo_raw_point;

/* Pose6D (msg/Pose6D.msg, set_pose6d common_lib.h:618-633): one IMU sample of
 * the frame's forward propagation, offset_time in seconds from the frame start. */
typedef struct livo_imu_pose {
    double offset_time;
    double acc[3];
    double gyr[3];
    double vel[3];
    double pos[3];
    double rot[9];  /* row-major */
} livo_imu_pose;

/* Raw frame -> resident scan.  With n_poses >= 2 every point is first moved to
 * the frame-end pose (rot_end, pos_end = state after propagation) through the
 * IMU segment it falls in, exactly as UndistortPcl's backward walk (poses must
 * have non-decreasing offset_time; the first point is re-compensated by every
 * remaining segment, as in the reference); then, for leaf_size > 0, PCL
 * VoxelGrid downsampling (voxel centroids of x, y, z, intensity, curvature in
 * ascending leaf order; a leaf too small for 32-bit indices keeps the input,
 * as PCL does).  The result becomes a resident scan (*scan_id), as
 * livo_scan_upload would.  undistorted (n) and down (down_cap; *n_down = its
 * size) are optional host copies. */
int livo_scan_preprocess(livo_ctx* ctx, const livo_raw_point* raw, int64_t n, const livo_imu_pose* poses,
                         int32_t n_poses, const double rot_end[9], const double pos_end[3], float leaf_size,
                         int32_t* scan_id, livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap,
                         int64_t* n_down);

/* ------------------------------------------------------------------------
 * VIO photometric update: LidarSelector::ComputeJ and
 * UpdateState (src/lidar_selection.cpp:748-978) for the visual points of
 * sub_sparse_map: per point, patch_size^2 bilinear residuals against its
 * reference patch at pyramid levels 2, 1, 0, the 6-wide Jacobian rows, and
 * the 18-dim iterated update (K1 = (HᵀH + (P / img_point_cov)^-1)^-1), then
 * cov -= G cov.  max_iterations is explicit: the compiled build never
 * assigns LidarSelector::NUM_MAX_ITERATIONS (the legacy pipeline sets it to
 * the LiDAR value, origin_laserMapping.cpp:1208).
 * ------------------------------------------------------------------------ */
/* vikit PinholeCamera (camera yaml: cam_fx ... cam_d0..d3; d[4] = k3). */
typedef struct livo_cam {
    double fx, fy, cx, cy;
    double d[5];
    int32_t width, height;
} livo_cam;

typedef struct livo_vio_params {
    livo_cam cam;
    double R_ci[9];          /* Rci = Rcl * Rli (lidar_selection.cpp:44), row-major */
    double P_ci[3];          /* Pci = Rcl * Pli + Pcl                                */
    double img_point_cov;    /* img_point_cov (10, laser_mapping.cpp:976)             */
    int32_t patch_size;      /* patch_size (4, laser_mapping.cpp:1015), <= 8          */
    int32_t max_iterations;  /* UpdateState iterations per level                      */
} livo_vio_params;

typedef struct livo_vio_stats {
    int32_t iterations[3];   /* per level 2, 1, 0 */
    int32_t updates[3];      /* iterations that updated the state (error did not grow) */
    float last_error[3];     /* UpdateState's return value per level */
    int32_t cov_updated;
    int64_t n_meas;
    int64_t out_of_frame;    /* patch samples outside the image (clamped; the reference reads out of bounds) */
} livo_vio_stats;

int livo_vio_params_default(livo_vio_params* p);
/* image: 8-bit gray, width x height, row stride = width.  pos: n x 3 world
 * positions; search_levels: n; patches: n x 3 x patch_size^2 reference
 * patches (levels 0, 1, 2, Feature::patch_).  state in/out, prior =
 * state_propagat (NULL: the input state).  errors (n, may be NULL) =
 * sub_sparse_map->errors after the last iteration. */
int livo_vio_update(livo_ctx* ctx, const livo_vio_params* p, const uint8_t* image, int32_t width, int32_t height,
                    const double* pos, const int32_t* search_levels, const float* patches, int64_t n,
                    livo_state* state, const livo_state* prior, float* errors, livo_vio_stats* stats);

/* ------------------------------------------------------------------------
 * ikd-Tree incremental map (the USE_ikdtree branch of
 * map_incremental, src/laser_mapping.cpp:383-384, and the ikd-Tree's
 * Delete_Point_Boxes).  The first call turns the built map (cell-grid search
 * structure, the default) into an incremental point set: ids = the build's
 * indices, then the next ids in input order for the points a call leaves in
 * the map.  Later k-NN (livo_knn, livo_h_share, the IEKF loops) search the
 * updated map; queries whose order the reference's tree shape would decide
 * (PointType_CMP ties) come in (distance, x, id) order.
 * livo_map_incremental with LIVO_BACKEND_IKDTREE runs Add_Points(world, true)
 * on the scan at the given state: counts[0] = its return value, counts[1] =
 * points deleted; cat = 1 for every point.
 * ------------------------------------------------------------------------ */
typedef struct livo_map_add_stats {
    int64_t events;     /* Add_Points' return value (tmp_counter, include/ikd-Tree/ikd_Tree.cpp:416,428) */
    int64_t added;      /* points of the call left in the map (new ids, input order)            */
    int64_t deleted;    /* map points removed (Delete_by_range of a downsample box, :414)        */
    int64_t ambiguous;  /* boxes whose kept stored point Search_by_range's order picks (ties)    */
    int64_t deferred;   /* points handled by the in-order pass (box-face rounding cases)         */
    int64_t map_points; /* points in the map after the call                                      */
} livo_map_add_stats;

/* KD_TREE::Add_Points(points, downsample_on) (ikd_Tree.cpp:382-457) with
 * downsample_size (set_downsample_param, :35-40); xyz at xyz + i*stride_bytes. */
int livo_map_add_points(livo_ctx* ctx, const float* xyz, int64_t n, int64_t stride_bytes, float downsample_size,
                        int downsample_on, livo_map_add_stats* stats);
/* KD_TREE::Delete_Point_Boxes (ikd_Tree.cpp:501-521): boxes n_boxes x 6 floats
 * {vertex_min[3], vertex_max[3]} (BoxPointType), half open; *deleted = points removed. */
int livo_map_delete_boxes(livo_ctx* ctx, const float* boxes, int64_t n_boxes, int64_t* deleted);
/* The map's points in id order: *n = count; xyz (cap x 3) and ids (cap) may be
 * NULL, else cap must be >= the count (LIVO_E_RANGE otherwise, *n still set). */
int livo_map_dump(livo_ctx* ctx, float* xyz, int32_t* ids, int64_t cap, int64_t* n);
/* Statistics of the last livo_map_add_points / ikd-Tree livo_map_incremental. */
int livo_map_last_add_stats(livo_ctx* ctx, livo_map_add_stats* out);

/* RGBpointBodyToWorld (src/laser_mapping.cpp:647-660) over laserCloudFullRes
 * (:258-265) at `state`: scan_id < 0 takes the last livo_scan_preprocess frame
 * at full resolution (feats_undistort, dense_map_en; resident until the next
 * frame), scan_id >= 0 a resident scan (feats_down_body, in the caller's point
 * order; intensity 0: a resident scan keeps x, y, z only).  out: n points
 * (world x, y, z; intensity copied; curvature 0), *n = their count; out may be
 * NULL to query the count, else cap >= *n (LIVO_E_RANGE otherwise). */
int livo_frame_to_world(livo_ctx* ctx, int32_t scan_id, const livo_state* state, livo_raw_point* out, int64_t cap,
                        int64_t* n);
/* LaserMapping::publish_frame_world_rgb (src/laser_mapping.cpp:1351-1381): the
 * cloud of livo_frame_to_world (same scan_id, same error codes, x, y, z bit for
 * bit) projected into the camera frame of `state` (Rcw = Rci Rwi^T, Pcw = -Rcw
 * Pwi + Pci, lidar_selection.cpp:900-901; of p only cam, R_ci and P_ci are
 * read), the points in front of the camera and inside the image kept in the
 * cloud's order, each with the bilinear sample of LidarSelector::getpixel
 * (src/lidar_selection.cpp:1004-1022).
 * bgr: 8-bit, interleaved B, G, R, row stride 3 * width; width / height must
 * equal p->cam.width / height (LIVO_E_INVALID).  bgr == NULL reuses the image
 * the previous successful call on this context uploaded (LIVO_E_INVALID if
 * there is none or its size differs).  getpixel indexes the image as a flat
 * byte array: u in (-1, 0) or [width - 1, width) reads the neighbouring row,
 * as the reference does; a tap outside the buffer (undefined there) reads 0
 * and the point counts in edge_reads.
 * *n = points kept (set on LIVO_OK and LIVO_E_RANGE).  out and src_index (the
 * kept point's position in the source cloud) may each be NULL; if one is not
 * and cap < *n: LIVO_E_RANGE, nothing written (cap >= n_in always suffices).
 * stats may be NULL. */
typedef struct livo_rgb_point {
    float x, y, z;
    uint8_t r, g, b, a; /* a = 255 */
} livo_rgb_point;
typedef struct livo_rgb_stats {
    int64_t n_in;         /* points of the source cloud                                   */
    int64_t n_out;        /* points kept (= *n)                                           */
    int64_t behind;       /* dropped: p_cam.z > 0 is false                                */
    int64_t out_of_frame; /* dropped: in front of the camera, isInFrame(.., 0) false      */
    int64_t edge_reads;   /* kept points with at least one tap outside the image buffer   */
} livo_rgb_stats;
int livo_cloud_colorize(livo_ctx* ctx, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                        const uint8_t* bgr, int32_t width, int32_t height, livo_rgb_point* out, int32_t* src_index,
                        int64_t cap, int64_t* n, livo_rgb_stats* stats);
/* LidarSelector::addSparseMap (src/lidar_selection.cpp:140-193, with getpatch
 * :117-138 and AddPoint's key :195-208): a frame's new visual map points.  The
 * cloud of livo_frame_to_world (same scan_id, x, y, z bit for bit; of p only
 * cam, R_ci, P_ci and patch_size are read) is projected into the gray image at
 * `state` with no p_cam.z test, as the reference has none; the points inside
 * the border (patch_size / 2 + 1) * 8 are scored with vikit's shiTomasiScore at
 * the truncated pixel, and of every cell of grid_size pixels (index =
 * (int)(u / grid_size) * (height / grid_size) + (int)(v / grid_size), which
 * aliases into the next column where height is no multiple of grid_size) the
 * point of the greatest positive score is selected, the lowest cloud index
 * among equals (`cur_value > map_value[index]`, in cloud order).  Selected
 * points come in ascending cell index, each with its level 0, 1, 2 patches in
 * Feature::patch layout, patch_size^2 * level + x * patch_size + y, as
 * livo_vio_update reads them (search level 0).  Feature::f is not produced.
 * gray: 8-bit, row stride width; width / height must equal p->cam.width /
 * height.  The image is kept in a buffer of this entry point's own
 * (livo_vio_update's and livo_cloud_colorize's are not touched); gray == NULL
 * reuses the image of the previous successful call (LIVO_E_INVALID if there
 * is none or its size differs).  LIVO_E_INVALID too for grid_size < 1,
 * patch_size outside 1..8, and a frame whose area inside the border is
 * narrower or lower than one cell.
 * *n = selected points (set on LIVO_OK and LIVO_E_CAPACITY).  out == NULL
 * with cap == 0 returns *n and the stats only; otherwise out (cap records) and
 * patches (cap x 3 x patch_size^2 floats) are both needed, and cap < *n
 * returns LIVO_E_CAPACITY with nothing written (n_cells always suffices).
 * stats may be NULL.  Two calls on the same input give the same bytes. */
typedef struct livo_vis_point {      /* 64 bytes */
    float   x, y, z;                 /* the cloud's world point (the bits of livo_frame_to_world)   */
    float   score;                   /* shiTomasiScore at (int)u, (int)v                             */
    double  u, v;                    /* new_frame_->w2c(pt)                                           */
    int32_t src_index;               /* index into the source cloud                                  */
    int32_t cell;                    /* grid index i of addSparseMap's second loop                    */
    int64_t voxel[3];                /* AddPoint's VOXEL_KEY                                          */
} livo_vis_point;
typedef struct livo_vis_stats {
    int64_t n_in;                    /* points of the source cloud                                    */
    int64_t in_frame;                /* passed isInFrame(pc.cast<int>(), (patch_size_half+1)*8)       */
    int64_t behind_in_frame;         /* of those: p_cam.z <= 0 or NaN (the reference has no z test here) */
    int64_t cell_overflow;           /* of those: index >= length (an out-of-bounds write in the reference) */
    int64_t n_out;                   /* selected points = cells of TYPE_POINTCLOUD                     */
    int64_t n_cells;                 /* length = (width/grid_size) * (height/grid_size)               */
} livo_vis_stats;
int livo_vio_select(livo_ctx* ctx, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                    int32_t grid_size, const uint8_t* gray, int32_t width, int32_t height,
                    livo_vis_point* out, float* patches, int64_t cap, int64_t* n, livo_vis_stats* stats);
/* ------------------------------------------------------------------------
 * The resident visual map (LidarSelector::feat_map, imgs_ and the features'
 * T_f_w_).  Points hold a position, a score, a voxel key and up to 20
 * observations (addObservation's cap, :945), kept in insertion order (index 0
 * the oldest held; the reference's obs_ is filled with push_front and runs the
 * other way); an observation holds its frame id, px, f = cam2world(px), level
 * and its patch pyramid (3 x patch_size^2 floats, Feature::patch layout); a
 * frame holds its gray image and pose.  livo_vmap_add stores what it is given
 * and never deletes; addObservation's policy (add_flag, the cap,
 * getFurthestViewObs / deleteFeatureRef, the new patch pyramid and score) is
 * livo_vio_observe below, which edits the map on the device.  An eviction can
 * leave a stored frame that no observation refers to; such a frame can never be
 * referred to again (observations are made from the current frame only), and
 * livo_vmap_release_frames gives its slot back to the frames stored later.
 * ------------------------------------------------------------------------ */
typedef struct livo_vmap_counts {
    int64_t n_points, n_obs, n_frames;
    int64_t max_points, max_frames;
    int32_t patch_size;
    int32_t width, height;           /* of the stored images (0 before the first frame)              */
    int32_t pad_;
} livo_vmap_counts;
typedef struct livo_vmap_point {     /* 64 bytes */
    double  pos[3];                  /* Point::pos_                                                   */
    float   value;                   /* Point::value (the shiTomasi score)                            */
    int32_t n_obs;                   /* observations, in list order from first_obs                    */
    int64_t voxel[3];                /* AddPoint's VOXEL_KEY                                          */
    int64_t first_obs;               /* index of its first observation in the dump                    */
} livo_vmap_point;
typedef struct livo_vmap_obs {       /* 48 bytes */
    int32_t frame_id, level;         /* Feature::id_, Feature::level                                  */
    double  px[2];                   /* Feature::px                                                   */
    double  f[3];                    /* Feature::f = cam2world(px)                                    */
} livo_vmap_obs;
/* (Re)creates an empty map of fixed capacities: max_points points of at most
 * 20 observations, max_frames frames, patches of patch_size (1..8) squared.
 * LIVO_E_INVALID for a capacity < 1. */
int livo_vmap_reset(livo_ctx* ctx, int64_t max_points, int64_t max_frames, int32_t patch_size);
/* Stores a past image and its pose (frame_cam of p at state: Rcw, Pcw; the
 * frame position -Rcw^T Pcw, in double) under frame_id (>= 0).  gray: 8-bit,
 * width x height = p->cam.width x height, row stride width, copied into a
 * buffer of the map's own; gray == NULL copies livo_vio_select's retained
 * image device to device.  Every frame of a map has the first one's size and
 * intrinsics source p->cam (undistorted: |d0| <= 1e-7).  LIVO_E_INVALID: no map,
 * a distorted camera, a size mismatch, no retained image, a duplicate id;
 * LIVO_E_CAPACITY: max_frames frames are live (livo_vmap_release_frames may
 * free some).  A released slot is taken before a fresh one. */
int livo_vmap_add_frame(livo_ctx* ctx, int32_t frame_id, const livo_state* state, const livo_vio_params* p,
                        const uint8_t* gray, int32_t width, int32_t height);
/* Adds n observations seen from stored frame frame_id.  point_ids == NULL
 * creates n points from livo_vis_point records (addSparseMap's tail): pos_ =
 * the record's float x, y, z widened, value = score, the voxel key = voxel,
 * one observation with px = (u, v) at level 0; their ids, consecutive from the
 * map's count, go to ids_out (n, may be NULL).  With point_ids, one
 * observation is appended to each listed point in order (addFrameRef): px from
 * the record's u, v, the level from levels (NULL: 0), the other fields
 * ignored.  patches: n x 3 x patch_size^2 floats as livo_vio_select writes
 * them.  f = ((u - cx) / fx, (v - cy) / fy, 1) normalised, in double, with the
 * frame's intrinsics.  LIVO_E_INVALID: an unknown frame or id, a level outside
 * 0..8; LIVO_E_CAPACITY: beyond max_points or 20 observations.  Nothing is
 * written on an error. */
int livo_vmap_add(livo_ctx* ctx, int32_t frame_id, int64_t n, const int32_t* point_ids, const livo_vis_point* pts,
                  const int32_t* levels, const float* patches, int32_t* ids_out);
/* n_frames counts the live frames: those stored and not released. */
int livo_vmap_info(livo_ctx* ctx, livo_vmap_counts* info);
/* Releases every stored frame that no observation refers to. released (cap ids, ascending
 * frame id; may be NULL with cap == 0 to count) and *n = frames released (set on LIVO_OK
 * and LIVO_E_CAPACITY; cap < *n releases nothing).  A released id may be stored again.
 * The counting form (released == NULL, cap == 0) returns LIVO_OK with *n = the frames a
 * releasing call would release now, and releases nothing; cap < *n with a buffer returns
 * LIVO_E_CAPACITY.  The references are counted on the device over every point's
 * observations; nothing that livo_vmap_dump shows changes.  LIVO_E_INVALID: no map. */
int livo_vmap_release_frames(livo_ctx* ctx, int32_t* released, int64_t cap, int64_t* n);
/* The map in id / list order: points (cap_points), obs (cap_obs) and patches
 * (cap_obs x 3 x patch_size^2) may all be NULL to query *n_points and *n_obs,
 * else the capacities must suffice (LIVO_E_RANGE otherwise, the counts set). */
int livo_vmap_dump(livo_ctx* ctx, livo_vmap_point* points, int64_t cap_points, livo_vmap_obs* obs, float* patches,
                   int64_t cap_obs, int64_t* n_points, int64_t* n_obs);

/* LidarSelector::addFromSparseMap (src/lidar_selection.cpp:332-593, with
 * getWarpMatrixAffine / getBestSearchLevel / warpAffine / NCC :224-318 and
 * Point::getCloseViewObs, src/point.cpp:142-170): the resident visual map
 * matched into the frame at `state`.  The cloud of livo_frame_to_world (same
 * scan_id, x, y, z bit for bit; it stands for pg_down: the 0.2 m VoxelGrid in
 * front is not run) gives the frame's 0.5 m voxel set and a depth image (on a
 * shared pixel the last cloud index wins, as the reference's sequential loop);
 * every map point whose stored key is in the set is projected, the nearest
 * point of each grid cell (cur_dist <= 10000; the greatest id among equals) is
 * tested for depth continuity, its observation of the closest view is chosen
 * (cosine >= 0.5), that observation's patch is warped from its own stored
 * image into the observation's stored level-0 patch (the reference aliases
 * patch_wrap = ref_ftr->patch: livo_vmap_dump shows it) with the affine
 * matrix and search level of the lowest cell that reached this step with the
 * same reference frame (Warp_map's key is the frame id), and compared with
 * the frame's level-0 patch: NCC (if ncc_en, rejected below ncc_thre) and the
 * squared error (rejected above outlier_threshold * patch_size^2).  The
 * survivors come in ascending cell index: out (records), pos (n x 3),
 * search_levels (n) and patches (n x 3 x patch_size^2) exactly as
 * livo_vio_update reads them.  DESIGN.md §8.9 has the arithmetic.
 * gray and its reuse as livo_vio_select, in a buffer of this entry point's
 * own.  LIVO_E_INVALID: no map (livo_vmap_reset), a distorted camera, a size
 * or patch size that differs from the map's, an odd patch_size, grid_size < 1
 * or a frame narrower than one cell inside the border.  An empty map gives
 * *n = 0.  *n = survivors (set on LIVO_OK and LIVO_E_CAPACITY).  out == NULL
 * with cap == 0 returns *n and the stats and leaves the map unchanged;
 * otherwise out, pos, search_levels and patches are all needed, and cap < *n
 * returns LIVO_E_CAPACITY with none of them written (the map's level-0
 * patches are rewarped as by a successful call).  stats may be NULL.  Two
 * calls on the same input give the same bytes. */
typedef struct livo_vmatch_point {   /* 48 bytes */
    int32_t point_id;                /* the map point                                                 */
    int32_t cell;                    /* grid index i (sub_sparse_map->index)                          */
    int32_t obs_index;               /* its chosen observation, in list order                         */
    int32_t frame_id;                /* ... and that observation's frame                              */
    int32_t search_level;
    float   error;                   /* sub_sparse_map->errors                                        */
    double  ncc;                     /* 0 when ncc_en is 0                                            */
    double  u, v;                    /* pc = new_frame_->w2c(pt->pos_)                                */
} livo_vmatch_point;
typedef struct livo_vmatch_stats {
    int64_t n_in;                    /* points of the source cloud                                    */
    int64_t n_voxels;                /* distinct 0.5 m voxels of the cloud (sub_feat_map.size())      */
    int64_t map_tested;              /* map points whose stored key is in the set                     */
    int64_t in_frame;                /* of those: in front of the camera and inside the border        */
    int64_t cell_overflow;           /* of those: index >= length (dropped)                           */
    int64_t cells_marked;            /* cells of TYPE_MAP                                             */
    int64_t depth_rejected, view_rejected, ncc_rejected, error_rejected;
    int64_t warp_shared;             /* cells that took another cell's warp (same reference frame)    */
    int64_t warp_nan;                /* cells whose inverse was NaN: the stored patch left as it was   */
    int64_t n_out;                   /* survivors = *n                                                */
} livo_vmatch_stats;
int livo_vio_match(livo_ctx* ctx, int32_t scan_id, const livo_state* state, const livo_vio_params* p,
                   int32_t grid_size, int32_t ncc_en, double ncc_thre, double outlier_threshold,
                   const uint8_t* gray, int32_t width, int32_t height, livo_vmatch_point* out, double* pos,
                   int32_t* search_levels, float* patches, int64_t cap, int64_t* n, livo_vmatch_stats* stats);
/* LidarSelector::addObservation (src/lidar_selection.cpp:905-962, with
 * Point::addFrameRef, deleteFeatureRef and getFurthestViewObs, src/point.cpp:
 * 61-65, 88-98, 211-239): the resident visual map brought up to date with the
 * frame just processed.  frame_id names a frame stored with livo_vmap_add_frame
 * at the state after livo_vio_update (new_frame_ after updateFrameState): its
 * stored Rcw / Pcw / position are new_frame_->T_f_w_ and pos(), its stored
 * image is img; the call takes no image and no state.  point_ids and
 * search_levels (n each; search_levels NULL: 0) are sub_sparse_map's
 * voxel_points and search_levels: the point_id and search_level columns of
 * livo_vio_match.  For every item, in this map's list order (index 0 = the
 * reference's obs_.back(), index n_obs - 1 its front):
 *   pt_cam = Rcw pos + Pcw; pt_cam.z <= 0 skips the item (a NaN passes);
 *   pc = world2cam(pt_cam); a pc outside the border (patch_size / 2 + 1) * 8
 *   skips it too (the reference has no such test: its getpatch and
 *   shiTomasiScore would read outside the image there).  A skipped item leaves
 *   its point untouched, also at 20 observations.
 *   add_flag: delta_p = |ref.Pcw + ref.Rcw cur.pos| > 0.5, ref the frame of
 *   observation 0, or |pc - px of observation 0| > 40.  (`delta_theta > 10`
 *   compares an acos with 10: it never holds and is not computed.)
 *   A point at 20 observations loses getFurthestViewObs(cur.pos)'s choice
 *   whether add_flag is set or not: the observation whose frame lies furthest
 *   from the current one, the newest among equals, the newest of all if no
 *   distance exceeds 0; the later ones move down by one.
 *   With add_flag the point's value becomes shiTomasiScore(img, (int)pc.x,
 *   (int)pc.y) and an observation of frame_id is appended: px = pc, f =
 *   cam2world(pc), the item's level, getpatch at levels 0, 1, 2.
 * out (n records in input order) and stats may be NULL.  Everything is
 * validated before anything is written: LIVO_E_INVALID for no map, an unknown
 * frame, n < 0, an id outside the map, a level outside 0..8 and a point id
 * listed twice (the reference has one point per grid cell).  n == 0 is
 * LIVO_OK.  DESIGN.md §8.10 has the arithmetic.  Two calls on the same input
 * give the same bytes. */
#define LIVO_VOBS_BEHIND       1     /* skipped: pt_cam.z <= 0                                        */
#define LIVO_VOBS_OUT_OF_FRAME 2     /* skipped: pc outside the border                                */
#define LIVO_VOBS_POSE         4     /* delta_p > 0.5                                                 */
#define LIVO_VOBS_PIXEL        8     /* pixel_dist > 40                                               */
#define LIVO_VOBS_DELETED      16    /* an observation was evicted                                    */
#define LIVO_VOBS_ADDED        32    /* an observation was appended                                   */
typedef struct livo_vobs_point {     /* 56 bytes */
    int32_t point_id;
    int32_t flags;                   /* LIVO_VOBS_* bits                                              */
    int32_t n_obs;                   /* the point's observations after the call                       */
    int32_t deleted_index;           /* the evicted observation's index before the call, -1: none     */
    int32_t deleted_frame_id;        /* ... and its frame, -1: none                                   */
    float   score;                   /* the new Point::value, 0 if nothing was added                  */
    double  u, v;                    /* pc; 0 for a skipped item, as delta_p and pixel_dist           */
    double  delta_p, pixel_dist;
} livo_vobs_point;
typedef struct livo_vobs_stats {
    int64_t n_in;
    int64_t behind, out_of_frame;    /* skipped items                                                 */
    int64_t pose_flagged, pixel_flagged;
    int64_t added, deleted;
    int64_t deleted_without_add;     /* points at 20 observations that lost one and gained none       */
    int64_t n_obs_total;             /* the map's observations after the call                         */
} livo_vobs_stats;
int livo_vio_observe(livo_ctx* ctx, int32_t frame_id, int64_t n, const int32_t* point_ids,
                     const int32_t* search_levels, livo_vobs_point* out, livo_vobs_stats* stats);
/* LidarSelector::detect(img, pg) (src/lidar_selection.cpp:1024-1073) behind its image
 * conversion: one camera frame through every stage above, resident from stage to stage.
 * The call equals this chain of calls, byte for byte in *state, stats, livo_vmap_dump and
 * livo_vmap_info:
 *   1. livo_vio_match(scan_id, *state, gray) with d's grid_size, ncc_en, ncc_thre and
 *      outlier_threshold                         -> the survivors S
 *   2. livo_vio_select(scan_id, *state, gray) with d->grid_size -> the new points N
 *   3. livo_vio_update(gray, S.pos, S.search_levels, S.patches, state, prior); without
 *      survivors *state is left as it is (ComputeJ returns at total_points == 0)
 *   4. livo_vmap_add_frame(frame_id, *state after 3, gray)
 *   5. livo_vio_observe(frame_id, S.point_id, S.search_level)
 *   6. livo_vmap_add(frame_id, N, point_ids = NULL)
 * The reference inserts addSparseMap's points before ComputeJ, their Feature holding
 * T_f_w_ at the state before the update; this map holds one pose per frame, the updated
 * one, and creates the points behind the observe, so that their ids cannot be among the
 * observed ones.
 * gray is required (a frame is a new image): it is uploaded once, serves 1 to 3 and
 * becomes the stored frame's image by a device copy.  No stage's result array is copied to
 * the host: behind 2 the counters are read (the survivor and selected counts size the
 * later launches), at the end the updated state, the observe's records and counters and
 * the stored frame.  livo_vio_select's and livo_vio_match's retained images are untouched.
 * Refused before any launch, with nothing changed: LIVO_E_INVALID for no map, gray == NULL,
 * frame_id < 0 or stored already, and whatever the six calls refuse in p, d, width and
 * height; LIVO_E_NOSCAN; LIVO_E_CAPACITY for a full frame store.  LIVO_E_CAPACITY too when
 * the map's points and N together exceed max_points, known behind 2: then *state is
 * untouched, no frame is stored, no observation and no point is added, stats holds match,
 * select, n_matched, n_new and first_new_id, and the map's level-0 patches are left
 * rewarped, exactly as livo_vio_match's own capacity error leaves them.  stats may be
 * NULL.  Two calls on the same input give the same bytes. */
typedef struct livo_vdetect_params {
    int32_t grid_size;          /* match and select */
    int32_t ncc_en;
    double  ncc_thre;
    double  outlier_threshold;
} livo_vdetect_params;
typedef struct livo_vdetect_stats {
    livo_vmatch_stats match;
    livo_vis_stats    select;
    livo_vio_stats    update;
    livo_vobs_stats   observe;
    int64_t n_matched;          /* survivors handed to the update and the observe */
    int64_t n_new;              /* points created                                  */
    int32_t first_new_id;       /* -1 if n_new == 0                                */
    int32_t pad_;
} livo_vdetect_stats;
int livo_vio_detect(livo_ctx* ctx, int32_t scan_id, int32_t frame_id, livo_state* state, const livo_state* prior,
                    const livo_vio_params* p, const livo_vdetect_params* d, const uint8_t* gray, int32_t width,
                    int32_t height, livo_vdetect_stats* stats);
/* pcl_wait_pub and pg_down: what a LiDAR frame hands to the camera frames that follow it.
 * Ids in the scan_id argument of the frame stages; no scan upload ever returns them (scan
 * ids are small slot indices). */
#define LIVO_CLOUD_WORLD      0x40000000  /* *pcl_wait_pub = *laserCloudWorld, laser_mapping.cpp:258-268 */
#define LIVO_CLOUD_WORLD_DOWN 0x40000001  /* pg_down, lidar_selection.cpp:341-344 */
typedef struct livo_cloud_info {
    int64_t n;            /* points of the world cloud */
    int64_t n_down;       /* points of pg_down; -1: not built (match_leaf <= 0) */
    int32_t down_filtered;/* 0: PCL returned its input (dx*dy*dz > INT32_MAX) or not built */
    int32_t pad_;
    int64_t device_bytes;
} livo_cloud_info;
/* Stores the cloud of livo_frame_to_world(src_scan_id, lio_state) on the device: n x 5 floats
 * in the caller's point order, bit for bit what that call returns (src_scan_id < 0: the last
 * preprocessed frame at full resolution, else a resident scan).  The buffer belongs to the
 * context and replaces the previous published cloud; it outlives the next
 * livo_scan_preprocess, the release of the source scan and any map change, and is freed with
 * the context.  match_leaf > 0 also builds pg_down: the PCL VoxelGrid of
 * livo_scan_preprocess over the stored float world points at that leaf (centroids of all
 * five columns, ascending leaf order; a leaf too small for 32-bit indices keeps the input,
 * as PCL does).  The reference filters inside every detect; the filter is a function of the
 * cloud alone, so one filter per LiDAR frame gives the same points.
 * livo_frame_to_world, livo_cloud_colorize, livo_vio_select, livo_vio_match and
 * livo_vio_detect take LIVO_CLOUD_WORLD and LIVO_CLOUD_WORLD_DOWN as scan_id: `state` then
 * places the camera only and the points are read as stored (livo_frame_to_world ignores
 * `state` but still requires it).  livo_vio_detect(LIVO_CLOUD_WORLD) runs its match on
 * pg_down where it exists and its select on the full cloud, as the reference does: its
 * chain is match(LIVO_CLOUD_WORLD_DOWN), select(LIVO_CLOUD_WORLD), then 3 to 6.  Both ids
 * are LIVO_E_NOSCAN before the first publish, LIVO_CLOUD_WORLD_DOWN also after a publish
 * with match_leaf <= 0, and both in every other entry point.
 * LIVO_E_INVALID: ctx or lio_state NULL, a non-finite match_leaf, a cloud id as
 * src_scan_id; LIVO_E_NOSCAN: an unknown scan; LIVO_E_RANGE: n > 2^31 - 1 - 256.  A refused
 * call leaves the previous cloud as it was.  info may be NULL. */
int livo_cloud_publish(livo_ctx* ctx, int32_t src_scan_id, const livo_state* lio_state, float match_leaf,
                       livo_cloud_info* info);
/* The published cloud's sizes; LIVO_E_NOSCAN before the first publish. */
int livo_cloud_info_get(livo_ctx* ctx, livo_cloud_info* out);

/* ------------------------------------------------------------------------
 * IMU forward propagation: ImuProcess::IMU_init / detectZeroVelocity
 * (src/IMU_Processing.cpp:92-197) and the first half of UndistortPcl
 * (:236-338), the step that produces the state every other entry point takes
 * ("after propagation"), its 18 x 18 covariance and the Pose6D table.
 * ------------------------------------------------------------------------ */
typedef struct livo_imu_sample { double stamp; double acc[3]; double gyr[3]; } livo_imu_sample;   /* sensor_msgs::Imu, seconds */

typedef struct livo_imu_params {       /* ImuProcess members the propagation reads */
    double cov_acc[3], cov_gyr[3], cov_bias_gyr[3], cov_bias_acc[3];
    double mean_acc[3];                 /* only G_m_s2 / |mean_acc| is used */
} livo_imu_params;

typedef struct livo_imu_carry {        /* what UndistortPcl keeps between calls */
    livo_imu_sample last_imu;           /* last_imu_      */
    double acc_s_last[3], angvel_last[3];
    double last_lidar_end_time;         /* last_lidar_end_time_ */
} livo_imu_carry;

typedef struct livo_imu_job {
    const livo_imu_sample* imu; int32_t n_imu;   /* meas.imu, without last_imu_ (the call pushes it in front) */
    double pcl_beg_time, pcl_end_time;           /* as computed at :211 and :219-221 */
} livo_imu_job;

enum {
    LIVO_IMU_INIT_COLLECTING = 0, /* init_iter_num < 50 (:159-163)                              */
    LIVO_IMU_INIT_RESET = 1,      /* not at rest: Reset() (:38-51, :153-157)                     */
    LIVO_IMU_INIT_DONE = 2        /* gravity, bias_g and the params' _inited values set (:184-196) */
};

/* The constructor's values (:18-34) and the values IMU_init leaves behind (:190-194: 0.01, 0.01,
 * 1e-4, 1e-4; mean_acc is kept).  Host code. */
int livo_imu_params_default(livo_imu_params* p);
int livo_imu_params_inited(livo_imu_params* p);
/* IMU_init with detectZeroVelocity over meas.imu (n samples): the running means and covariances
 * in params->mean_acc / cov_acc / cov_gyr and mean_gyr, counted by *init_iter_num (1 at the
 * start, as the constructor sets it).  *status: LIVO_IMU_INIT_*.  On RESET mean_acc, mean_gyr
 * and *init_iter_num take Reset()'s values (the caller clears its carry, as Reset() does); on
 * DONE state->gravity = -mean_acc / |mean_acc| * 9.81, state->bias_g = mean_gyr and the
 * covariances take livo_imu_params_inited's values.  In every case the caller's carry takes
 * last_imu = imu[n - 1] (:149) unless it was reset.  n == 0 changes nothing (Process2 :390).
 * Plain host code, no device needed: ctx is not used and may be NULL. */
int livo_imu_init(livo_ctx* ctx, const livo_imu_sample* imu, int32_t n, livo_imu_params* params,
                  int32_t* init_iter_num, double mean_gyr[3], livo_state* state, int32_t* status);
/* n independent forward propagations (:236-338) in one launch, one wave per job.  Job j reads
 * jobs[j], carries[j], states[j]; it writes the propagated state (rot, pos, vel at
 * pcl_end_time, the covariance F_x P F_x^T + cov_w per sample), the updated carry, and, with
 * poses != NULL, its Pose6D table at poses + j * pose_cap: row 0 from the carry and the
 * incoming state (:238), then one row per propagated sample; n_poses[j] = its rows (n_poses may
 * be NULL).  Samples whose stamp lies before carry.last_lidar_end_time are skipped (:251).
 * LIVO_E_RANGE, before anything runs, if poses != NULL and a job's table exceeds pose_cap
 * (n_imu + 1 rows always suffice).  Touches neither the map nor the scans: allowed while
 * batches are in flight. */
int livo_imu_propagate_batch(livo_ctx* ctx, int32_t n, const livo_imu_job* jobs, const livo_imu_params* params,
                             livo_imu_carry* carries, livo_state* states, livo_imu_pose* poses, int32_t pose_cap,
                             int32_t* n_poses);
/* The batch with n = 1; it also leaves the table and the frame-end pose resident in the
 * context for livo_scan_preprocess_imu (replacing those of the previous call; a camera frame
 * propagates with no points behind it).  poses and n_poses may be NULL. */
int livo_imu_propagate(livo_ctx* ctx, const livo_imu_job* job, const livo_imu_params* params, livo_imu_carry* carry,
                       livo_state* state, livo_imu_pose* poses, int32_t pose_cap, int32_t* n_poses);
/* livo_scan_preprocess with the table and the end pose of the last livo_imu_propagate, read
 * where they lie on the device.  LIVO_E_INVALID if no table is resident. */
int livo_scan_preprocess_imu(livo_ctx* ctx, const livo_raw_point* raw, int64_t n, float leaf_size, int32_t* scan_id,
                             livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap, int64_t* n_down);

/* ------------------------------------------------------------------------
 * Sensor handlers: the driver's message to the time-ordered frame on the device.
 *   Preprocess::process, feature_enabled == false     src/preprocess.cpp:82-116
 *     avia_handler :315-349, oust64_handler :424-453, velodyne_handler with point
 *     times :578-637, xt32_handler :650-680
 *   sort(meas.lidar->points, time_list)                src/laser_mapping.cpp:705
 *   UndistortPcl's slice from lidar_scan_index_now     src/IMU_Processing.cpp:217-235
 * Not built: feature extraction (give_feature), extract_normal (#define NORMAL) and the
 * Velodyne branch that derives point times from yaw (given_offset_time == false).
 * ------------------------------------------------------------------------ */
typedef struct livo_livox_point {      /* livox_ros_driver::CustomPoint as it lies in memory, 20 B */
    uint32_t offset_time;               /* ns from the message's timebase */
    float x, y, z;
    uint8_t reflectivity, tag, line, pad;
} livo_livox_point;

typedef struct livo_cloud_layout {     /* sensor_msgs::PointCloud2: point_step and the byte offsets its `fields` give */
    int32_t point_step, off_x, off_y, off_z, off_intensity, off_time;
} livo_cloud_layout;                   /* x, y, z, intensity: float32.  time: uint32 ns (OUST64 `t`),
                                          float32 s (VELO16 `time`), float64 s (XT32 `timestamp`) */

enum { LIVO_LIDAR_AVIA = 1, LIVO_LIDAR_VELO16 = 2, LIVO_LIDAR_OUST64 = 3, LIVO_LIDAR_XT32 = 4 };  /* preprocess.h:14 */

typedef struct livo_ingest_params {    /* Preprocess members, laser_mapping.cpp:989-993 */
    int32_t lidar_type;                /* LIVO_LIDAR_* */
    int32_t n_scans, point_filter_num, reserved;
    double  blind;
} livo_ingest_params;

typedef struct livo_ingest_info {
    int64_t n_in, n_kept, cursor;      /* cursor = lidar_scan_index_now */
    int64_t n_rejected, n_decimated;   /* failed the handler's predicate (AVIA: point 0 too, which its loop never
                                          visits) / passed it but not the 1-in-point_filter_num */
    float   end_curvature;             /* points.back().curvature after the sort (ms); 0 when n_kept == 0 */
} livo_ingest_info;

/* AVIA, 16, 2, 0.01: the nh.param defaults. */
int livo_ingest_params_default(livo_ingest_params* p);
/* The message's n points are uploaded as they are, in one copy (page-locked memory, livo_host_register,
 * is read by the copy engine directly; the buffer is free again on return), the handler of
 * p->lidar_type and the time sort run on the device, and the result, 5 floats a point, stays in the
 * context as the current frame (meas.lidar) with cursor = 0, replacing the previous one.  The handlers
 * are the reference's as written: AVIA never emits point 0, compares x*x + y*y with `blind`
 * unsquared and counts its 1-in-point_filter_num over the survivors; OUST64 keeps r^2 == blind^2 and
 * VELO16 drops it; XT32 compares r^2 with `blind` unsquared.  The sort is stable on the float's
 * order-preserving 32-bit key: ties keep message order (one of the outcomes std::sort may produce),
 * -0.0 lies before +0.0, NaNs with the sign bit set lie first and the others last (the reference's
 * order of NaN times is undefined, and livo_frame_take's count assumes there are none).
 * livo_frame_ingest_livox takes LIVO_LIDAR_AVIA only, livo_frame_ingest_cloud the other three, with
 * every offset of `layout` (all five are checked, each field whole inside point_step <= 240).
 * LIVO_E_INVALID: a NULL argument, point_filter_num < 1, n_scans < 0, n < 0, a lidar_type that is
 * unknown or does not match the call, a layout that does not fit, and a VELO16 message with n > 0
 * whose last point has time <= 0: the reference then derives the times from yaw, ring by ring
 * (given_offset_time == false), which is not built here.  LIVO_E_RANGE: n > 2^31 - 1 - 256.
 * LIVO_E_HIP: no device.  LIVO_E_BUSY while a batch is in flight.  info may be NULL. */
int livo_frame_ingest_livox(livo_ctx* ctx, const livo_ingest_params* p, const livo_livox_point* pts, int64_t n,
                            livo_ingest_info* info);
int livo_frame_ingest_cloud(livo_ctx* ctx, const livo_ingest_params* p, const void* data, int64_t n,
                            const livo_cloud_layout* layout, livo_ingest_info* info);
/* The current frame's counts and cursor; LIVO_E_INVALID before any ingest. */
int livo_frame_info(livo_ctx* ctx, livo_ingest_info* info);
/* The resident, sorted frame (= meas.lidar): *n = its points; out == NULL queries, else cap >= *n
 * (LIVO_E_RANGE otherwise).  LIVO_E_INVALID before any ingest. */
int livo_frame_dump(livo_ctx* ctx, livo_raw_point* out, int64_t cap, int64_t* n);
/* UndistortPcl's slice and livo_scan_preprocess_imu's body: starting at the cursor, the points with
 * (double)curvature <= offset_limit_ms are taken (*n_taken; the cursor advances by it, and returns
 * to 0 afterwards with is_lidar_end), de-skewed where they lie against the table and end pose of the
 * last livo_imu_propagate, filtered at leaf_size and made a resident scan (*scan_id; undistorted,
 * down, down_cap, n_down as livo_scan_preprocess_imu's).  The caller computes the limit as the
 * reference does: (pcl_end_time - lidar_beg_time) * 1000.0 on a LiDAR frame, with pcl_end_time =
 * lidar_beg_time + end_curvature / 1000.0, and 0.0 on a camera frame (:219-224).  scan_id == NULL
 * moves the cursor only (a camera frame, whose feats_undistort Run() never reads).  *n_taken == 0
 * makes no scan: *scan_id = -1, and the frame of livo_frame_to_world(-1) is empty.  Otherwise
 * livo_frame_to_world(-1) and livo_cloud_publish(-1) see the taken range.  LIVO_E_INVALID: ctx or
 * n_taken NULL, a non-finite leaf_size, no ingest yet, a scan_id before any livo_imu_propagate.
 * LIVO_E_BUSY while a batch is in flight.  A refused or failed take leaves the cursor where it was. */
int livo_frame_take(livo_ctx* ctx, double offset_limit_ms, int is_lidar_end, float leaf_size, int32_t* scan_id,
                    livo_raw_point* undistorted, livo_raw_point* down, int64_t down_cap, int64_t* n_down,
                    int64_t* n_taken);

/* ---- One LiDAR frame in one call: the LIO half of LaserMapping::Run() (laser_mapping.cpp:37-284) ---- */
typedef struct livo_lio_params {
    float   filter_size_surf;     /* livo_frame_take's leaf_size */
    float   match_leaf;           /* livo_cloud_publish's; <= 0: no pg_down */
    double  filter_size_map_min;  /* livo_map_incremental's fs */
    int32_t ekf_inited;           /* flg_EKF_inited (laser_mapping.cpp:79): 0 skips the IEKF loop */
    int32_t first_scan;           /* ikdtree.Root_Node == nullptr / flg_first_scan (:133-152) */
    int32_t dense_map_en;         /* publish the full-resolution frame (-1) or the new scan */
    int32_t prev_scan_id;         /* the facade's current scan, -1: none */
} livo_lio_params;

enum { LIVO_LIO_EMPTY = 0, LIVO_LIO_FIRST_SCAN = 1, LIVO_LIO_UPDATED = 2 };

typedef struct livo_lio_stats {
    int32_t stage;                /* LIVO_LIO_* */
    int32_t scan_id;              /* the new resident scan, -1 if none */
    int64_t n_taken, n_down;
    int32_t map_built;            /* FIRST_SCAN: 1 if n_down > 5 and the map was built / filled */
    int32_t pad_;
    livo_iter_stats iter;         /* zeroed when the loop did not run */
    int64_t map_counts[2];        /* livo_map_incremental's */
    livo_cloud_info cloud;        /* livo_cloud_publish's (zeroed unless stage == LIVO_LIO_UPDATED) */
} livo_lio_stats;

/* Everything between "the driver's message is resident" (livo_frame_ingest_*) and "the map and
 * pcl_wait_pub are updated", with the state on the device from the propagation to the publish.  The
 * call equals this chain, byte for byte, in *state, *state_propagat, *carry, *stats, livo_map_dump /
 * livo_ivox_dump, livo_frame_to_world(LIVO_CLOUD_WORLD / LIVO_CLOUD_WORLD_DOWN), livo_cloud_info_get
 * and the resident Pose6D table:
 *   1. livo_imu_propagate(job, imu, carry, state), then *state_propagat = *state (:58-59);
 *   2. livo_frame_take(offset_limit_ms, is_lidar_end = 1, filter_size_surf, &scan_id); n_taken == 0:
 *      LIVO_LIO_EMPTY, nothing further runs and prev_scan_id stays resident;
 *   3. first_scan (:133-152): with n_down > 5, livo_map_build (ikd-Tree backend) or
 *      livo_ivox_add_points (iVox) of the down-sampled points; LIVO_LIO_FIRST_SCAN either way, no loop,
 *      no map_incremental, no publish, prev_scan_id untouched;
 *   4. prev_scan_id >= 0: livo_scan_inherit_neighbors(scan_id, prev_scan_id) on the iVox backend, then
 *      livo_scan_release(prev_scan_id);
 *   5. ekf_inited: livo_iekf_update(scan_id, state, state_propagat, &iter);
 *   6. livo_map_incremental(scan_id, state, filter_size_map_min, ekf_inited, NULL, map_counts);
 *   7. livo_cloud_publish(dense_map_en ? -1 : scan_id, state, match_leaf, &cloud): LIVO_LIO_UPDATED.
 * The propagated state is not copied to the host between the stages: the de-skew reads its end pose,
 * the IEKF slot (state, prior, the covariance factors) is staged from it by a kernel, and stages 6 and 7
 * read the pose from the loop's slot (ekf_inited == 0: from the propagated state).  The host receives
 * the state once, at the end, with the carry, iter and the counts that size launches.
 * The refusals listed here happen before any launch and change nothing (the cursor, *carry, *state,
 * the map and the published cloud stay); an error a stage reports later (LIVO_E_OOM, LIVO_E_HIP,
 * LIVO_E_RANGE) leaves what the stages before it did.  LIVO_E_INVALID: a NULL argument (stats may be NULL), no ingest yet, what the
 * seven calls refuse in their own arguments (n_imu < 0, samples missing, a non-finite
 * filter_size_surf or match_leaf, filter_size_map_min not > 0); LIVO_E_NOMAP: first_scan == 0 on a
 * backend that holds no map (iVox: not initialised, whatever first_scan is); LIVO_E_NOSCAN: an
 * unknown prev_scan_id; LIVO_E_BUSY: a submitted batch is in flight; LIVO_E_HIP: no device.  Two
 * calls on the same input give the same bytes. */
int livo_lio_frame(livo_ctx* ctx, const livo_imu_job* job, const livo_imu_params* imu, livo_imu_carry* carry,
                   double offset_limit_ms, const livo_lio_params* p, livo_state* state, livo_state* state_propagat,
                   livo_lio_stats* stats);

/* ------------------------------------------------------------------------
 * Loop search: the resident Stable Triangle Descriptor database (include/STD/STDesc.cpp)
 *   STDescManager::AddSTDescs            :355-374
 *   STDescManager::SearchLoop            :299-353
 *     candidate_selector :960-1099, candidate_verify :1102-1192, triangle_solver :1194-1219,
 *     plane_geometric_verify :1221-1280
 * GenerateSTDescs' products, the key frame's descriptors and plane cloud, are what livo_std_stage
 * takes; livo_std_generate (below) makes them on the device from the resident key cloud.
 * ------------------------------------------------------------------------ */
#define LIVO_STD_MAX_FRAMES 20000    /* MAX_FRAME_N (STDesc.h): the reference's vote array */
#define LIVO_STD_MAX_CANDIDATES 64   /* candidate_num beyond it is refused (the reference's default: 50) */

typedef struct livo_std_params {     /* read_parameters' defaults (:83-93), not STDesc.h's initialisers */
    int32_t skip_near_num;           /* 50 */
    int32_t candidate_num;           /* 50 */
    double  rough_dis_threshold;     /* 0.01 */
    double  vertex_diff_threshold;   /* 0.5 */
    double  icp_threshold;           /* 0.5 */
    double  normal_threshold;        /* 0.2 */
    double  dis_threshold;           /* 0.5 */
} livo_std_params;

typedef struct livo_std_desc {       /* STDesc (STDesc.h), 152 B */
    double   side_length[3], vertex_A[3], vertex_B[3], vertex_C[3], center[3], vertex_attached[3];
    uint32_t frame_id;
    uint32_t pad;
} livo_std_desc;

typedef struct livo_std_plane {      /* a plane cloud's point: x, y, z and normal_x, _y, _z */
    float xyz[3], normal[3];
} livo_std_plane;

typedef struct livo_std_pair {
    int32_t src;        /* index into the staged descriptors */
    int32_t frame;      /* the stored descriptor's frame */
    int32_t db_index;   /* ... and its insertion index in the database (livo_std_dump's order) */
} livo_std_pair;

typedef struct livo_std_result {     /* loop_result, loop_transform and loop_std_pair's size */
    int32_t frame;                   /* -1: no loop */
    int32_t n_candidates;
    int32_t n_pairs;
    int32_t candidate;               /* the winner's index in livo_std_candidates, -1 with no loop */
    double  score;                   /* 0 with no loop */
    double  rot[9];                  /* row-major; identity with no loop (laser_mapping.cpp:1255-1256) */
    double  t[3];
} livo_std_result;

typedef struct livo_std_candidate {  /* one STDMatchList and what candidate_verify made of it */
    int32_t frame, votes;            /* votes = the match list's length */
    int32_t use_size, max_vote, max_vote_index, pad;
    double  score;                   /* -1 with max_vote < 4; NaN with an empty source plane cloud */
    double  rot[9], t[3];            /* identity / zero with max_vote < 4 */
} livo_std_candidate;

typedef struct livo_std_info {
    int64_t frames, descs, planes, cells;
    int64_t max_descs, max_frames, max_planes;
    int64_t staged_descs, staged_planes;  /* -1: nothing staged */
} livo_std_info;

int livo_std_params_default(livo_std_params* p);
/* An empty database for up to max_descs descriptors, max_frames key frames and max_planes plane
 * points, with the search's parameters.  LIVO_E_INVALID: a NULL argument, a non-finite or negative
 * threshold, skip_near_num < 0, candidate_num outside [0, LIVO_STD_MAX_CANDIDATES], a capacity < 1
 * (all found before the context is read); LIVO_E_RANGE: max_frames > LIVO_STD_MAX_FRAMES, max_descs
 * or max_planes > 2^31 - 1 - 1024. */
int livo_std_reset(livo_ctx* ctx, const livo_std_params* params, int64_t max_descs, int64_t max_frames,
                   int64_t max_planes);
/* The current key frame, GenerateSTDescs' products, uploaded once; it stays resident until the next
 * stage or reset (a commit keeps it staged).  LIVO_E_INVALID: NULL with a count > 0, a negative count,
 * a non-finite descriptor or plane, no reset; LIVO_E_RANGE: a |side_length| >= 2^20 - 2. */
int livo_std_stage(livo_ctx* ctx, const livo_std_desc* descs, int64_t n, const livo_std_plane* planes, int64_t m);
/* SearchLoop of the staged frame against the committed ones.  pairs (may be NULL) receives the
 * winner's success list in match-list order, up to cap entries; *n_pairs (may be NULL) its length.
 * LIVO_E_INVALID: ctx or out NULL, cap < 0, no reset, nothing staged. */
int livo_std_search(livo_ctx* ctx, livo_std_result* out, livo_std_pair* pairs, int64_t cap, int64_t* n_pairs);
/* AddSTDescs of the staged frame, and its plane cloud as plane_cloud_vec_[*frame].  LIVO_E_INVALID:
 * no reset, nothing staged, a staged frame_id that is not the new frame's index; LIVO_E_CAPACITY: the
 * frame does not fit (nothing is added).  frame may be NULL. */
int livo_std_commit(livo_ctx* ctx, int32_t* frame);
/* The last search's candidates in candidate order, and one candidate's match list. */
int livo_std_candidates(livo_ctx* ctx, livo_std_candidate* out, int64_t cap, int64_t* n);
int livo_std_matches(livo_ctx* ctx, int32_t candidate, livo_std_pair* pairs, int64_t cap, int64_t* n);
int livo_std_info_get(livo_ctx* ctx, livo_std_info* info);
/* The stored descriptors in insertion order (descs NULL: the count only) and the plane cloud of
 * `frame` (frame < 0 or planes NULL with n_planes NULL: skipped).  LIVO_E_RANGE: a cap too small. */
int livo_std_dump(livo_ctx* ctx, livo_std_desc* descs, int64_t desc_cap, int64_t* n_descs, int32_t frame,
                  livo_std_plane* planes, int64_t plane_cap, int64_t* n_planes);

/* ------------------------------------------------------------------------
 * A key frame's descriptors on the device: STDescManager::GenerateSTDescs (STDesc.cpp:264-297)
 *   init_voxel_map :376-422, init_plane :1367-1409, getPlane :492-507, build_connection :424-490,
 *   corner_extractor :509-617, extract_corner :619-781, non_maxi_suppression :783-822,
 *   build_stdesc :824-958
 * over the key cloud, the frames of the world cloud a key frame is made of
 * (laser_mapping.cpp:1239-1248).  Where the reference's result is implementation-defined the port
 * pins it: voxels are visited in order of first appearance in the key cloud; a
 * plane's normal has its component of largest magnitude positive (the first of equal ones); the
 * maximum_corner_num cut orders by attached count descending, then by index in the suppressed
 * list; build_stdesc visits only the neighbours that exist, ordered by (distance, index).
 * ------------------------------------------------------------------------ */
#define LIVO_STD_GEN_MAX_IMAGE 80    /* the side of extract_corner's projection image the kernel holds */
#define LIVO_STD_GEN_MAX_NEAR 64     /* descriptor_near_num beyond it is refused */

typedef struct livo_std_gen_params { /* read_parameters' defaults (:57-81) */
    double  voxel_size;                  /* 2.0 */
    double  plane_detection_thre;        /* 0.01 */
    double  plane_merge_normal_thre;     /* 0.1 */
    double  proj_image_resolution;       /* 0.5 */
    double  proj_dis_min;                /* 0 */
    double  proj_dis_max;                /* 2 */
    double  corner_thre;                 /* 10 */
    double  non_max_suppression_radius;  /* 2.0 */
    double  descriptor_min_len;          /* 2 */
    double  descriptor_max_len;          /* 50 */
    double  std_side_resolution;         /* 0.2 */
    int32_t voxel_init_num;              /* 10 */
    int32_t maximum_corner_num;          /* 100 */
    int32_t descriptor_near_num;         /* 10 */
    int32_t pad;
} livo_std_gen_params;

typedef struct livo_std_gen_stats {
    int64_t points, voxels, plane_voxels, jobs;
    int64_t corners_raw, corners_suppressed, corners;  /* before suppression, after it, after the cut */
    int64_t triangles_tried;                           /* the (i, m, n) visited */
    int64_t descs;
} livo_std_gen_stats;

typedef struct livo_std_corner {     /* the PointXYZINormal fields build_stdesc reads */
    float xyz[3];
    float attached;                  /* intensity: the points of the corner's cell */
    float normal[3];
    float pad;
} livo_std_corner;

int livo_std_gen_params_default(livo_std_gen_params* p);
/* The key cloud: resident, grow-only, x y z floats in world coordinates.  livo_std_key_add appends
 * a resident cloud device to device; it takes the ids livo_frame_to_world takes (LIVO_CLOUD_WORLD
 * is the reference's case: the caller vouches that another id's cloud is in world coordinates) and
 * answers LIVO_E_NOSCAN as that call does.  A resident scan is appended in the order it is stored in,
 * which is not the order it was uploaded in (the published clouds are stored as published); the
 * voxel visiting order follows the key cloud's order.  livo_std_key_add_host appends n host points, the next
 * stride_bytes (>= 12) behind the last; LIVO_E_INVALID for a non-finite one.  LIVO_E_RANGE: more
 * than 2^31 - 1 - 1024 points. */
int livo_std_key_add(livo_ctx* ctx, int32_t scan_id);
int livo_std_key_add_host(livo_ctx* ctx, const float* xyz, int64_t n, int64_t stride_bytes);
int livo_std_key_clear(livo_ctx* ctx);
int livo_std_key_count(livo_ctx* ctx, int64_t* n);
/* GenerateSTDescs of the key cloud.  Its products become the staged frame, the state
 * livo_std_stage leaves, with frame_id = the number of committed frames; the key cloud is cleared
 * (laser_mapping.cpp:1249).  An empty cloud, or one without planes, stages zero descriptors.  Two
 * calls on the same input give the same bytes.  stats may be NULL.
 * Found before the context is read: LIVO_E_INVALID: a NULL argument, a non-finite or negative
 * threshold, voxel_size, proj_image_resolution or std_side_resolution not > 0, voxel_init_num < 0,
 * maximum_corner_num < 1, descriptor_near_num outside [3, LIVO_STD_GEN_MAX_NEAR]; LIVO_E_RANGE:
 * voxel_size * sqrt(17) >= 10 (extract_corner's box starts at +-10 and a point of the 27 voxels
 * round V lies up to sqrt(17) edges from the connected plane's centre), an image side
 * (int)(2 * voxel_size * sqrt(17) / proj_image_resolution + 5) > LIVO_STD_GEN_MAX_IMAGE,
 * descriptor_max_len * 1000 >= 2^21 - 1 or descriptor_max_len / std_side_resolution >= 2^20 - 2
 * (the packed keys).  Then LIVO_E_INVALID: no livo_std_reset, a non-finite point of a cloud added
 * on the device; LIVO_E_RANGE: a voxel coordinate beyond +-(2^20 - 2).  A refused call leaves the
 * key cloud and the staged frame as they were (but for the staged frame's corner list, which the
 * device-side refusals drop). */
int livo_std_generate(livo_ctx* ctx, const livo_std_gen_params* params, livo_std_gen_stats* stats);
/* The staged frame read back: descriptors, plane cloud and, behind a livo_std_generate, the final
 * corner list (0 behind a livo_std_stage).  Each of the three: NULL with its count pointer set
 * gives the count only; LIVO_E_RANGE: a cap too small.  LIVO_E_INVALID: nothing staged. */
int livo_std_staged(livo_ctx* ctx, livo_std_desc* descs, int64_t desc_cap, int64_t* n_descs, livo_std_plane* planes,
                    int64_t plane_cap, int64_t* n_planes, livo_std_corner* corners, int64_t corner_cap,
                    int64_t* n_corners);
/* For tests only (no caller of the reference's interface needs it; it may change): diagnostics of the
 * last livo_std_generate, in the order the stages made them: per voxel in
 * visiting order its first point's index, point count and plane flag (3 x voxels), and per job
 * its voxel's visiting rank, its direction's plane voxel's rank, the points projected and the 27
 * member ranks + 1 (30 x jobs).  NULL with the count pointer set gives the counts. */
int livo_std_gen_debug(livo_ctx* ctx, int32_t* voxels, int64_t voxel_cap, int64_t* n_voxels, int32_t* jobs,
                       int64_t job_cap, int64_t* n_jobs);

int livo_sync(livo_ctx* ctx);
/* Diagnostics: the incremental map's grid rebuilds since the context was made,
 * out[0] by a sort of every id, out[1] by merging the added ids into the grid;
 * out[2] the Add_Points batches redone with 64-bit box keys (a wrapped-key clash),
 * out[3] the merged rebuilds run inside Add_Points' pass (counted in out[1] too). */
int livo_debug_map_rebuilds(livo_ctx* ctx, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* LIVO_H */
