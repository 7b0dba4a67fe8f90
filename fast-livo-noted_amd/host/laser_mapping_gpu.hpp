// laser_mapping_gpu.hpp — C++ facade over the livo C ABI with the call shape
// of the reference's scan-to-map update (snowflakezzz/FAST-LIVO-noted).
//
// The reference keeps this path inside LaserMapping as private members with
// implicit state:
//
//   ikdtree.Build(feats_down_world->points)      src/laser_mapping.cpp:134-142
//   feats_down_body / feats_down_size            src/laser_mapping.cpp:129-131
//   void h_share_model(MatrixXd &HPH, VectorXd &HPL)
//                                                include/laser_mapping.h:83,
//                                                src/laser_mapping.cpp:485-644
//   the IEKF loop in Run()                       src/laser_mapping.cpp:166-238
//
// LaserMappingGpu holds the same state under the same names (state,
// state_propagat, nearest_search_en, effct_feat_num) and exposes the same two
// operations, so a maintainer swaps the bodies of h_share_model() and of the
// iteration loop for calls into this class.  Matrix and state
// arguments are templates: any type with Eigen's accessors works (the
// reference's MatrixXd / VectorXd / StatesGroup with rot_end(i,j),
// pos_end(i), cov(i,j), ...), and nothing here needs Eigen itself.
//
// Errors: the reference has no error path (it would divide by zero at
// laser_mapping.cpp:561 on an empty match set); the facade throws
// livo::Error carrying the LIVO_E_* code of the failing C-ABI call.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "livo.h"

namespace livo {

class Error : public std::runtime_error {
public:
    Error(const char* what, int code)
        : std::runtime_error(std::string(what) + ": " + livo_error_string(code)), code_(code) {}
    int code() const { return code_; }

private:
    int code_;
};

inline void check(int rc, const char* what) {
    if (rc != LIVO_OK) throw Error(what, rc);
}

// StatesGroup (include/common_lib.h:518-603) <-> livo_state (row-major).
template <class S>
livo_state to_livo_state(const S& s) {
    livo_state o{};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o.rot[3 * i + j] = s.rot_end(i, j);
        o.pos[i] = s.pos_end(i);
        o.vel[i] = s.vel_end(i);
        o.bias_g[i] = s.bias_g(i);
        o.bias_a[i] = s.bias_a(i);
        o.gravity[i] = s.gravity(i);
    }
    for (int i = 0; i < LIVO_DIM_STATE; i++)
        for (int j = 0; j < LIVO_DIM_STATE; j++) o.cov[LIVO_DIM_STATE * i + j] = s.cov(i, j);
    return o;
}

template <class S>
void from_livo_state(const livo_state& o, S& s) {
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) s.rot_end(i, j) = o.rot[3 * i + j];
        s.pos_end(i) = o.pos[i];
        s.vel_end(i) = o.vel[i];
        s.bias_g(i) = o.bias_g[i];
        s.bias_a(i) = o.bias_a[i];
        s.gravity(i) = o.gravity[i];
    }
    for (int i = 0; i < LIVO_DIM_STATE; i++)
        for (int j = 0; j < LIVO_DIM_STATE; j++) s.cov(i, j) = o.cov[LIVO_DIM_STATE * i + j];
}

class LaserMappingGpu {
public:
    // Defaults are the reference's (livo_params_default); `device` is the HIP ordinal.
    explicit LaserMappingGpu(int device = 0, const livo_params* params = nullptr) {
        livo_params p;
        if (params) {
            p = *params;
        } else {
            check(livo_params_default(&p), "livo_params_default");
        }
        check(livo_ctx_create(device, &p, &ctx_), "livo_ctx_create");
        check(livo_params_default(&params_), "livo_params_default");
        params_ = p;
        check(livo_imu_params_default(&imu_params), "livo_imu_params_default");
        check(livo_ingest_params_default(&ingest_params), "livo_ingest_params_default");
    }
    ~LaserMappingGpu() {
        if (ctx_) {
            if (scan_id_ >= 0) livo_scan_release(ctx_, scan_id_);
            livo_ctx_destroy(ctx_);
        }
    }
    LaserMappingGpu(const LaserMappingGpu&) = delete;
    LaserMappingGpu& operator=(const LaserMappingGpu&) = delete;

    // ikdtree.Build(points): x,y,z floats at xyz + i*stride (PointType: stride 48).
    void build_map(const float* xyz, int64_t M, int64_t stride_bytes = 3 * sizeof(float)) {
        check(livo_map_build(ctx_, xyz, M, stride_bytes), "livo_map_build");
    }

    // The compiled default backend: ivox_ = make_shared<IVoxType>(ivox_options_)
    // (laser_mapping.cpp:776, options :1021-1035); h_share_model / iterate then
    // search the iVox map (laser_mapping.cpp:519-521).
    void use_ivox(const livo_ivox_params* options = nullptr) {
        check(livo_ivox_init(ctx_, options), "livo_ivox_init");
        check(livo_ctx_set_backend(ctx_, LIVO_BACKEND_IVOX), "livo_ctx_set_backend");
        ivox_ = true;
    }
    // ivox_->AddPoints(points) (the first scan, laser_mapping.cpp:145-150).
    void ivox_add_points(const float* xyz, int64_t n, int64_t stride_bytes = 3 * sizeof(float)) {
        check(livo_ivox_add_points(ctx_, xyz, n, stride_bytes), "livo_ivox_add_points");
    }

    // feats_down_body for the next update (laser_mapping.cpp:129-131, 164-166).
    // Nearest_Points.resize keeps the previous scan's entries, which only the
    // iVox search can leave in place (ivox3d.h:165-167): carried over then.
    void set_scan(const float* body_xyz, int64_t N, int64_t stride_bytes = 3 * sizeof(float)) {
        int32_t id = -1;
        check(livo_scan_upload(ctx_, body_xyz, N, stride_bytes, &id), "livo_scan_upload");
        adopt_scan(id, N);
    }

    // The raw frame instead: UndistortPcl's per-point de-skew with the frame's
    // IMU poses (IMU_Processing.cpp:340-378) and downSizeFilterSurf
    // (laser_mapping.cpp:129-130) on the device; `down` (optional, cap
    // down_cap) receives feats_down_body.
    void set_scan_raw(const livo_raw_point* raw, int64_t n, const livo_imu_pose* poses, int32_t n_poses,
                      float filter_size_surf, livo_raw_point* down = nullptr, int64_t down_cap = 0) {
        int32_t id = -1;
        int64_t nd = 0;
        check(livo_scan_preprocess(ctx_, raw, n, poses, n_poses, state.rot, state.pos, filter_size_surf, &id,
                                   nullptr, down, down_cap, &nd),
              "livo_scan_preprocess");
        adopt_scan(id, nd);
    }

    // p_imu->Process2(LidarMeasures, state, feats_undistort) behind IMU_init (laser_mapping.cpp:119,
    // IMU_Processing.cpp:381-403): UndistortPcl's forward propagation of `state` over meas.imu
    // (imu_params and imu_carry are ImuProcess's members), state_propagat = state
    // (laser_mapping.cpp:122), and, with n > 0 points, the backward walk and downSizeFilterSurf
    // through the table the propagation left on the device.  n == 0 is the camera frame
    // (is_lidar_end == false, pcl_end_time = lidar_beg_time + img_offset_time): the propagated
    // `state` is then what detectFromPublished() takes.  `down` as set_scan_raw's.
    void Process2(const livo_imu_sample* imu, int32_t n_imu, double pcl_beg_time, double pcl_end_time,
                  const livo_raw_point* raw, int64_t n, float filter_size_surf, livo_raw_point* down = nullptr,
                  int64_t down_cap = 0) {
        livo_imu_job job{};
        job.imu = imu;
        job.n_imu = n_imu;
        job.pcl_beg_time = pcl_beg_time;
        job.pcl_end_time = pcl_end_time;
        check(livo_imu_propagate(ctx_, &job, &imu_params, &imu_carry, &state, nullptr, 0, nullptr),
              "livo_imu_propagate");
        state_propagat = state;
        if (n <= 0) return;
        int32_t id = -1;
        int64_t nd = 0;
        check(livo_scan_preprocess_imu(ctx_, raw, n, filter_size_surf, &id, nullptr, down, down_cap, &nd),
              "livo_scan_preprocess_imu");
        adopt_scan(id, nd);
    }
    // livox_pcl_cbk / standard_pcl_cbk (laser_mapping.cpp) with sync_packages' step 1 (:691-708):
    // p_pre->process(msg, ptr) and the time sort run on the device (ingest_params are Preprocess's
    // members), the frame stays there as meas.lidar with lidar_scan_index_now = 0, and
    // lidar_beg_time = the message's stamp, lidar_end_time = lidar_beg_time + points.back().curvature
    // / 1000 (:707).  `pts` / `data` are the driver's buffers as they are.
    livo_ingest_info livox_pcl_cbk(const livo_livox_point* pts, int64_t n, double stamp) {
        livo_ingest_info info{};
        check(livo_frame_ingest_livox(ctx_, &ingest_params, pts, n, &info), "livo_frame_ingest_livox");
        frame_pushed(info, stamp);
        return info;
    }
    livo_ingest_info standard_pcl_cbk(const void* data, int64_t n, const livo_cloud_layout& layout, double stamp) {
        livo_ingest_info info{};
        check(livo_frame_ingest_cloud(ctx_, &ingest_params, data, n, &layout, &info), "livo_frame_ingest_cloud");
        frame_pushed(info, stamp);
        return info;
    }

    // Process2 on the frame the callback left on the device: UndistortPcl's times (:211, :219-224)
    // from lidar_beg_time, last_update_time and the frame's end, the forward propagation, and the
    // slice from lidar_scan_index_now, which never comes to the host.  is_lidar_end: the LiDAR
    // frame's end (the slice is de-skewed, filtered and becomes the current scan; `down` as
    // set_scan_raw's); else a camera frame at lidar_beg_time + img_offset_time, whose slice only
    // moves the cursor (Run() never reads its feats_undistort).  Returns the points taken.
    int64_t Process2(const livo_imu_sample* imu, int32_t n_imu, bool is_lidar_end, double img_offset_time,
                     float filter_size_surf, livo_raw_point* down = nullptr, int64_t down_cap = 0) {
        const double pcl_beg_time = lidar_beg_time > last_update_time ? lidar_beg_time : last_update_time;
        const double pcl_end_time = is_lidar_end ? lidar_beg_time + frame_end_curvature / double(1000)
                                                 : lidar_beg_time + img_offset_time;
        const double pcl_offset_time = is_lidar_end ? (pcl_end_time - lidar_beg_time) * double(1000) : 0.0;
        livo_imu_job job{};
        job.imu = imu;
        job.n_imu = n_imu;
        job.pcl_beg_time = pcl_beg_time;
        job.pcl_end_time = pcl_end_time;
        check(livo_imu_propagate(ctx_, &job, &imu_params, &imu_carry, &state, nullptr, 0, nullptr),
              "livo_imu_propagate");
        state_propagat = state;
        last_update_time = pcl_end_time;  // (:231)
        int32_t id = -1;
        int64_t nd = 0, taken = 0;
        check(livo_frame_take(ctx_, pcl_offset_time, is_lidar_end ? 1 : 0, filter_size_surf,
                              is_lidar_end ? &id : nullptr, nullptr, down, down_cap, &nd, &taken),
              "livo_frame_take");
        if (id >= 0) adopt_scan(id, nd);
        return taken;
    }

    // The LIO half of Run() on a LiDAR frame (laser_mapping.cpp:37-284) as one call on the frame the
    // callback left on the device: Process2(..., is_lidar_end = true, ...), the first scan's map
    // (flg_first_scan: cleared once a scan has built / filled it), iterate() behind flg_EKF_inited,
    // map_incremental() and publish_cloud(), with `state` on the device in between: it comes to the
    // host once, at the end, with state_propagat.  Returns the call's statistics; the members
    // the separate methods set (state, state_propagat, imu_carry, last_update_time, the current scan,
    // flg_EKF_converged, effct_feat_num, points_added, points_no_downsample) are set as they set them.
    livo_lio_stats RunLidarFrame(const livo_imu_sample* imu, int32_t n_imu, float filter_size_surf,
                                 double filter_size_map_min, bool flg_EKF_inited = true, bool dense_map_en = true,
                                 float match_leaf = 0.2f) {
        const double pcl_beg_time = lidar_beg_time > last_update_time ? lidar_beg_time : last_update_time;
        const double pcl_end_time = lidar_beg_time + frame_end_curvature / double(1000);
        const double pcl_offset_time = (pcl_end_time - lidar_beg_time) * double(1000);
        livo_imu_job job{};
        job.imu = imu;
        job.n_imu = n_imu;
        job.pcl_beg_time = pcl_beg_time;
        job.pcl_end_time = pcl_end_time;
        livo_lio_params p{};
        p.filter_size_surf = filter_size_surf;
        p.match_leaf = match_leaf;
        p.filter_size_map_min = filter_size_map_min;
        p.ekf_inited = flg_EKF_inited ? 1 : 0;
        p.first_scan = flg_first_scan ? 1 : 0;
        p.dense_map_en = dense_map_en ? 1 : 0;
        p.prev_scan_id = scan_id_;
        livo_lio_stats st{};
        check(livo_lio_frame(ctx_, &job, &imu_params, &imu_carry, pcl_offset_time, &p, &state, &state_propagat, &st),
              "livo_lio_frame");
        last_update_time = pcl_end_time;  // (:231)
        if (st.stage == LIVO_LIO_FIRST_SCAN) {
            adopt_scan(st.scan_id, st.n_down);  // (the call leaves the previous scan to its owner here)
            if (st.map_built) flg_first_scan = false;
        } else if (st.stage == LIVO_LIO_UPDATED) {
            scan_id_ = st.scan_id;  // (the previous one was inherited from and released inside the call)
            feats_down_size = st.n_down;
            nearest_search_en = true;
            if (flg_EKF_inited) {
                flg_EKF_converged = st.iter.converged != 0;
                if (st.iter.iterations > 0) effct_feat_num = st.iter.effct_feat_num[st.iter.iterations - 1];
            }
            points_added = st.map_counts[0];
            points_no_downsample = st.map_counts[1];
        }
        return st;
    }

    // p_imu->IMU_init(meas, state, init_iter_num) (IMU_Processing.cpp:147-198) while imu_need_init:
    // returns true once gravity and bias_g are set (imu_need_init_ = false).
    bool IMU_init(const livo_imu_sample* imu, int32_t n_imu) {
        int32_t status = LIVO_IMU_INIT_COLLECTING;
        check(livo_imu_init(ctx_, imu, n_imu, &imu_params, &init_iter_num, mean_gyr, &state, &status), "livo_imu_init");
        if (status == LIVO_IMU_INIT_RESET) {
            imu_carry = livo_imu_carry{};  // Reset(): angvel_last, last_imu_
        } else if (n_imu > 0) {
            imu_carry.last_imu = imu[n_imu - 1];  // :149
        }
        return status == LIVO_IMU_INIT_DONE;
    }

    // map_incremental() (laser_mapping.cpp:329-389) at the updated state: the iVox branch
    // (counts = added, added without downsampling) or, on the ikd-Tree backend, Add_Points
    // of every point (:383-384; counts = Add_Points' return value, points deleted).
    void map_incremental(double filter_size_map_min, bool flg_EKF_inited = true) {
        int64_t counts[2] = {0, 0};
        check(livo_map_incremental(ctx_, scan_id_, &state, filter_size_map_min, flg_EKF_inited ? 1 : 0, nullptr,
                                   counts),
              "livo_map_incremental");
        points_added = counts[0];
        points_no_downsample = counts[1];
    }

    // Run()'s tail (laser_mapping.cpp:258-268): *pcl_wait_pub = *laserCloudWorld, the frame
    // (dense_map_en: the last set_scan_raw frame at full resolution, else the current
    // feats_down_body) at the LIO-updated `state`, kept on the device for every camera frame
    // until the next LiDAR frame ends: detectFromPublished() reads it at the state the IMU
    // has propagated to the image's time.  match_leaf > 0 also builds the pg_down that each
    // detect filters out of it (lidar_selection.cpp:7, 341-344); call it after map_incremental().
    livo_cloud_info publish_cloud(bool dense_map_en = true, float match_leaf = 0.2f) {
        if (!dense_map_en && scan_id_ < 0) throw Error("publish_cloud", LIVO_E_NOSCAN);
        livo_cloud_info info{};
        check(livo_cloud_publish(ctx_, dense_map_en ? -1 : scan_id_, &state, match_leaf, &info), "livo_cloud_publish");
        return info;
    }

    template <class S>
    void set_state(const S& s) { state = to_livo_state(s); }
    template <class S>
    void set_state_propagat(const S& s) { state_propagat = to_livo_state(s); }
    template <class S>
    void get_state(S& s) const { from_livo_state(state, s); }

    // h_share_model(HPH, HPL) (laser_mapping.cpp:485-644): HPH is resized to
    // 9x9 and HPL to 9 exactly as the reference does; effct_feat_num is set;
    // the k-NN runs iff nearest_search_en, else cached neighbours are reused.
    template <class MatX, class VecX>
    void h_share_model(MatX& HPH, VecX& HPL) {
        double hth[81], htl[9];
        int64_t eff = 0;
        check(livo_h_share(ctx_, scan_id_, &state, nearest_search_en ? 1 : 0, hth, htl, &eff, nullptr),
              "livo_h_share");
        HPH.resize(9, 9);
        HPL.resize(9);
        for (int i = 0; i < 9; i++) {
            for (int j = 0; j < 9; j++) HPH(i, j) = hth[9 * i + j];
            HPL(i) = htl[i];
        }
        effct_feat_num = eff;
    }

    // The iteration loop of Run() (laser_mapping.cpp:166-238) for the current
    // scan: state is updated in place from prior state_propagat; the final
    // covariance update (I - G) P is included.  Returns the loop's statistics.
    livo_iter_stats iterate() {
        livo_iter_stats st{};
        check(livo_iekf_update(ctx_, scan_id_, &state, &state_propagat, &st), "livo_iekf_update");
        flg_EKF_converged = st.converged != 0;
        if (st.iterations > 0) effct_feat_num = st.effct_feat_num[st.iterations - 1];
        return st;
    }

    // publish_frame_world_rgb() (laser_mapping.cpp:1351-1381) up to the publisher: the
    // cloud of pcl_wait_pub at `state` (dense_map_en: the last set_scan_raw frame at full
    // resolution, else the current feats_down_body) projected into the camera of
    // `vio` (cam, R_ci, P_ci) and coloured from img_rgb (lidar_selector->img_rgb: 8-bit
    // B, G, R, row stride 3 * width).  Fills laserCloudWorldRGB with the kept points in
    // the cloud's order; img_rgb == nullptr reuses the image of the previous call (the
    // frame's image colours the dense and the downsampled cloud with one upload).
    livo_rgb_stats publish_frame_world_rgb(const livo_vio_params& vio, const uint8_t* img_rgb, int32_t width,
                                           int32_t height, std::vector<livo_rgb_point>& laserCloudWorldRGB,
                                           bool dense_map_en = true) {
        if (!dense_map_en && scan_id_ < 0) throw Error("publish_frame_world_rgb", LIVO_E_NOSCAN);
        const int32_t id = dense_map_en ? -1 : scan_id_;
        int64_t n = 0;
        check(livo_frame_to_world(ctx_, id, &state, nullptr, 0, &n), "livo_frame_to_world");  // the cloud's size
        laserCloudWorldRGB.resize((size_t)n);
        livo_rgb_stats st{};
        check(livo_cloud_colorize(ctx_, id, &state, &vio, img_rgb, width, height, laserCloudWorldRGB.data(), nullptr,
                                  n, &n, &st),
              "livo_cloud_colorize");
        laserCloudWorldRGB.resize((size_t)n);
        return st;
    }

    // lidar_selector->addSparseMap(img, pg) (lidar_selection.cpp:140-193): pg is the same
    // cloud publish_frame_world_rgb takes (dense_map_en: the last set_scan_raw frame at
    // full resolution, else the current feats_down_body) at `state`, img the 8-bit gray
    // image (row stride width; nullptr reuses the image of the previous call).  Fills
    // `points` with the best-scored point of each grid_size cell, in ascending cell
    // order, and `patches` with their level 0, 1, 2 patches (3 * patch_size^2 floats a
    // point, Feature::patch layout) as livo_vio_update reads them; what the reference
    // files in feat_map is points[k].voxel -> (points[k], patches of k).
    livo_vis_stats addSparseMap(const livo_vio_params& vio, const uint8_t* img, int32_t width, int32_t height,
                                int32_t grid_size, std::vector<livo_vis_point>& points, std::vector<float>& patches,
                                bool dense_map_en = true) {
        if (!dense_map_en && scan_id_ < 0) throw Error("addSparseMap", LIVO_E_NOSCAN);
        const int32_t id = dense_map_en ? -1 : scan_id_;
        int64_t n = 0;
        livo_vis_stats st{};
        check(livo_vio_select(ctx_, id, &state, &vio, grid_size, img, width, height, nullptr, nullptr, 0, &n, &st),
              "livo_vio_select");  // the sizing call (it uploads the image)
        const size_t per = (size_t)3 * (size_t)vio.patch_size * (size_t)vio.patch_size;
        points.resize((size_t)n);
        patches.resize((size_t)n * per);
        if (n > 0)
            check(livo_vio_select(ctx_, id, &state, &vio, grid_size, nullptr, width, height, points.data(),
                                  patches.data(), n, &n, &st),
                  "livo_vio_select");
        return st;
    }

    // lidar_selector->addFromSparseMap(img, pg) (lidar_selection.cpp:332-593) on the resident
    // visual map (livo_vmap_reset / livo_vmap_add_frame / livo_vmap_add): pg and img as
    // addSparseMap takes them (the image in a buffer of this stage's own; nullptr reuses the
    // previous call's).  Fills sub_sparse_map's arrays as livo_vio_update reads them:
    // `pos` (3 doubles a point), `search_levels`, `patches` (3 * patch_size^2 floats a point),
    // and `points` (the records: map point, cell, observation, error), in ascending cell order.
    livo_vmatch_stats addFromSparseMap(const livo_vio_params& vio, const uint8_t* img, int32_t width, int32_t height,
                                       int32_t grid_size, bool ncc_en, double ncc_thre, double outlier_threshold,
                                       std::vector<livo_vmatch_point>& points, std::vector<double>& pos,
                                       std::vector<int32_t>& search_levels, std::vector<float>& patches,
                                       bool dense_map_en = true) {
        if (!dense_map_en && scan_id_ < 0) throw Error("addFromSparseMap", LIVO_E_NOSCAN);
        const int32_t id = dense_map_en ? -1 : scan_id_;
        int64_t n = 0;
        livo_vmatch_stats st{};
        check(livo_vio_match(ctx_, id, &state, &vio, grid_size, ncc_en ? 1 : 0, ncc_thre, outlier_threshold, img, width,
                             height, nullptr, nullptr, nullptr, nullptr, 0, &n, &st),
              "livo_vio_match");  // the sizing call (it uploads the image and leaves the map as it is)
        const size_t per = (size_t)3 * (size_t)vio.patch_size * (size_t)vio.patch_size;
        points.resize((size_t)n);
        pos.resize((size_t)n * 3);
        search_levels.resize((size_t)n);
        patches.resize((size_t)n * per);
        if (n > 0)
            check(livo_vio_match(ctx_, id, &state, &vio, grid_size, ncc_en ? 1 : 0, ncc_thre, outlier_threshold, nullptr,
                                 width, height, points.data(), pos.data(), search_levels.data(), patches.data(), n, &n,
                                 &st),
                  "livo_vio_match");
        return st;
    }

    // lidar_selector->addObservation(img) (lidar_selection.cpp:905-962) on the resident visual
    // map: `points` are the records addFromSparseMap returned for this frame (sub_sparse_map's
    // voxel_points and search_levels), frame_id the frame stored with livo_vmap_add_frame at
    // the state after the update (new_frame_ after updateFrameState; its stored image is img).
    // `records`, if given, takes one livo_vobs_point per point, in the same order.
    livo_vobs_stats addObservation(int32_t frame_id, const std::vector<livo_vmatch_point>& points,
                                   std::vector<livo_vobs_point>* records = nullptr) {
        std::vector<int32_t> ids(points.size()), levels(points.size());
        for (size_t k = 0; k < points.size(); k++) {
            ids[k] = points[k].point_id;
            levels[k] = points[k].search_level;
        }
        if (records) records->resize(points.size());
        livo_vobs_stats st{};
        check(livo_vio_observe(ctx_, frame_id, (int64_t)points.size(), ids.data(), levels.data(),
                               records ? records->data() : nullptr, &st),
              "livo_vio_observe");
        return st;
    }

    // lidar_selector->detect(img, pg) (lidar_selection.cpp:1024-1073) behind its image
    // conversion, as one call on the resident visual map: addFromSparseMap and addSparseMap at
    // `state`, ComputeJ on the matches (state_propagat the prior; `state` is updated in place),
    // the frame stored under frame_id at the updated state with img, addObservation of the
    // matches and the new points added, pg and img as addSparseMap takes them (img is
    // required).  Nothing of the stages' results comes to the host; the statistics do.
    livo_vdetect_stats detect(const livo_vio_params& vio, const uint8_t* img, int32_t width, int32_t height,
                              int32_t frame_id, int32_t grid_size, bool ncc_en, double ncc_thre,
                              double outlier_threshold, bool dense_map_en = true) {
        if (!dense_map_en && scan_id_ < 0) throw Error("detect", LIVO_E_NOSCAN);
        livo_vdetect_params d{};
        d.grid_size = grid_size;
        d.ncc_en = ncc_en ? 1 : 0;
        d.ncc_thre = ncc_thre;
        d.outlier_threshold = outlier_threshold;
        livo_vdetect_stats st{};
        check(livo_vio_detect(ctx_, dense_map_en ? -1 : scan_id_, frame_id, &state, &state_propagat, &vio, &d, img,
                              width, height, &st),
              "livo_vio_detect");
        return st;
    }

    // lidar_selector->detect(img, pcl_wait_pub) (laser_mapping.cpp:93) on the cloud of
    // publish_cloud(): `state` places the camera only, addFromSparseMap reads pg_down where
    // it was built and addSparseMap the full cloud.
    livo_vdetect_stats detectFromPublished(const livo_vio_params& vio, const uint8_t* img, int32_t width,
                                           int32_t height, int32_t frame_id, int32_t grid_size, bool ncc_en,
                                           double ncc_thre, double outlier_threshold) {
        livo_vdetect_params d{};
        d.grid_size = grid_size;
        d.ncc_en = ncc_en ? 1 : 0;
        d.ncc_thre = ncc_thre;
        d.outlier_threshold = outlier_threshold;
        livo_vdetect_stats st{};
        check(livo_vio_detect(ctx_, LIVO_CLOUD_WORLD, frame_id, &state, &state_propagat, &vio, &d, img, width, height,
                              &st),
              "livo_vio_detect");
        return st;
    }

    // The stored frames that no observation refers to any more give their slots back (the
    // reference never frees imgs_; this map has a fixed frame store).  -> their ids, ascending
    std::vector<int32_t> releaseFrames() {
        int64_t n = 0;
        check(livo_vmap_release_frames(ctx_, nullptr, 0, &n), "livo_vmap_release_frames");
        std::vector<int32_t> ids((size_t)n);
        if (n > 0) check(livo_vmap_release_frames(ctx_, ids.data(), n, &n), "livo_vmap_release_frames");
        ids.resize((size_t)n);
        return ids;
    }

    // ---- Loop closure (LaserMapping::loop_detect, laser_mapping.cpp:1223-1349): STDescManager's
    // database on the device.  GenerateSTDescs runs there too (loop_detect); StdStage takes a host's products. ----
    struct LoopResult {
        int frame = -1;          // loop_result.first
        double score = 0.0;      // loop_result.second
        double rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // loop_transform.second, row-major
        double t[3] = {0, 0, 0};                      // loop_transform.first
        std::vector<livo_std_pair> pairs;             // loop_std_pair, as indices (staged, stored)
        int n_candidates = 0;
    };

    // STDescManager(config): an empty database (read_parameters' defaults where config is null)
    void StdReset(int64_t max_descs, int64_t max_frames, int64_t max_planes, const livo_std_params* config = nullptr) {
        livo_std_params p;
        check(livo_std_params_default(&p), "livo_std_params_default");
        check(livo_std_reset(ctx_, config ? config : &p, max_descs, max_frames, max_planes), "livo_std_reset");
    }
    // the hand-off of GenerateSTDescs(cloud, stds_vec): the key frame's descriptors and plane cloud
    void StdStage(const std::vector<livo_std_desc>& stds_vec, const std::vector<livo_std_plane>& plane_cloud) {
        check(livo_std_stage(ctx_, stds_vec.data(), (int64_t)stds_vec.size(), plane_cloud.data(),
                             (int64_t)plane_cloud.size()),
              "livo_std_stage");
        staged_descs_ = (int64_t)stds_vec.size();
    }
    // std_manager->SearchLoop(stds_vec, loop_result, loop_transform, loop_std_pair) on the staged frame
    LoopResult SearchLoop() {
        LoopResult out;
        livo_std_result r{};
        int64_t n = 0;
        out.pairs.resize((size_t)(staged_descs_ * 27));
        check(livo_std_search(ctx_, &r, out.pairs.data(), (int64_t)out.pairs.size(), &n), "livo_std_search");
        if (n > (int64_t)out.pairs.size()) {  // (a cell's run may hold several matches of one descriptor)
            out.pairs.resize((size_t)n);
            check(livo_std_search(ctx_, &r, out.pairs.data(), n, &n), "livo_std_search");
        }
        out.pairs.resize((size_t)n);
        out.frame = r.frame;
        out.score = r.score;
        for (int i = 0; i < 9; i++) out.rot[i] = r.rot[i];
        for (int i = 0; i < 3; i++) out.t[i] = r.t[i];
        out.n_candidates = r.n_candidates;
        return out;
    }
    // std_manager->AddSTDescs(stds_vec) of the staged frame -> its frame index
    int32_t AddSTDescs() {
        int32_t frame = -1;
        check(livo_std_commit(ctx_, &frame), "livo_std_commit");
        return frame;
    }

    // The loop detection of a LiDAR frame (laser_mapping.cpp:1239-1262): the frame's world cloud joins the key
    // cloud; every sub_frame_num frames GenerateSTDescs runs on it, SearchLoop when more than skip_near_num key
    // frames are stored, then AddSTDescs.  -> true when a key frame was made (out, may be null, holds its search).
    bool loop_detect(int sub_frame_num, int skip_near_num, const livo_std_gen_params* config = nullptr,
                     LoopResult* out = nullptr, livo_std_gen_stats* stats = nullptr) {
        check(livo_std_key_add(ctx_, LIVO_CLOUD_WORLD), "livo_std_key_add");
        if (++key_frames_pending_ < sub_frame_num) return false;
        key_frames_pending_ = 0;
        livo_std_gen_params p;
        check(livo_std_gen_params_default(&p), "livo_std_gen_params_default");
        livo_std_gen_stats st{};
        check(livo_std_generate(ctx_, config ? config : &p, &st), "livo_std_generate");
        staged_descs_ = st.descs;
        if (stats) *stats = st;
        LoopResult none;
        livo_std_info info{};
        check(livo_std_info_get(ctx_, &info), "livo_std_info_get");
        if (out) *out = info.frames > skip_near_num ? SearchLoop() : none;
        AddSTDescs();
        return true;
    }

    livo_ctx* ctx() const { return ctx_; }
    const livo_params& params() const { return params_; }

    // Reference member names (laser_mapping.h): the implicit state of the path.
    livo_state state{};
    livo_state state_propagat{};
    bool nearest_search_en = true;
    bool flg_EKF_converged = false;
    bool flg_first_scan = false;  // RunLidarFrame: the next frame builds / fills the map (set it for a session without one)
    int64_t effct_feat_num = 0;
    int64_t feats_down_size = 0;
    int64_t points_added = 0, points_no_downsample = 0;  // last map_incremental
    // ImuProcess's members (IMU_Processing.h): the noise terms and mean_acc, what UndistortPcl
    // keeps between calls, and IMU_init's counters
    livo_imu_params imu_params{};
    livo_imu_carry imu_carry{};
    int32_t init_iter_num = 1;
    double mean_gyr[3] = {0.0, 0.0, 0.0};
    // Preprocess's members (lidar_type, N_SCANS, point_filter_num, blind) and LidarMeasureGroup's
    // times: the current frame's stamp, its end (sync_packages :707) and last_update_time
    livo_ingest_params ingest_params{};
    double lidar_beg_time = 0.0, lidar_end_time = 0.0, last_update_time = 0.0;
    float frame_end_curvature = 0.f;  // meas.lidar->points.back().curvature (ms)

private:
    void frame_pushed(const livo_ingest_info& info, double stamp) {
        frame_end_curvature = info.end_curvature;
        lidar_beg_time = stamp;
        lidar_end_time = lidar_beg_time + info.end_curvature / double(1000);
    }
    void adopt_scan(int32_t id, int64_t N) {
        if (scan_id_ >= 0) {
            if (ivox_) check(livo_scan_inherit_neighbors(ctx_, id, scan_id_), "livo_scan_inherit_neighbors");
            check(livo_scan_release(ctx_, scan_id_), "livo_scan_release");
        }
        scan_id_ = id;
        feats_down_size = N;
        nearest_search_en = true;
    }

    livo_ctx* ctx_ = nullptr;
    livo_params params_{};
    int32_t scan_id_ = -1;
    bool ivox_ = false;
    int64_t staged_descs_ = 0;
    int key_frames_pending_ = 0;       // frames in the key cloud since the last key frame (loop_detect)
};

}  // namespace livo
