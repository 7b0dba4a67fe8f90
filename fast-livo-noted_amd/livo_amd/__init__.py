"""livo_amd — Python binding of the MI355X LIO scan-to-map C ABI (include/livo.h).

A thin ctypes layer over fast-livo-noted_amd/lib/liblivo_hip.so used by the
tests, smoke() and bench.py.  It mirrors the reference call surface for this
path:

    KD_TREE::Build / Nearest_Search      -> Context.map_build / Context.knn
    LaserMapping::h_share_model          -> Context.h_share
    IVox (AddPoints / GetClosestPoint)   -> Context.ivox_init / ivox_add_points / ivox_knn
    LaserMapping::map_incremental        -> Context.map_incremental
    IEKF loop of LaserMapping::Run       -> Context.iekf_update(_batch)
    LaserMapping::publish_frame_world_rgb -> Context.colorize
    LidarSelector::addSparseMap          -> Context.vio_select
    feat_map / imgs_ (the visual map)    -> Context.vmap_reset / vmap_add_frame / vmap_add / vmap_dump
    LidarSelector::addFromSparseMap      -> Context.vio_match
    LidarSelector::addObservation        -> Context.vio_observe
    LidarSelector::detect (one frame)    -> Context.vio_detect, Context.vmap_release_frames
    pcl_wait_pub / pg_down (Run's tail)  -> Context.cloud_publish, CLOUD_WORLD, CLOUD_WORLD_DOWN
    ImuProcess::IMU_init                 -> imu_init
    ImuProcess::UndistortPcl (forward)   -> Context.imu_propagate(_batch), Context.scan_preprocess_imu

There is no CPU fallback: loading fails loudly if the HIP library is missing,
and every compute call raises LivoError when the GPU path fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("LIVO_LIB") or os.path.join(PKG_ROOT, "lib", "liblivo_hip.so")  # LIVO_LIB: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "livo.h")

DIM_STATE = 18
NUM_MATCH_POINTS = 5
MAX_EVALS = 16

LIVO_OK = 0
ERRORS = {-1: "LIVO_E_INVALID", -2: "LIVO_E_HIP", -3: "LIVO_E_NOMAP", -4: "LIVO_E_NOSCAN", -5: "LIVO_E_OOM",
          -6: "LIVO_E_RANGE", -7: "LIVO_E_CAPACITY", -8: "LIVO_E_BUSY"}
MAX_INFLIGHT = 2  # LIVO_MAX_INFLIGHT
BACKEND_IKDTREE = 0  # -DUSE_ikdtree build (CMakeLists.txt:15)
BACKEND_IVOX = 1     # the reference's default build: faster_lio::IVox
CLOUD_WORLD = 0x40000000       # LIVO_CLOUD_WORLD: the published world cloud as a frame stage's scan_id
CLOUD_WORLD_DOWN = 0x40000001  # LIVO_CLOUD_WORLD_DOWN: its pg_down


class LivoError(RuntimeError):
    def __init__(self, fn, code):
        self.code = code
        super().__init__(f"{fn} failed: {ERRORS.get(code, code)} ({code})")


class Params(C.Structure):
    _fields_ = [("laser_point_cov", C.c_double), ("R_LI", C.c_double * 9), ("t_LI", C.c_double * 3),
                ("max_residual", C.c_double), ("plane_threshold", C.c_float), ("max_nn_sqdist", C.c_float),
                ("max_iterations", C.c_int32), ("flags", C.c_int32)]


class State(C.Structure):
    _fields_ = [("rot", C.c_double * 9), ("pos", C.c_double * 3), ("vel", C.c_double * 3),
                ("bias_g", C.c_double * 3), ("bias_a", C.c_double * 3), ("gravity", C.c_double * 3),
                ("cov", C.c_double * 324)]


class IterStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("knn_passes", C.c_int32), ("converged", C.c_int32),
                ("rematch_num", C.c_int32), ("effct_feat_num", C.c_int64 * MAX_EVALS),
                ("solution", (C.c_double * 18) * MAX_EVALS), ("res_mean", C.c_double * MAX_EVALS)]


class MapInfo(C.Structure):
    _fields_ = [("num_points", C.c_int64), ("depth", C.c_int32), ("ball_chunks", C.c_int32),
                ("num_slots", C.c_int64), ("device_bytes", C.c_int64), ("ball_entries", C.c_int64)]


class PointOut(C.Structure):
    _fields_ = [("normvec", C.c_void_p), ("selected", C.c_void_p), ("nn_idx", C.c_void_p),
                ("nn_sqdist", C.c_void_p), ("world_xyz", C.c_void_p), ("visits", C.c_void_p),
                ("ori_xyz", C.c_void_p), ("corr_normvec", C.c_void_p), ("n_ori", C.c_void_p)]


class Timings(C.Structure):
    _fields_ = [("knn_ms", C.c_double), ("rematch_knn_ms", C.c_double), ("plane_ms", C.c_double),
                ("solve_ms", C.c_double),
                ("knn_launches", C.c_int64), ("knn_visits", C.c_int64), ("knn_queries", C.c_int64),
                ("effct_points", C.c_int64), ("knn_replays", C.c_int64), ("knn_points", C.c_int64),
                ("eval_ms", C.c_double * 16), ("eval_searched", C.c_int32 * 16), ("n_evals", C.c_int32),
                ("reserved_", C.c_int32), ("batch_ms", C.c_double), ("gap_ms", C.c_double)]


# every entry point of include/livo.h, with its ctypes signature
_P = C.c_void_p
IKN = 23  # LIVO_IKFOM_DOF


class IkfomState(C.Structure):
    """livo_ikfom_state: state_ikfom with quaternions (w, x, y, z) and the S2 gravity vector."""
    _fields_ = [("pos", C.c_double * 3), ("rot", C.c_double * 4), ("offset_R", C.c_double * 4),
                ("offset_T", C.c_double * 3), ("vel", C.c_double * 3), ("bg", C.c_double * 3),
                ("ba", C.c_double * 3), ("grav", C.c_double * 3), ("cov", C.c_double * (IKN * IKN))]


class IkfomStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("knn_passes", C.c_int32), ("converged", C.c_int32),
                ("t", C.c_int32), ("effct_feat_num", C.c_int64 * 16), ("dx", (C.c_double * IKN) * 16),
                ("res_mean", C.c_double * 16)]


_IK_FIELDS = (("pos", 3), ("rot", 4), ("offset_R", 4), ("offset_T", 3), ("vel", 3), ("bg", 3), ("ba", 3),
              ("grav", 3))


def ikfom_to_c(st: dict) -> IkfomState:
    s = IkfomState()
    for k, n in _IK_FIELDS:
        getattr(s, k)[:] = np.asarray(st[k], np.float64).reshape(n).tolist()
    s.cov[:] = np.asarray(st["cov"], np.float64).reshape(IKN * IKN).tolist()
    return s


def ikfom_from_c(s: IkfomState) -> dict:
    out = {k: np.array(getattr(s, k)[:]) for k, _ in _IK_FIELDS}
    out["cov"] = np.array(s.cov[:]).reshape(IKN, IKN)
    return out


def ikfom_stats_from_c(st: IkfomStats) -> dict:
    ne = st.iterations
    return {"iterations": ne, "knn_passes": st.knn_passes, "converged": st.converged, "t": st.t,
            "effct_feat_num": [st.effct_feat_num[i] for i in range(min(ne, 16))],
            "dx": np.array([list(st.dx[i]) for i in range(min(ne, 16))]),
            "res_mean": [st.res_mean[i] for i in range(min(ne, 16))]}


class IvoxParams(C.Structure):
    _fields_ = [("resolution", C.c_float), ("nearby_type", C.c_int32), ("capacity", C.c_int64)]


class IvoxInfo(C.Structure):
    _fields_ = [("num_points", C.c_int64), ("num_grids", C.c_int64), ("ids_issued", C.c_int64),
                ("max_grid_points", C.c_int64), ("device_bytes", C.c_int64), ("add_passes", C.c_int64)]


class Cam(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("d", C.c_double * 5), ("width", C.c_int32), ("height", C.c_int32)]


class VioParams(C.Structure):
    _fields_ = [("cam", Cam), ("R_ci", C.c_double * 9), ("P_ci", C.c_double * 3), ("img_point_cov", C.c_double),
                ("patch_size", C.c_int32), ("max_iterations", C.c_int32)]


class VioStats(C.Structure):
    _fields_ = [("iterations", C.c_int32 * 3), ("updates", C.c_int32 * 3), ("last_error", C.c_float * 3),
                ("cov_updated", C.c_int32), ("n_meas", C.c_int64), ("out_of_frame", C.c_int64)]


class RgbPoint(C.Structure):
    """livo_rgb_point: one point of the coloured world cloud (PointXYZRGB's x, y, z, r, g, b)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float),
                ("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("a", C.c_uint8)]


RGB_POINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32),
                            ("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("a", np.uint8)])


class RgbStats(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_out", C.c_int64), ("behind", C.c_int64), ("out_of_frame", C.c_int64),
                ("edge_reads", C.c_int64)]


class VisPoint(C.Structure):
    """livo_vis_point: one new visual map point of addSparseMap (64 bytes)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("score", C.c_float),
                ("u", C.c_double), ("v", C.c_double), ("src_index", C.c_int32), ("cell", C.c_int32),
                ("voxel", C.c_int64 * 3)]


VIS_POINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("score", np.float32),
                            ("u", np.float64), ("v", np.float64), ("src_index", np.int32), ("cell", np.int32),
                            ("voxel", np.int64, (3,))])


class VisStats(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("in_frame", C.c_int64), ("behind_in_frame", C.c_int64),
                ("cell_overflow", C.c_int64), ("n_out", C.c_int64), ("n_cells", C.c_int64)]


class VmapCounts(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_obs", C.c_int64), ("n_frames", C.c_int64), ("max_points", C.c_int64),
                ("max_frames", C.c_int64), ("patch_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("pad_", C.c_int32)]


VMAP_POINT_DTYPE = np.dtype([("pos", np.float64, (3,)), ("value", np.float32), ("n_obs", np.int32),
                             ("voxel", np.int64, (3,)), ("first_obs", np.int64)])
VMAP_OBS_DTYPE = np.dtype([("frame_id", np.int32), ("level", np.int32), ("px", np.float64, (2,)),
                           ("f", np.float64, (3,))])
VMATCH_POINT_DTYPE = np.dtype([("point_id", np.int32), ("cell", np.int32), ("obs_index", np.int32),
                               ("frame_id", np.int32), ("search_level", np.int32), ("error", np.float32),
                               ("ncc", np.float64), ("u", np.float64), ("v", np.float64)])


class VmatchStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in (
        "n_in", "n_voxels", "map_tested", "in_frame", "cell_overflow", "cells_marked", "depth_rejected",
        "view_rejected", "ncc_rejected", "error_rejected", "warp_shared", "warp_nan", "n_out")]


VOBS_POINT_DTYPE = np.dtype([("point_id", np.int32), ("flags", np.int32), ("n_obs", np.int32),
                             ("deleted_index", np.int32), ("deleted_frame_id", np.int32), ("score", np.float32),
                             ("u", np.float64), ("v", np.float64), ("delta_p", np.float64),
                             ("pixel_dist", np.float64)])
VOBS_BEHIND, VOBS_OUT_OF_FRAME, VOBS_POSE, VOBS_PIXEL, VOBS_DELETED, VOBS_ADDED = 1, 2, 4, 8, 16, 32  # LIVO_VOBS_*


class VobsStats(C.Structure):
    _fields_ = [(f, C.c_int64) for f in (
        "n_in", "behind", "out_of_frame", "pose_flagged", "pixel_flagged", "added", "deleted", "deleted_without_add",
        "n_obs_total")]


class VdetectParams(C.Structure):
    _fields_ = [("grid_size", C.c_int32), ("ncc_en", C.c_int32), ("ncc_thre", C.c_double),
                ("outlier_threshold", C.c_double)]


class VdetectStats(C.Structure):
    _fields_ = [("match", VmatchStats), ("select", VisStats), ("update", VioStats), ("observe", VobsStats),
                ("n_matched", C.c_int64), ("n_new", C.c_int64), ("first_new_id", C.c_int32), ("pad_", C.c_int32)]


class CloudInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_down", C.c_int64), ("down_filtered", C.c_int32), ("pad_", C.c_int32),
                ("device_bytes", C.c_int64)]


class LioParams(C.Structure):
    _fields_ = [("filter_size_surf", C.c_float), ("match_leaf", C.c_float), ("filter_size_map_min", C.c_double),
                ("ekf_inited", C.c_int32), ("first_scan", C.c_int32), ("dense_map_en", C.c_int32),
                ("prev_scan_id", C.c_int32)]


LIO_EMPTY, LIO_FIRST_SCAN, LIO_UPDATED = 0, 1, 2  # LIVO_LIO_*


class LioStats(C.Structure):
    _fields_ = [("stage", C.c_int32), ("scan_id", C.c_int32), ("n_taken", C.c_int64), ("n_down", C.c_int64),
                ("map_built", C.c_int32), ("pad_", C.c_int32), ("iter", IterStats), ("map_counts", C.c_int64 * 2),
                ("cloud", CloudInfo)]


def _stats_dict(st) -> dict:
    """A stats struct as a dict (arrays as lists)."""
    out = {}
    for f, _ in st._fields_:
        v = getattr(st, f)
        out[f] = list(v) if hasattr(v, "__len__") else v
    return out


def vio_params(cam: dict, Rci, Pci) -> VioParams:
    """livo_vio_params from a camera dict (fx, fy, cx, cy, d, width, height) and the extrinsics."""
    p = VioParams()
    _check("livo_vio_params_default", load().livo_vio_params_default(C.byref(p)))
    p.cam.fx, p.cam.fy, p.cam.cx, p.cam.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    p.cam.d[:] = list(cam["d"]) + [0.0] * (5 - len(cam["d"]))
    p.cam.width, p.cam.height = cam["width"], cam["height"]
    p.R_ci[:] = np.asarray(Rci, np.float64).reshape(9).tolist()
    p.P_ci[:] = np.asarray(Pci, np.float64).reshape(3).tolist()
    return p


class MapAddStats(C.Structure):
    _fields_ = [("events", C.c_int64), ("added", C.c_int64), ("deleted", C.c_int64), ("ambiguous", C.c_int64),
                ("deferred", C.c_int64), ("map_points", C.c_int64)]


class ImuSample(C.Structure):
    _fields_ = [("stamp", C.c_double), ("acc", C.c_double * 3), ("gyr", C.c_double * 3)]


class ImuParams(C.Structure):
    _fields_ = [("cov_acc", C.c_double * 3), ("cov_gyr", C.c_double * 3), ("cov_bias_gyr", C.c_double * 3),
                ("cov_bias_acc", C.c_double * 3), ("mean_acc", C.c_double * 3)]


class ImuCarry(C.Structure):
    _fields_ = [("last_imu", ImuSample), ("acc_s_last", C.c_double * 3), ("angvel_last", C.c_double * 3),
                ("last_lidar_end_time", C.c_double)]


class ImuJob(C.Structure):
    _fields_ = [("imu", C.c_void_p), ("n_imu", C.c_int32), ("pcl_beg_time", C.c_double),
                ("pcl_end_time", C.c_double)]


IMU_INIT_COLLECTING, IMU_INIT_RESET, IMU_INIT_DONE = 0, 1, 2
LIDAR_AVIA, LIDAR_VELO16, LIDAR_OUST64, LIDAR_XT32 = 1, 2, 3, 4  # LIVO_LIDAR_* (preprocess.h:14)


class LivoxPoint(C.Structure):
    _fields_ = [("offset_time", C.c_uint32), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float),
                ("reflectivity", C.c_uint8), ("tag", C.c_uint8), ("line", C.c_uint8), ("pad", C.c_uint8)]


LIVOX_POINT_DTYPE = np.dtype([("offset_time", np.uint32), ("x", np.float32), ("y", np.float32), ("z", np.float32),
                              ("reflectivity", np.uint8), ("tag", np.uint8), ("line", np.uint8), ("pad", np.uint8)])


class CloudLayout(C.Structure):
    _fields_ = [("point_step", C.c_int32), ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32),
                ("off_intensity", C.c_int32), ("off_time", C.c_int32)]


class IngestParams(C.Structure):
    _fields_ = [("lidar_type", C.c_int32), ("n_scans", C.c_int32), ("point_filter_num", C.c_int32),
                ("reserved", C.c_int32), ("blind", C.c_double)]


class IngestInfo(C.Structure):
    _fields_ = [("n_in", C.c_int64), ("n_kept", C.c_int64), ("cursor", C.c_int64), ("n_rejected", C.c_int64),
                ("n_decimated", C.c_int64), ("end_curvature", C.c_float)]


def ingest_params(**kw) -> IngestParams:
    """livo_ingest_params_default (AVIA, 16, 2, 0.01) with the given members replaced."""
    p = IngestParams()
    _check("livo_ingest_params_default", load().livo_ingest_params_default(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p
STD_MAX_FRAMES = 20000    # LIVO_STD_MAX_FRAMES
STD_MAX_CANDIDATES = 64   # LIVO_STD_MAX_CANDIDATES


class StdParams(C.Structure):
    _fields_ = [("skip_near_num", C.c_int32), ("candidate_num", C.c_int32), ("rough_dis_threshold", C.c_double),
                ("vertex_diff_threshold", C.c_double), ("icp_threshold", C.c_double), ("normal_threshold", C.c_double),
                ("dis_threshold", C.c_double)]


class StdDesc(C.Structure):
    _fields_ = [("side_length", C.c_double * 3), ("vertex_A", C.c_double * 3), ("vertex_B", C.c_double * 3),
                ("vertex_C", C.c_double * 3), ("center", C.c_double * 3), ("vertex_attached", C.c_double * 3),
                ("frame_id", C.c_uint32), ("pad", C.c_uint32)]


class StdPlane(C.Structure):
    _fields_ = [("xyz", C.c_float * 3), ("normal", C.c_float * 3)]


class StdPair(C.Structure):
    _fields_ = [("src", C.c_int32), ("frame", C.c_int32), ("db_index", C.c_int32)]


class StdResult(C.Structure):
    _fields_ = [("frame", C.c_int32), ("n_candidates", C.c_int32), ("n_pairs", C.c_int32), ("candidate", C.c_int32),
                ("score", C.c_double), ("rot", C.c_double * 9), ("t", C.c_double * 3)]


class StdCandidate(C.Structure):
    _fields_ = [("frame", C.c_int32), ("votes", C.c_int32), ("use_size", C.c_int32), ("max_vote", C.c_int32),
                ("max_vote_index", C.c_int32), ("pad", C.c_int32), ("score", C.c_double), ("rot", C.c_double * 9),
                ("t", C.c_double * 3)]


class StdInfo(C.Structure):
    _fields_ = [("frames", C.c_int64), ("descs", C.c_int64), ("planes", C.c_int64), ("cells", C.c_int64),
                ("max_descs", C.c_int64), ("max_frames", C.c_int64), ("max_planes", C.c_int64),
                ("staged_descs", C.c_int64), ("staged_planes", C.c_int64)]


STD_DESC_DTYPE = np.dtype([("side_length", np.float64, (3,)), ("vertex_A", np.float64, (3,)),
                           ("vertex_B", np.float64, (3,)), ("vertex_C", np.float64, (3,)),
                           ("center", np.float64, (3,)), ("vertex_attached", np.float64, (3,)),
                           ("frame_id", np.uint32), ("pad", np.uint32)])
STD_PLANE_DTYPE = np.dtype([("xyz", np.float32, (3,)), ("normal", np.float32, (3,))])
STD_PAIR_DTYPE = np.dtype([("src", np.int32), ("frame", np.int32), ("db_index", np.int32)])
STD_CANDIDATE_DTYPE = np.dtype([("frame", np.int32), ("votes", np.int32), ("use_size", np.int32),
                                ("max_vote", np.int32), ("max_vote_index", np.int32), ("pad", np.int32),
                                ("score", np.float64), ("rot", np.float64, (9,)), ("t", np.float64, (3,))])


def std_params(**kw) -> StdParams:
    """livo_std_params_default (read_parameters' defaults) with the given members replaced."""
    p = StdParams()
    _check("livo_std_params_default", load().livo_std_params_default(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


STD_GEN_MAX_IMAGE = 80    # LIVO_STD_GEN_MAX_IMAGE
STD_GEN_MAX_NEAR = 64     # LIVO_STD_GEN_MAX_NEAR


class StdGenParams(C.Structure):
    _fields_ = [("voxel_size", C.c_double), ("plane_detection_thre", C.c_double), ("plane_merge_normal_thre", C.c_double),
                ("proj_image_resolution", C.c_double), ("proj_dis_min", C.c_double), ("proj_dis_max", C.c_double),
                ("corner_thre", C.c_double), ("non_max_suppression_radius", C.c_double),
                ("descriptor_min_len", C.c_double), ("descriptor_max_len", C.c_double), ("std_side_resolution", C.c_double),
                ("voxel_init_num", C.c_int32), ("maximum_corner_num", C.c_int32), ("descriptor_near_num", C.c_int32),
                ("pad", C.c_int32)]


class StdGenStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("points", "voxels", "plane_voxels", "jobs", "corners_raw", "corners_suppressed",
                                         "corners", "triangles_tried", "descs")]


class StdCorner(C.Structure):
    _fields_ = [("xyz", C.c_float * 3), ("attached", C.c_float), ("normal", C.c_float * 3), ("pad", C.c_float)]


STD_CORNER_DTYPE = np.dtype([("xyz", np.float32, (3,)), ("attached", np.float32), ("normal", np.float32, (3,)),
                             ("pad", np.float32)])


def std_gen_params(**kw) -> StdGenParams:
    """livo_std_gen_params_default (read_parameters' defaults) with the given members replaced."""
    p = StdGenParams()
    _check("livo_std_gen_params_default", load().livo_std_gen_params_default(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_IMU_PARAM_FIELDS = ("cov_acc", "cov_gyr", "cov_bias_gyr", "cov_bias_acc", "mean_acc")


def imu_params_to_c(p: dict | None) -> ImuParams:
    """None: the constructor's values (livo_imu_params_default); keys left out keep those."""
    q = ImuParams()
    _check("livo_imu_params_default", load().livo_imu_params_default(C.byref(q)))
    for k, v in (p or {}).items():
        getattr(q, k)[:] = np.asarray(v, np.float64).reshape(3).tolist()
    return q


def imu_params_from_c(q: ImuParams) -> dict:
    return {k: np.array(getattr(q, k)[:]) for k in _IMU_PARAM_FIELDS}


def imu_params_inited(p: dict | None = None) -> dict:
    q = imu_params_to_c(p)
    _check("livo_imu_params_inited", load().livo_imu_params_inited(C.byref(q)))
    return imu_params_from_c(q)


def imu_carry_to_c(c: dict) -> ImuCarry:
    """carry: last_imu (7: stamp, acc, gyr), acc_s_last, angvel_last, last_lidar_end_time."""
    q = ImuCarry()
    li = np.asarray(c["last_imu"], np.float64).reshape(7)
    q.last_imu.stamp = li[0]
    q.last_imu.acc[:] = li[1:4].tolist()
    q.last_imu.gyr[:] = li[4:7].tolist()
    q.acc_s_last[:] = np.asarray(c["acc_s_last"], np.float64).reshape(3).tolist()
    q.angvel_last[:] = np.asarray(c["angvel_last"], np.float64).reshape(3).tolist()
    q.last_lidar_end_time = float(c["last_lidar_end_time"])
    return q


def imu_carry_from_c(q: ImuCarry) -> dict:
    return {"last_imu": np.array([q.last_imu.stamp] + q.last_imu.acc[:] + q.last_imu.gyr[:]),
            "acc_s_last": np.array(q.acc_s_last[:]), "angvel_last": np.array(q.angvel_last[:]),
            "last_lidar_end_time": q.last_lidar_end_time}


def new_imu_carry() -> dict:
    """The constructor's carry: an empty last_imu_, zero rates, last_lidar_end_time_ 0."""
    return {"last_imu": np.zeros(7), "acc_s_last": np.zeros(3), "angvel_last": np.zeros(3),
            "last_lidar_end_time": 0.0}


def imu_init(imu: np.ndarray, params: dict | None, init_iter_num: int, mean_gyr, state: dict):
    """ImuProcess::IMU_init over meas.imu (n, 7: stamp, acc, gyr).  Host code: needs no GPU.
    -> (status, params, init_iter_num, mean_gyr, state)."""
    imu = np.ascontiguousarray(imu, np.float64).reshape(-1, 7)
    q = imu_params_to_c(params)
    it = C.c_int32(init_iter_num)
    mg = np.ascontiguousarray(np.array(mean_gyr, np.float64).reshape(3))
    s = state_to_c(state)
    status = C.c_int32(-1)
    _check("livo_imu_init", load().livo_imu_init(None, _ptr(imu), imu.shape[0], C.byref(q), C.byref(it), _ptr(mg),
                                                 C.byref(s), C.byref(status)))
    return status.value, imu_params_from_c(q), it.value, mg, state_from_c(s)


SIGNATURES = {
    "livo_abi_version": (C.c_int, []),
    "livo_error_string": (C.c_char_p, [C.c_int]),
    "livo_params_default": (C.c_int, [C.POINTER(Params)]),
    "livo_ctx_create": (C.c_int, [C.c_int, C.POINTER(Params), C.POINTER(_P)]),
    "livo_ctx_destroy": (C.c_int, [_P]),
    "livo_ctx_set_params": (C.c_int, [_P, C.POINTER(Params)]),
    "livo_ctx_set_profiling": (C.c_int, [_P, C.c_int]),
    "livo_last_timings": (C.c_int, [_P, C.POINTER(Timings)]),
    "livo_map_build": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "livo_map_get_info": (C.c_int, [_P, C.POINTER(MapInfo)]),
    "livo_knn": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    "livo_scan_upload": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "livo_scan_upload_async": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "livo_debug_map_rebuilds": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "livo_scan_upload_batch_async": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, _P]),
    "livo_host_register": (C.c_int, [_P, _P, C.c_size_t]),
    "livo_host_unregister": (C.c_int, [_P, _P]),
    "livo_scan_release": (C.c_int, [_P, C.c_int32]),
    "livo_scan_neighbors": (C.c_int, [_P, C.c_int32, _P, _P]),
    "livo_h_share": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.c_int, _P, _P, C.POINTER(C.c_int64),
                               C.POINTER(PointOut)]),
    "livo_iekf_update": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.POINTER(State), C.POINTER(IterStats)]),
    "livo_iekf_update_batch": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "livo_iekf_update_batch_submit": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "livo_iekf_update_batch_wait": (C.c_int, [_P, C.c_int32, _P, _P]),
    "livo_ikfom_update": (C.c_int, [_P, C.c_int32, C.POINTER(IkfomState), C.POINTER(IkfomStats)]),
    "livo_ikfom_update_batch": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "livo_ikfom_update_batch_submit": (C.c_int, [_P, C.c_int32, _P, _P, C.POINTER(C.c_int32)]),
    "livo_ikfom_update_batch_wait": (C.c_int, [_P, C.c_int32, _P, _P]),
    "livo_ctx_set_backend": (C.c_int, [_P, C.c_int]),
    "livo_ivox_params_default": (C.c_int, [C.POINTER(IvoxParams)]),
    "livo_ivox_init": (C.c_int, [_P, C.POINTER(IvoxParams)]),
    "livo_ivox_add_points": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "livo_ivox_knn": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_double, _P, _P, _P]),
    "livo_ivox_get_info": (C.c_int, [_P, C.POINTER(IvoxInfo)]),
    "livo_ivox_dump": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_map_incremental": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.c_double, C.c_int, _P, _P]),
    "livo_scan_inherit_neighbors": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "livo_scan_preprocess": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, _P, _P, C.c_float, C.POINTER(C.c_int32),
                                       _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_vio_params_default": (C.c_int, [C.POINTER(VioParams)]),
    "livo_vio_update": (C.c_int, [_P, C.POINTER(VioParams), _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64,
                                  C.POINTER(State), C.POINTER(State), _P, C.POINTER(VioStats)]),
    "livo_map_add_points": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_float, C.c_int, C.POINTER(MapAddStats)]),
    "livo_map_delete_boxes": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_map_dump": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_map_last_add_stats": (C.c_int, [_P, C.POINTER(MapAddStats)]),
    "livo_frame_to_world": (C.c_int, [_P, C.c_int32, C.POINTER(State), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_cloud_colorize": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.POINTER(VioParams), _P, C.c_int32, C.c_int32,
                                      _P, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(RgbStats)]),
    "livo_vio_select": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.POINTER(VioParams), C.c_int32, _P, C.c_int32,
                                  C.c_int32, _P, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(VisStats)]),
    "livo_vmap_reset": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int32]),
    "livo_vmap_add_frame": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.POINTER(VioParams), _P, C.c_int32,
                                      C.c_int32]),
    "livo_vmap_add": (C.c_int, [_P, C.c_int32, C.c_int64, _P, _P, _P, _P, _P]),
    "livo_vmap_info": (C.c_int, [_P, C.POINTER(VmapCounts)]),
    "livo_vmap_dump": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "livo_vio_match": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.POINTER(VioParams), C.c_int32, C.c_int32,
                                 C.c_double, C.c_double, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64,
                                 C.POINTER(C.c_int64), C.POINTER(VmatchStats)]),
    "livo_vio_observe": (C.c_int, [_P, C.c_int32, C.c_int64, _P, _P, _P, C.POINTER(VobsStats)]),
    "livo_vmap_release_frames": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_vio_detect": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(State), C.POINTER(State), C.POINTER(VioParams),
                                  C.POINTER(VdetectParams), _P, C.c_int32, C.c_int32, C.POINTER(VdetectStats)]),
    "livo_cloud_publish": (C.c_int, [_P, C.c_int32, C.POINTER(State), C.c_float, C.POINTER(CloudInfo)]),
    "livo_cloud_info_get": (C.c_int, [_P, C.POINTER(CloudInfo)]),
    "livo_imu_params_default": (C.c_int, [C.POINTER(ImuParams)]),
    "livo_imu_params_inited": (C.c_int, [C.POINTER(ImuParams)]),
    "livo_imu_init": (C.c_int, [_P, _P, C.c_int32, C.POINTER(ImuParams), C.POINTER(C.c_int32), _P,
                                C.POINTER(State), C.POINTER(C.c_int32)]),
    "livo_imu_propagate_batch": (C.c_int, [_P, C.c_int32, _P, C.POINTER(ImuParams), _P, _P, _P, C.c_int32, _P]),
    "livo_imu_propagate": (C.c_int, [_P, C.POINTER(ImuJob), C.POINTER(ImuParams), C.POINTER(ImuCarry),
                                     C.POINTER(State), _P, C.c_int32, C.POINTER(C.c_int32)]),
    "livo_scan_preprocess_imu": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.POINTER(C.c_int32), _P, _P, C.c_int64,
                                           C.POINTER(C.c_int64)]),
    "livo_ingest_params_default": (C.c_int, [C.POINTER(IngestParams)]),
    "livo_frame_ingest_livox": (C.c_int, [_P, C.POINTER(IngestParams), _P, C.c_int64, C.POINTER(IngestInfo)]),
    "livo_frame_ingest_cloud": (C.c_int, [_P, C.POINTER(IngestParams), _P, C.c_int64, C.POINTER(CloudLayout),
                                          C.POINTER(IngestInfo)]),
    "livo_frame_info": (C.c_int, [_P, C.POINTER(IngestInfo)]),
    "livo_frame_dump": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_frame_take": (C.c_int, [_P, C.c_double, C.c_int, C.c_float, C.POINTER(C.c_int32), _P, _P, C.c_int64,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "livo_lio_frame": (C.c_int, [_P, C.POINTER(ImuJob), C.POINTER(ImuParams), C.POINTER(ImuCarry), C.c_double,
                                 C.POINTER(LioParams), C.POINTER(State), C.POINTER(State), C.POINTER(LioStats)]),
    "livo_std_params_default": (C.c_int, [C.POINTER(StdParams)]),
    "livo_std_reset": (C.c_int, [_P, C.POINTER(StdParams), C.c_int64, C.c_int64, C.c_int64]),
    "livo_std_stage": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64]),
    "livo_std_search": (C.c_int, [_P, C.POINTER(StdResult), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_std_commit": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "livo_std_candidates": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_std_matches": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_std_info_get": (C.c_int, [_P, C.POINTER(StdInfo)]),
    "livo_std_gen_params_default": (C.c_int, [C.POINTER(StdGenParams)]),
    "livo_std_key_add": (C.c_int, [_P, C.c_int32]),
    "livo_std_key_add_host": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "livo_std_key_clear": (C.c_int, [_P]),
    "livo_std_key_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "livo_std_generate": (C.c_int, [_P, C.POINTER(StdGenParams), C.POINTER(StdGenStats)]),
    "livo_std_staged": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64), _P, C.c_int64, C.POINTER(C.c_int64), _P,
                                  C.c_int64, C.POINTER(C.c_int64)]),
    "livo_std_gen_debug": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "livo_std_dump": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64), C.c_int32, _P, C.c_int64,
                                C.POINTER(C.c_int64)]),
    "livo_sync": (C.c_int, [_P]),
}

_lib = None


def load(path: str = LIB_PATH):
    """Load liblivo_hip.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise ImportError(f"HIP library not built: {path} (run __graft_entry__.build())")
        L = C.CDLL(path)
        # an A/B variant of an older build (LIVO_LIB) may lack entry points added since
        old_ok = os.path.abspath(path) != os.path.abspath(os.path.join(PKG_ROOT, "lib", "liblivo_hip.so"))
        for name, (res, args) in SIGNATURES.items():
            if old_ok and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def page_aligned_copy(a: np.ndarray) -> np.ndarray:
    """A C-contiguous copy of `a` whose data starts on a 4 KiB page (for
    livo_host_register: the copy engine then reads whole pages of it)."""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + 4096, np.uint8)
    off = (-raw.ctypes.data) % 4096
    out = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def _check(fn, rc):
    if rc != LIVO_OK:
        raise LivoError(fn, rc)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_params(**kw) -> Params:
    p = Params()
    _check("livo_params_default", load().livo_params_default(C.byref(p)))
    for k, v in kw.items():
        if k in ("R_LI",):
            p.R_LI[:] = np.asarray(v, np.float64).reshape(9).tolist()
        elif k == "t_LI":
            p.t_LI[:] = np.asarray(v, np.float64).reshape(3).tolist()
        else:
            setattr(p, k, v)
    return p


def state_to_c(st: dict) -> State:
    s = State()
    s.rot[:] = np.asarray(st["rot"], np.float64).reshape(9).tolist()
    for k in ("pos", "vel", "bias_g", "bias_a", "gravity"):
        getattr(s, k)[:] = np.asarray(st[k], np.float64).reshape(3).tolist()
    s.cov[:] = np.asarray(st["cov"], np.float64).reshape(324).tolist()
    return s


def state_from_c(s: State) -> dict:
    return {"rot": np.array(s.rot[:]).reshape(3, 3), "pos": np.array(s.pos[:]), "vel": np.array(s.vel[:]),
            "bias_g": np.array(s.bias_g[:]), "bias_a": np.array(s.bias_a[:]),
            "gravity": np.array(s.gravity[:]), "cov": np.array(s.cov[:]).reshape(18, 18)}


def stats_from_c(st: IterStats) -> dict:
    ne = min(st.iterations, MAX_EVALS)
    return {"iterations": st.iterations, "knn_passes": st.knn_passes, "converged": st.converged,
            "rematch_num": st.rematch_num, "effct_feat_num": [st.effct_feat_num[i] for i in range(ne)],
            "solution": np.array([list(st.solution[i]) for i in range(ne)]).reshape(ne, 18),
            "res_mean": [st.res_mean[i] for i in range(ne)]}


class Context:
    """One livo_ctx: a HIP stream, the device map and resident scans on one GPU."""

    def __init__(self, device: int = 0, params: Params | None = None, **kw):
        L = load()
        self._L = L
        self.params = params if params is not None else default_params(**kw)
        h = C.c_void_p()
        _check("livo_ctx_create", L.livo_ctx_create(device, C.byref(self.params), C.byref(h)))
        self.h = h
        self.scans = {}

    def close(self):
        if getattr(self, "h", None):
            self._L.livo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_params(self, **kw):
        for k, v in kw.items():
            if k == "R_LI":
                self.params.R_LI[:] = np.asarray(v, np.float64).reshape(9).tolist()
            elif k == "t_LI":
                self.params.t_LI[:] = np.asarray(v, np.float64).reshape(3).tolist()
            else:
                setattr(self.params, k, v)
        _check("livo_ctx_set_params", self._L.livo_ctx_set_params(self.h, C.byref(self.params)))

    # ------------------------------------------------------------ map ----
    def map_build(self, xyz: np.ndarray):
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        _check("livo_map_build", self._L.livo_map_build(self.h, _ptr(xyz), xyz.shape[0], xyz.shape[1] * 4))

    def map_rebuilds(self) -> tuple:
        """(grid rebuilds by sorting every id, by merging the added ids, Add_Points batches
        redone with 64-bit box keys, merged rebuilds run inside Add_Points' pass) of the incremental map."""
        out = (C.c_int64 * 4)()
        _check("livo_debug_map_rebuilds", self._L.livo_debug_map_rebuilds(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def map_info(self) -> dict:
        mi = MapInfo()
        _check("livo_map_get_info", self._L.livo_map_get_info(self.h, C.byref(mi)))
        return {"num_points": mi.num_points, "depth": mi.depth, "num_slots": mi.num_slots,
                "device_bytes": mi.device_bytes, "ball_chunks": mi.ball_chunks, "ball_entries": mi.ball_entries}

    def knn(self, q: np.ndarray, k: int = 5):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        n = q.shape[0]
        idx = np.empty((n, k), np.int32)
        d = np.empty((n, k), np.float32)
        _check("livo_knn", self._L.livo_knn(self.h, _ptr(q), n, k, _ptr(idx), _ptr(d)))
        return idx, d

    # ---------------------------------------------------------- scans ----
    def scan_upload(self, xyz: np.ndarray) -> int:
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        sid = C.c_int32()
        _check("livo_scan_upload", self._L.livo_scan_upload(self.h, _ptr(xyz), xyz.shape[0], xyz.shape[1] * 4,
                                                            C.byref(sid)))
        self.scans[sid.value] = xyz.shape[0]
        return sid.value

    def scan_upload_async(self, xyz: np.ndarray) -> int:
        """livo_scan_upload_async: returns once the points are staged; the copy and
        Morton sort run on the context's upload stream (batches wait for them)."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        sid = C.c_int32()
        _check("livo_scan_upload_async",
               self._L.livo_scan_upload_async(self.h, _ptr(xyz), xyz.shape[0], xyz.shape[1] * 4, C.byref(sid)))
        self.scans[sid.value] = xyz.shape[0]
        return sid.value

    def scan_upload_batch_async(self, scans) -> list:
        """livo_scan_upload_batch_async: a list of (N_b, w) float32 arrays (one width w
        >= 3 for all) in one pass; returns their scan ids.  Arrays in page-locked
        memory (host_register) with w = 3 are read by the copy engine directly and
        must stay unchanged until a batch using the scans returns."""
        arrs = [np.ascontiguousarray(x, np.float32) for x in scans]
        n = len(arrs)
        w = arrs[0].shape[1] if n else 3
        assert all(a.ndim == 2 and a.shape[1] == w for a in arrs) and w >= 3
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        ns = (C.c_int64 * max(n, 1))(*[a.shape[0] for a in arrs])
        ids = (C.c_int32 * max(n, 1))()
        _check("livo_scan_upload_batch_async",
               self._L.livo_scan_upload_batch_async(self.h, ptrs, ns, n, w * 4, ids))
        for b in range(n):
            self.scans[ids[b]] = arrs[b].shape[0]
        self._keep = arrs  # (the arrays the device may still read from)
        return [ids[b] for b in range(n)]

    def host_register(self, arr: np.ndarray):
        """Page-lock a C-contiguous array's memory (livo_host_register)."""
        assert arr.flags["C_CONTIGUOUS"] and arr.nbytes > 0
        _check("livo_host_register", self._L.livo_host_register(self.h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr: np.ndarray):
        _check("livo_host_unregister", self._L.livo_host_unregister(self.h, arr.ctypes.data))

    def scan_release(self, sid: int):
        _check("livo_scan_release", self._L.livo_scan_release(self.h, sid))
        self.scans.pop(sid, None)

    def scan_neighbors(self, sid: int):
        """(idx (N, 5) int32, sqdist (N, 5) float32) of the scan's last search."""
        n = self.scans[sid]
        idx = np.empty((n, 5), np.int32)
        d = np.empty((n, 5), np.float32)
        _check("livo_scan_neighbors", self._L.livo_scan_neighbors(self.h, sid, _ptr(idx), _ptr(d)))
        return idx, d

    # -------------------------------------------------------- hot path ----
    def h_share(self, sid: int, state: dict, search_en: bool = True, outputs: bool = True):
        n = self.scans[sid]
        HTH = np.zeros(81)
        HTL = np.zeros(9)
        eff = C.c_int64()
        po = None
        res = {}
        if outputs:
            res = {"normvec": np.zeros((n, 4), np.float32), "sel": np.zeros(n, np.uint8),
                   "nn_idx": np.zeros((n, 5), np.int32), "nn_d": np.zeros((n, 5), np.float32),
                   "world": np.zeros((n, 3), np.float32), "visits": np.zeros(1, np.int64),
                   "ori": np.zeros((n, 3), np.float32), "corr_normvec": np.zeros((n, 4), np.float32),
                   "n_ori": np.zeros(1, np.int64)}
            po = PointOut(_ptr(res["normvec"]), _ptr(res["sel"]), _ptr(res["nn_idx"]), _ptr(res["nn_d"]),
                          _ptr(res["world"]), _ptr(res["visits"]), _ptr(res["ori"]), _ptr(res["corr_normvec"]),
                          _ptr(res["n_ori"]))
        st = state_to_c(state)
        _check("livo_h_share", self._L.livo_h_share(self.h, sid, C.byref(st), int(bool(search_en)), _ptr(HTH),
                                                    _ptr(HTL), C.byref(eff), C.byref(po) if po else None))
        res.update({"HTH": HTH.reshape(9, 9), "HTL": HTL, "effct": eff.value})
        if outputs:
            res["visits"] = int(res["visits"][0])
            k = int(res.pop("n_ori")[0])
            res["ori"] = res["ori"][:k]                    # laserCloudOri
            res["corr_normvec"] = res["corr_normvec"][:k]  # corr_normvect
        return res

    def frame_to_world(self, state: dict, sid: int = -1) -> np.ndarray:
        """RGBpointBodyToWorld of the last preprocessed full-res frame (sid < 0) or a resident
        scan: (n, 5) float32 x, y, z (world), intensity, curvature (livo_frame_to_world)."""
        st = state_to_c(state)
        n = C.c_int64()
        _check("livo_frame_to_world", self._L.livo_frame_to_world(self.h, sid, C.byref(st), None, 0, C.byref(n)))
        out = np.zeros((n.value, 5), np.float32)
        _check("livo_frame_to_world", self._L.livo_frame_to_world(self.h, sid, C.byref(st), _ptr(out), n.value,
                                                                  C.byref(n)))
        return out

    def cloud_publish(self, state: dict, sid: int = -1, match_leaf: float = 0.2) -> dict:
        """pcl_wait_pub at the end of a LiDAR frame (livo_cloud_publish): frame_to_world(state, sid) kept on
        the device as CLOUD_WORLD for the camera frames that follow, and with match_leaf > 0 its VoxelGrid
        (pg_down) as CLOUD_WORLD_DOWN.  Returns cloud_info()."""
        st = state_to_c(state)
        ci = CloudInfo()
        _check("livo_cloud_publish", self._L.livo_cloud_publish(self.h, sid, C.byref(st), match_leaf, C.byref(ci)))
        return {f: int(getattr(ci, f)) for f, _ in CloudInfo._fields_ if f != "pad_"}

    def cloud_info(self) -> dict:
        """The published cloud's n, n_down (-1: no pg_down), down_filtered and device_bytes."""
        ci = CloudInfo()
        _check("livo_cloud_info_get", self._L.livo_cloud_info_get(self.h, C.byref(ci)))
        return {f: int(getattr(ci, f)) for f, _ in CloudInfo._fields_ if f != "pad_"}

    def colorize(self, state: dict, image_bgr, vio_params: VioParams, scan_id: int = -1):
        """publish_frame_world_rgb's coloured cloud (livo_cloud_colorize): the cloud of frame_to_world(state,
        scan_id) in the camera of vio_params (cam, R_ci, P_ci) at `state`, the points in the image kept in
        order with their bilinear colour.  image_bgr: (height, width, 3) uint8, B G R; None reuses the image
        of the previous call.  Returns (points: RGB_POINT_DTYPE array, src_index: int32, stats: dict)."""
        st = state_to_c(state)
        img = None
        if image_bgr is not None:
            img = np.ascontiguousarray(image_bgr, np.uint8)
            if img.ndim != 3 or img.shape[2] != 3:
                raise ValueError("image_bgr must be (height, width, 3)")
            w, h = img.shape[1], img.shape[0]
        else:
            w, h = vio_params.cam.width, vio_params.cam.height
        n = C.c_int64()
        # the size of the source cloud bounds the result: one call, one upload
        _check("livo_frame_to_world", self._L.livo_frame_to_world(self.h, scan_id, C.byref(st), None, 0, C.byref(n)))
        cap = n.value
        pts = np.zeros(cap, RGB_POINT_DTYPE)
        idx = np.zeros(cap, np.int32)
        rs = RgbStats()
        _check("livo_cloud_colorize", self._L.livo_cloud_colorize(
            self.h, scan_id, C.byref(st), C.byref(vio_params), _ptr(img), w, h, _ptr(pts), _ptr(idx), cap,
            C.byref(n), C.byref(rs)))
        stats = {f: int(getattr(rs, f)) for f, _ in RgbStats._fields_}
        return pts[:n.value].copy(), idx[:n.value].copy(), stats

    def iekf_update(self, sid: int, state: dict, prior: dict | None = None):
        st = state_to_c(state)
        pr = state_to_c(prior) if prior is not None else None
        stats = IterStats()
        _check("livo_iekf_update", self._L.livo_iekf_update(self.h, sid, C.byref(st),
                                                            C.byref(pr) if pr is not None else None,
                                                            C.byref(stats)))
        return state_from_c(st), stats_from_c(stats)

    def iekf_update_batch(self, sids, states, priors=None, raw: bool = False):
        n = len(sids)
        if raw:
            # hot loop (bench): states / priors are ctypes State arrays (at least
            # n entries each: the library reads and writes n); the id and stats
            # buffers are the context's own, reused while the ids repeat, so the
            # returned stats array is overwritten by the next raw call (copy it
            # to keep it)
            nb = n * C.sizeof(State)
            if C.sizeof(states) < nb or (priors is not None and C.sizeof(priors) < nb):
                raise ValueError(f"iekf_update_batch(raw): states/priors hold fewer than {n} State entries")
            key = tuple(sids)
            cache = getattr(self, "_raw_batch", None)
            if cache is None or cache[0] != key:
                ids = (C.c_int32 * n)(*sids)
                stats = (IterStats * n)()
                cache = self._raw_batch = (key, ids, stats, C.addressof(ids), C.addressof(stats))
            _, ids, stats, p_ids, p_stats = cache
            _check("livo_iekf_update_batch",
                   self._L.livo_iekf_update_batch(self.h, n, p_ids, C.addressof(states),
                                                  C.addressof(priors) if priors is not None else None, p_stats))
            return states, stats
        ids = (C.c_int32 * n)(*sids)
        sts = (State * n)(*[state_to_c(s) for s in states])
        prs = (State * n)(*[state_to_c(s) for s in priors]) if priors is not None else None
        stats = (IterStats * n)()
        _check("livo_iekf_update_batch",
               self._L.livo_iekf_update_batch(self.h, n, C.cast(ids, C.c_void_p), C.cast(sts, C.c_void_p),
                                              C.cast(prs, C.c_void_p) if prs is not None else None,
                                              C.cast(stats, C.c_void_p)))
        return [state_from_c(s) for s in sts], [stats_from_c(s) for s in stats]

    def iekf_update_batch_submit(self, sids, states, priors=None) -> int:
        """Enqueue a batched update and return its ticket (livo_iekf_update_batch_submit).
        states / priors: dicts, or ctypes State arrays of at least len(sids) entries
        (copied at the call); at most MAX_INFLIGHT batches are outstanding."""
        n = len(sids)
        ids = (C.c_int32 * n)(*sids)
        if not isinstance(states, C.Array):
            states = (State * n)(*[state_to_c(s) for s in states])
        if priors is not None and not isinstance(priors, C.Array):
            priors = (State * n)(*[state_to_c(s) for s in priors])
        nb = n * C.sizeof(State)
        if C.sizeof(states) < nb or (priors is not None and C.sizeof(priors) < nb):
            raise ValueError(f"iekf_update_batch_submit: states/priors hold fewer than {n} State entries")
        ticket = C.c_int32(-1)
        _check("livo_iekf_update_batch_submit",
               self._L.livo_iekf_update_batch_submit(self.h, n, C.addressof(ids), C.addressof(states),
                                                     C.addressof(priors) if priors is not None else None,
                                                     C.byref(ticket)))
        return ticket.value

    def iekf_update_batch_wait(self, ticket: int, n: int, out=None, stats=None):
        """Collect a submitted batch of n scans (livo_iekf_update_batch_wait).  With out
        (a ctypes State array of >= n entries) and stats (IterStats array or None) the
        raw arrays are filled and returned; else lists of dicts."""
        raw = out is not None
        if out is None:
            out = (State * max(n, 1))()
            stats = (IterStats * max(n, 1))()
        if C.sizeof(out) < n * C.sizeof(State) or (stats is not None and C.sizeof(stats) < n * C.sizeof(IterStats)):
            raise ValueError(f"iekf_update_batch_wait: output arrays hold fewer than {n} entries")
        _check("livo_iekf_update_batch_wait",
               self._L.livo_iekf_update_batch_wait(self.h, ticket, C.addressof(out),
                                                   C.addressof(stats) if stats is not None else None))
        if raw:
            return out, stats
        return [state_from_c(out[b]) for b in range(n)], [stats_from_c(stats[b]) for b in range(n)]

    # ------------------------------------------------------------ IKFoM ----
    def ikfom_update(self, sid: int, state: dict):
        """IKFoM iterated update (esekfom.hpp:1619-1928) of one resident scan."""
        st = ikfom_to_c(state)
        stats = IkfomStats()
        _check("livo_ikfom_update", self._L.livo_ikfom_update(self.h, sid, C.byref(st), C.byref(stats)))
        return ikfom_from_c(st), ikfom_stats_from_c(stats)

    def ikfom_update_batch(self, sids, states, raw: bool = False):
        n = len(sids)
        ids = (C.c_int32 * n)(*sids)
        sts = states if raw else (IkfomState * n)(*[ikfom_to_c(s) for s in states])
        stats = (IkfomStats * n)()
        _check("livo_ikfom_update_batch",
               self._L.livo_ikfom_update_batch(self.h, n, C.cast(ids, C.c_void_p), C.cast(sts, C.c_void_p),
                                               C.cast(stats, C.c_void_p)))
        if raw:
            return sts, stats
        return [ikfom_from_c(s) for s in sts], [ikfom_stats_from_c(s) for s in stats]

    def ikfom_update_batch_submit(self, sids, states, raw: bool = False) -> int:
        """livo_ikfom_update_batch_submit: enqueue, return the ticket."""
        n = len(sids)
        ids = (C.c_int32 * max(n, 1))(*sids)
        sts = states if raw else (IkfomState * max(n, 1))(*[ikfom_to_c(s) for s in states])
        t = C.c_int32()
        _check("livo_ikfom_update_batch_submit",
               self._L.livo_ikfom_update_batch_submit(self.h, n, C.cast(ids, C.c_void_p), C.cast(sts, C.c_void_p),
                                                      C.byref(t)))
        return t.value

    def ikfom_update_batch_wait(self, ticket: int, n: int, out=None, stats=None):
        """livo_ikfom_update_batch_wait; with out / stats (ctypes arrays) the raw arrays."""
        raw = out is not None
        if out is None:
            out = (IkfomState * max(n, 1))()
            stats = (IkfomStats * max(n, 1))()
        _check("livo_ikfom_update_batch_wait",
               self._L.livo_ikfom_update_batch_wait(self.h, ticket, C.cast(out, C.c_void_p),
                                                    C.cast(stats, C.c_void_p) if stats is not None else None))
        if raw:
            return out, stats
        return [ikfom_from_c(out[b]) for b in range(n)], [ikfom_stats_from_c(stats[b]) for b in range(n)]

    # ----------------------------------------------------------- iVox ----
    def set_backend(self, backend: int):
        _check("livo_ctx_set_backend", self._L.livo_ctx_set_backend(self.h, backend))
        self.backend = backend

    # ------------------------------------------- ikd-Tree incremental map ----
    def map_add_points(self, xyz: np.ndarray, downsample_size: float = 0.5, downsample: bool = True) -> dict:
        """KD_TREE::Add_Points (ikd_Tree.cpp:382-457) on the device map."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        st = MapAddStats()
        _check("livo_map_add_points", self._L.livo_map_add_points(self.h, _ptr(xyz), xyz.shape[0], xyz.shape[1] * 4,
                                                                  downsample_size, int(bool(downsample)),
                                                                  C.byref(st)))
        return {k: getattr(st, k) for k, _ in MapAddStats._fields_}

    def map_delete_boxes(self, boxes) -> int:
        """KD_TREE::Delete_Point_Boxes (ikd_Tree.cpp:501-521); boxes (n, 6) = vertex_min, vertex_max."""
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        n = C.c_int64()
        _check("livo_map_delete_boxes", self._L.livo_map_delete_boxes(self.h, _ptr(b), b.shape[0], C.byref(n)))
        return n.value

    def map_dump(self):
        """(xyz (n, 3), ids (n,)) of the map's points in id order."""
        n = C.c_int64()
        _check("livo_map_dump", self._L.livo_map_dump(self.h, None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), np.float32)
        ids = np.zeros(n.value, np.int32)
        _check("livo_map_dump", self._L.livo_map_dump(self.h, _ptr(xyz), _ptr(ids), n.value, C.byref(n)))
        return xyz, ids

    def map_last_add_stats(self) -> dict:
        st = MapAddStats()
        _check("livo_map_last_add_stats", self._L.livo_map_last_add_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MapAddStats._fields_}

    def ivox_init(self, resolution: float = 0.2, nearby_type: int = 18, capacity: int = 1_000_000):
        p = IvoxParams(resolution, nearby_type, capacity)
        _check("livo_ivox_init", self._L.livo_ivox_init(self.h, C.byref(p)))

    def ivox_add_points(self, xyz: np.ndarray):
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 2 and xyz.shape[1] >= 3
        _check("livo_ivox_add_points", self._L.livo_ivox_add_points(self.h, _ptr(xyz), xyz.shape[0],
                                                                    xyz.shape[1] * 4))

    def ivox_knn(self, q: np.ndarray, max_num: int = 5, max_range: float = 5.0):
        """GetClosestPoint: idx, sqdist (n, max_num) in the reference's order, cnt (-1: nothing found)."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        n = q.shape[0]
        idx = np.empty((n, max_num), np.int32)
        d = np.empty((n, max_num), np.float32)
        cnt = np.empty(n, np.int32)
        _check("livo_ivox_knn", self._L.livo_ivox_knn(self.h, _ptr(q), n, max_num, max_range, _ptr(idx), _ptr(d),
                                                      _ptr(cnt)))
        return idx, d, cnt

    def ivox_info(self) -> dict:
        i = IvoxInfo()
        _check("livo_ivox_get_info", self._L.livo_ivox_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in IvoxInfo._fields_}

    def ivox_dump(self):
        """All points (xyz, ids, grid keys), grid by grid, insertion order inside a grid."""
        n = self.ivox_info()["num_points"]
        xyz = np.zeros((n, 3), np.float32)
        ids = np.zeros(n, np.int32)
        keys = np.zeros((n, 3), np.int32)
        got = C.c_int64()
        _check("livo_ivox_dump", self._L.livo_ivox_dump(self.h, _ptr(xyz), _ptr(ids), _ptr(keys), n, C.byref(got)))
        return xyz, ids, keys

    def map_incremental(self, sid: int, state: dict, filter_size_map: float = 0.5, ekf_inited: bool = True):
        """Returns (cat per point: 0 skipped / 1 added / 2 added without downsampling, counts dict).
        With the ikd-Tree backend: Add_Points of every point (cat 1), counts = the add statistics."""
        n = self.scans[sid]
        cat = np.zeros(n, np.uint8)
        counts = np.zeros(2, np.int64)
        s = state_to_c(state)
        _check("livo_map_incremental", self._L.livo_map_incremental(self.h, sid, C.byref(s), filter_size_map,
                                                                    int(bool(ekf_inited)), _ptr(cat),
                                                                    _ptr(counts)))
        if getattr(self, "backend", BACKEND_IKDTREE) == BACKEND_IKDTREE:
            return cat, self.map_last_add_stats()
        return cat, {"added": int(counts[0]), "no_downsample": int(counts[1])}

    def scan_preprocess(self, raw: np.ndarray, poses=None, rot_end=None, pos_end=None, leaf_size: float = 0.5):
        """Raw frame (n, 5: x, y, z, intensity, curvature ms) -> resident scan id, with the de-skewed
        points (n, 5) and the downsampled cloud (k, 5) (livo_scan_preprocess)."""
        raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 5)
        n = raw.shape[0]
        und = np.zeros_like(raw)
        down = np.zeros_like(raw)
        nd = C.c_int64()
        sid = C.c_int32()
        if poses is not None:
            poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 22)
            rot_end = np.ascontiguousarray(rot_end, np.float64).reshape(9)
            pos_end = np.ascontiguousarray(pos_end, np.float64).reshape(3)
        npo = 0 if poses is None else poses.shape[0]
        _check("livo_scan_preprocess", self._L.livo_scan_preprocess(
            self.h, _ptr(raw), n, _ptr(poses), npo, _ptr(rot_end), _ptr(pos_end), leaf_size, C.byref(sid),
            _ptr(und), _ptr(down), n, C.byref(nd)))
        self.scans[sid.value] = int(nd.value)
        return sid.value, und, down[:nd.value].copy()

    def imu_propagate(self, imu: np.ndarray, pcl_beg_time: float, pcl_end_time: float, params: dict | None,
                      carry: dict, state: dict, want_poses: bool = True):
        """UndistortPcl's forward propagation of one frame (livo_imu_propagate): imu (n, 7: stamp, acc, gyr)
        is meas.imu.  -> (state, carry, poses (rows, 22) or None); the table and the end pose stay
        resident for scan_preprocess_imu."""
        imu = np.ascontiguousarray(imu, np.float64).reshape(-1, 7)
        job = ImuJob(_ptr(imu).value if imu.shape[0] else None, imu.shape[0], pcl_beg_time, pcl_end_time)
        q, cy, s = imu_params_to_c(params), imu_carry_to_c(carry), state_to_c(state)
        cap = imu.shape[0] + 1
        poses = np.zeros((cap, 22)) if want_poses else None
        npo = C.c_int32()
        _check("livo_imu_propagate", self._L.livo_imu_propagate(self.h, C.byref(job), C.byref(q), C.byref(cy),
                                                                C.byref(s), _ptr(poses), cap, C.byref(npo)))
        return state_from_c(s), imu_carry_from_c(cy), (poses[:npo.value].copy() if want_poses else None)

    def imu_propagate_batch(self, jobs: list, params: dict | None, carries: list, states: list,
                            want_poses: bool = True, pose_cap: int | None = None):
        """n independent propagations in one launch (livo_imu_propagate_batch).  jobs: (imu (n_j, 7),
        pcl_beg_time, pcl_end_time) each.  -> (states, carries, list of pose tables or None)."""
        n = len(jobs)
        imus = [np.ascontiguousarray(j[0], np.float64).reshape(-1, 7) for j in jobs]
        cj = (ImuJob * max(n, 1))()
        for k in range(n):
            cj[k] = ImuJob(_ptr(imus[k]).value if imus[k].shape[0] else None, imus[k].shape[0], jobs[k][1],
                           jobs[k][2])
        cc = (ImuCarry * max(n, 1))(*[imu_carry_to_c(c) for c in carries])
        cs = (State * max(n, 1))(*[state_to_c(s) for s in states])
        cap = (max([m.shape[0] for m in imus] + [0]) + 1) if pose_cap is None else pose_cap
        poses = np.zeros((max(n, 1), cap, 22)) if want_poses else None
        cnt = np.zeros(max(n, 1), np.int32)
        q = imu_params_to_c(params)
        _check("livo_imu_propagate_batch", self._L.livo_imu_propagate_batch(
            self.h, n, C.cast(cj, C.c_void_p), C.byref(q), C.cast(cc, C.c_void_p), C.cast(cs, C.c_void_p),
            _ptr(poses), cap, _ptr(cnt)))
        return ([state_from_c(cs[k]) for k in range(n)], [imu_carry_from_c(cc[k]) for k in range(n)],
                [poses[k, :cnt[k]].copy() for k in range(n)] if want_poses else None)

    def scan_preprocess_imu(self, raw: np.ndarray, leaf_size: float = 0.5):
        """scan_preprocess with the resident table and end pose of the last imu_propagate."""
        raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 5)
        n = raw.shape[0]
        und = np.zeros_like(raw)
        down = np.zeros_like(raw)
        nd = C.c_int64()
        sid = C.c_int32()
        _check("livo_scan_preprocess_imu", self._L.livo_scan_preprocess_imu(
            self.h, _ptr(raw), n, leaf_size, C.byref(sid), _ptr(und), _ptr(down), n, C.byref(nd)))
        self.scans[sid.value] = int(nd.value)
        return sid.value, und, down[:nd.value].copy()

    def frame_ingest_livox(self, pts: np.ndarray, params: IngestParams | None = None) -> dict:
        """A livox CustomMsg's points (LIVOX_POINT_DTYPE, or raw bytes of 20 a point) through avia_handler and
        the time sort on the device (livo_frame_ingest_livox); the frame stays resident.  -> the info dict."""
        pts = np.ascontiguousarray(pts)
        n = pts.nbytes // 20
        info = IngestInfo()
        _check("livo_frame_ingest_livox", self._L.livo_frame_ingest_livox(
            self.h, C.byref(params or ingest_params()), _ptr(pts) if n else None, n, C.byref(info)))
        return _stats_dict(info)

    def frame_ingest_cloud(self, data: np.ndarray, layout: CloudLayout, params: IngestParams) -> dict:
        """A PointCloud2's data (bytes, point_step a point) through the handler of params.lidar_type
        (livo_frame_ingest_cloud).  -> the info dict."""
        data = np.ascontiguousarray(data)
        n = data.nbytes // layout.point_step
        info = IngestInfo()
        _check("livo_frame_ingest_cloud", self._L.livo_frame_ingest_cloud(
            self.h, C.byref(params), _ptr(data) if n else None, n, C.byref(layout), C.byref(info)))
        return _stats_dict(info)

    def frame_info(self) -> dict:
        info = IngestInfo()
        _check("livo_frame_info", self._L.livo_frame_info(self.h, C.byref(info)))
        return _stats_dict(info)

    def frame_dump(self) -> np.ndarray:
        """The resident, time-ordered frame (n_kept, 5: x, y, z, intensity, curvature ms)."""
        n = C.c_int64()
        _check("livo_frame_dump", self._L.livo_frame_dump(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 5), np.float32)
        if n.value:
            _check("livo_frame_dump", self._L.livo_frame_dump(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def frame_take(self, offset_limit_ms: float, is_lidar_end: bool, leaf_size: float = 0.5, make_scan: bool = True):
        """UndistortPcl's slice of the resident frame from its cursor, then scan_preprocess_imu's body on it
        (livo_frame_take).  -> (n_taken, scan id or -1, de-skewed points, downsampled cloud); with
        make_scan=False (a camera frame) only the cursor moves: (n_taken, None, None, None)."""
        nt = C.c_int64()
        if not make_scan:
            _check("livo_frame_take", self._L.livo_frame_take(self.h, offset_limit_ms, int(is_lidar_end), leaf_size,
                                                              None, None, None, 0, None, C.byref(nt)))
            return nt.value, None, None, None
        cap = max(self.frame_info()["n_kept"], 1)
        und = np.zeros((cap, 5), np.float32)
        down = np.zeros((cap, 5), np.float32)
        nd, sid = C.c_int64(), C.c_int32()
        _check("livo_frame_take", self._L.livo_frame_take(self.h, offset_limit_ms, int(is_lidar_end), leaf_size,
                                                          C.byref(sid), _ptr(und), _ptr(down), cap, C.byref(nd),
                                                          C.byref(nt)))
        if sid.value >= 0:
            self.scans[sid.value] = int(nd.value)
        return nt.value, sid.value, und[:nt.value].copy(), down[:nd.value].copy()

    def lio_frame(self, imu: np.ndarray, pcl_beg_time: float, pcl_end_time: float, params: dict | None, carry: dict,
                  state: dict, offset_limit_ms: float, filter_size_surf: float = 0.5, filter_size_map_min: float = 0.5,
                  match_leaf: float = 0.2, ekf_inited: bool = True, first_scan: bool = False,
                  dense_map_en: bool = True, prev_scan_id: int = -1):
        """One LiDAR frame of the ingested message in one call (livo_lio_frame): imu_propagate, frame_take,
        the first scan's map or adopt + iekf_update + map_incremental + cloud_publish, the state on the device
        in between.  -> (state, state_propagat, carry, stats); stats: stage (LIO_*), scan_id, n_taken, n_down,
        map_built, iter (the raw IterStats bytes as `iter_raw`, and iekf_update's dict as `iter`), map_counts,
        cloud (cloud_info's dict)."""
        imu = np.ascontiguousarray(imu, np.float64).reshape(-1, 7)
        job = ImuJob(_ptr(imu).value if imu.shape[0] else None, imu.shape[0], pcl_beg_time, pcl_end_time)
        q, cy, s, sp = imu_params_to_c(params), imu_carry_to_c(carry), state_to_c(state), State()
        lp = LioParams(filter_size_surf, match_leaf, filter_size_map_min, int(bool(ekf_inited)), int(bool(first_scan)),
                       int(bool(dense_map_en)), int(prev_scan_id))
        ls = LioStats()
        _check("livo_lio_frame", self._L.livo_lio_frame(self.h, C.byref(job), C.byref(q), C.byref(cy), offset_limit_ms,
                                                        C.byref(lp), C.byref(s), C.byref(sp), C.byref(ls)))
        if ls.scan_id >= 0:
            self.scans[ls.scan_id] = int(ls.n_down)
        if ls.stage == LIO_UPDATED and prev_scan_id >= 0:
            self.scans.pop(prev_scan_id, None)
        stats = {"stage": ls.stage, "scan_id": ls.scan_id, "n_taken": ls.n_taken, "n_down": ls.n_down,
                 "map_built": ls.map_built, "iter": stats_from_c(ls.iter),
                 "iter_raw": np.frombuffer(bytes(ls.iter), np.uint8).copy(),
                 "map_counts": [int(ls.map_counts[0]), int(ls.map_counts[1])],
                 "cloud": {f: int(getattr(ls.cloud, f)) for f, _ in CloudInfo._fields_ if f != "pad_"}}
        return state_from_c(s), state_from_c(sp), imu_carry_from_c(cy), stats

    # ------------------------------------------------------------ VIO ----
    def vio_update(self, frame: dict, state: dict, prior: dict | None = None, max_iter: int = 4,
                   img_point_cov: float = 10.0):
        """LidarSelector::ComputeJ / UpdateState on a frame dict (livo_amd.synth.make_vio_frame layout):
        image, cam, pos, levels, patches, patch_size, Rci, Pci.  Returns (state, stats, errors)."""
        p = VioParams()
        _check("livo_vio_params_default", self._L.livo_vio_params_default(C.byref(p)))
        cam = frame["cam"]
        p.cam.fx, p.cam.fy, p.cam.cx, p.cam.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        p.cam.d[:] = list(cam["d"]) + [0.0] * (5 - len(cam["d"]))
        p.cam.width, p.cam.height = cam["width"], cam["height"]
        p.R_ci[:] = np.asarray(frame["Rci"], np.float64).reshape(9).tolist()
        p.P_ci[:] = np.asarray(frame["Pci"], np.float64).reshape(3).tolist()
        p.img_point_cov = img_point_cov
        p.patch_size = frame["patch_size"]
        p.max_iterations = max_iter
        img = np.ascontiguousarray(frame["image"], np.uint8)
        pos = np.ascontiguousarray(frame["pos"], np.float64).reshape(-1, 3)
        lev = np.ascontiguousarray(frame["levels"], np.int32)
        pat = np.ascontiguousarray(frame["patches"], np.float32)
        n = pos.shape[0]
        s = state_to_c(state)
        pr = state_to_c(prior) if prior is not None else None
        err = np.zeros(max(n, 1), np.float32)
        st = VioStats()
        _check("livo_vio_update", self._L.livo_vio_update(
            self.h, C.byref(p), _ptr(img), img.shape[1], img.shape[0], _ptr(pos), _ptr(lev), _ptr(pat), n,
            C.byref(s), C.byref(pr) if pr is not None else None, _ptr(err), C.byref(st)))
        stats = {"iterations": list(st.iterations), "updates": list(st.updates), "last_error": list(st.last_error),
                 "cov_updated": st.cov_updated, "n_meas": st.n_meas, "out_of_frame": st.out_of_frame}
        return state_from_c(s), stats, err[:n]

    def vio_select(self, state: dict, gray, vio_params: VioParams, grid_size: int, scan_id: int = -1):
        """LidarSelector::addSparseMap (livo_vio_select): of the cloud of frame_to_world(state, scan_id), the
        best shiTomasi-scored point of every grid_size cell of the gray image in the camera of vio_params
        (cam, R_ci, P_ci, patch_size) at `state`, with its level 0..2 patches.  gray: (height, width) uint8;
        None reuses the image of the previous call.  Returns (points: VIS_POINT_DTYPE array in ascending
        cell order, patches: (n, 3 * patch_size^2) float32 as vio_update reads them, stats: dict)."""
        st = state_to_c(state)
        img = None
        if gray is not None:
            img = np.ascontiguousarray(gray, np.uint8)
            if img.ndim != 2:
                raise ValueError("gray must be (height, width)")
            w, h = img.shape[1], img.shape[0]
        else:
            w, h = vio_params.cam.width, vio_params.cam.height
        n = C.c_int64()
        vs = VisStats()
        # the sizing call uploads the image; the real one reuses it
        _check("livo_vio_select", self._L.livo_vio_select(
            self.h, scan_id, C.byref(st), C.byref(vio_params), grid_size, _ptr(img), w, h, None, None, 0,
            C.byref(n), C.byref(vs)))
        cap = n.value
        pst3 = 3 * vio_params.patch_size * vio_params.patch_size
        pts = np.zeros(cap, VIS_POINT_DTYPE)
        pat = np.zeros((cap, pst3), np.float32)
        if cap > 0:
            _check("livo_vio_select", self._L.livo_vio_select(
                self.h, scan_id, C.byref(st), C.byref(vio_params), grid_size, None, w, h, _ptr(pts), _ptr(pat), cap,
                C.byref(n), C.byref(vs)))
        stats = {f: int(getattr(vs, f)) for f, _ in VisStats._fields_}
        return pts[:n.value], pat[:n.value], stats

    # ------------------------------------------------- the visual map ----
    def vmap_reset(self, max_points: int, max_frames: int, patch_size: int):
        """An empty resident visual map of fixed capacities (livo_vmap_reset)."""
        _check("livo_vmap_reset", self._L.livo_vmap_reset(self.h, max_points, max_frames, patch_size))

    def vmap_add_frame(self, frame_id: int, state: dict, vio_params: VioParams, gray=None):
        """Stores a past gray image (None: vio_select's retained one) and its pose under frame_id."""
        st = state_to_c(state)
        img = None if gray is None else np.ascontiguousarray(gray, np.uint8)
        if img is not None and img.ndim != 2:
            raise ValueError("gray must be (height, width)")
        w, h = (vio_params.cam.width, vio_params.cam.height) if img is None else (img.shape[1], img.shape[0])
        _check("livo_vmap_add_frame", self._L.livo_vmap_add_frame(
            self.h, frame_id, C.byref(st), C.byref(vio_params), _ptr(img), w, h))

    def vmap_add(self, frame_id: int, pts, patches, point_ids=None, levels=None):
        """Observations from frame_id (livo_vmap_add): pts a VIS_POINT_DTYPE array, patches (n, 3 ps^2).
        point_ids None creates the points and returns their ids; else one observation is appended to each."""
        pts = np.ascontiguousarray(pts, VIS_POINT_DTYPE)
        pat = np.ascontiguousarray(patches, np.float32)
        n = len(pts)
        ids = None if point_ids is None else np.ascontiguousarray(point_ids, np.int32)
        lev = None if levels is None else np.ascontiguousarray(levels, np.int32)
        if pat.size != n * 3 * self.vmap_info()["patch_size"] ** 2 or (ids is not None and len(ids) != n) or \
                (lev is not None and len(lev) != n):
            raise ValueError("pts, patches, point_ids and levels disagree in length")
        out = np.zeros(n, np.int32)
        _check("livo_vmap_add", self._L.livo_vmap_add(
            self.h, frame_id, n, _ptr(ids), _ptr(pts), _ptr(lev), _ptr(pat), _ptr(out)))
        return out if ids is None else ids

    def vmap_info(self) -> dict:
        v = VmapCounts()
        _check("livo_vmap_info", self._L.livo_vmap_info(self.h, C.byref(v)))
        return {f: int(getattr(v, f)) for f, _ in VmapCounts._fields_ if f != "pad_"}

    def vmap_dump(self):
        """(points: VMAP_POINT_DTYPE, obs: VMAP_OBS_DTYPE, patches (n_obs, 3 ps^2)) in id / list order."""
        n_p, n_o = C.c_int64(), C.c_int64()
        _check("livo_vmap_dump", self._L.livo_vmap_dump(self.h, None, 0, None, None, 0, C.byref(n_p), C.byref(n_o)))
        ps = self.vmap_info()["patch_size"]
        pts = np.zeros(n_p.value, VMAP_POINT_DTYPE)
        obs = np.zeros(n_o.value, VMAP_OBS_DTYPE)
        pat = np.zeros((n_o.value, 3 * ps * ps), np.float32)
        if n_p.value > 0:
            _check("livo_vmap_dump", self._L.livo_vmap_dump(
                self.h, _ptr(pts), len(pts), _ptr(obs), _ptr(pat), len(obs), C.byref(n_p), C.byref(n_o)))
        return pts, obs, pat

    def vio_match(self, state: dict, gray, vio_params: VioParams, grid_size: int, ncc_en: bool = False,
                  ncc_thre: float = 0.0, outlier_threshold: float = 100.0, scan_id: int = -1, frame: dict = None):
        """LidarSelector::addFromSparseMap (livo_vio_match): the resident visual map matched into the gray
        image (None: the image of the previous call) in the camera of vio_params at `state`, the cloud of
        frame_to_world(state, scan_id) giving the voxel set and the depth image.  Returns a dict that
        vio_update accepts (pos, levels, patches, patch_size, cam, Rci, Pci and, when gray is given, image)
        with records (VMATCH_POINT_DTYPE, ascending cell) and stats; `frame` entries are copied in first."""
        st = state_to_c(state)
        img = None
        if gray is not None:
            img = np.ascontiguousarray(gray, np.uint8)
            if img.ndim != 2:
                raise ValueError("gray must be (height, width)")
            w, h = img.shape[1], img.shape[0]
        else:
            w, h = vio_params.cam.width, vio_params.cam.height
        n = C.c_int64()
        vs = VmatchStats()
        head = (self.h, scan_id, C.byref(st), C.byref(vio_params), grid_size, int(bool(ncc_en)), float(ncc_thre),
                float(outlier_threshold))
        # the sizing call uploads the image; the real one reuses it
        _check("livo_vio_match", self._L.livo_vio_match(
            *head, _ptr(img), w, h, None, None, None, None, 0, C.byref(n), C.byref(vs)))
        cap = n.value
        pst3 = 3 * vio_params.patch_size * vio_params.patch_size
        rec = np.zeros(cap, VMATCH_POINT_DTYPE)
        pos = np.zeros((cap, 3), np.float64)
        lev = np.zeros(cap, np.int32)
        pat = np.zeros((cap, pst3), np.float32)
        if cap > 0:
            _check("livo_vio_match", self._L.livo_vio_match(
                *head, None, w, h, _ptr(rec), _ptr(pos), _ptr(lev), _ptr(pat), cap, C.byref(n), C.byref(vs)))
        cam = vio_params.cam
        out = dict(frame or {})
        out.update({"pos": pos, "levels": lev, "patches": pat, "patch_size": int(vio_params.patch_size),
                    "cam": {"fx": cam.fx, "fy": cam.fy, "cx": cam.cx, "cy": cam.cy, "d": list(cam.d),
                            "width": cam.width, "height": cam.height},
                    "Rci": np.array(vio_params.R_ci[:]).reshape(3, 3), "Pci": np.array(vio_params.P_ci[:]),
                    "records": rec, "stats": {f: int(getattr(vs, f)) for f, _ in VmatchStats._fields_}})
        if img is not None:
            out["image"] = img
        return out

    def vio_observe(self, frame_id: int, point_ids, levels=None):
        """LidarSelector::addObservation (livo_vio_observe): the resident visual map brought up to date with the
        stored frame frame_id (stored at the state after vio_update).  point_ids / levels: the point_id and
        search_level columns of vio_match's records (levels None: 0); no id twice.  Returns (records:
        VOBS_POINT_DTYPE in input order, stats: dict)."""
        ids = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        lev = None if levels is None else np.ascontiguousarray(levels, np.int32).reshape(-1)
        if lev is not None and len(lev) != len(ids):
            raise ValueError("point_ids and levels disagree in length")
        rec = np.zeros(len(ids), VOBS_POINT_DTYPE)
        vs = VobsStats()
        _check("livo_vio_observe", self._L.livo_vio_observe(
            self.h, frame_id, len(ids), _ptr(ids), _ptr(lev), _ptr(rec), C.byref(vs)))
        return rec, {f: int(getattr(vs, f)) for f, _ in VobsStats._fields_}

    def vio_detect(self, frame_id: int, state: dict, gray, vio_params: VioParams, grid_size: int,
                   ncc_en: bool = False, ncc_thre: float = 0.0, outlier_threshold: float = 100.0, scan_id: int = -1,
                   prior: dict | None = None):
        """LidarSelector::detect (livo_vio_detect): one camera frame in one call, equal to vio_match and
        vio_select at `state`, vio_update on the survivors, vmap_add_frame(frame_id) at the updated state,
        vio_observe of the survivors and vmap_add of the selected points, with nothing but counters, the state
        and the observe's records crossing to the host.  vio_params carries max_iterations and img_point_cov.
        Returns (state, {"match", "select", "update", "observe": the stages' stats dicts, "n_matched", "n_new",
        "first_new_id"})."""
        img = np.ascontiguousarray(gray, np.uint8)
        if img.ndim != 2:
            raise ValueError("gray must be (height, width)")
        st = state_to_c(state)
        pr = state_to_c(prior) if prior is not None else None
        d = VdetectParams(int(grid_size), int(bool(ncc_en)), float(ncc_thre), float(outlier_threshold))
        vs = VdetectStats()
        _check("livo_vio_detect", self._L.livo_vio_detect(
            self.h, scan_id, frame_id, C.byref(st), C.byref(pr) if pr is not None else None, C.byref(vio_params),
            C.byref(d), _ptr(img), img.shape[1], img.shape[0], C.byref(vs)))
        stats = {k: _stats_dict(getattr(vs, k)) for k in ("match", "select", "update", "observe")}
        stats.update(n_matched=int(vs.n_matched), n_new=int(vs.n_new), first_new_id=int(vs.first_new_id))
        return state_from_c(st), stats

    def vmap_release_frames(self) -> np.ndarray:
        """Releases the stored frames that no observation refers to (livo_vmap_release_frames); their slots go
        to the frames stored next.  Returns the released frame ids, ascending."""
        n = C.c_int64()
        _check("livo_vmap_release_frames", self._L.livo_vmap_release_frames(self.h, None, 0, C.byref(n)))
        ids = np.zeros(n.value, np.int32)
        if n.value > 0:
            _check("livo_vmap_release_frames", self._L.livo_vmap_release_frames(self.h, _ptr(ids), len(ids),
                                                                                C.byref(n)))
        return ids[:n.value]

    def std_reset(self, params: StdParams | None = None, max_descs: int = 1 << 16, max_frames: int = 1024,
                  max_planes: int = 1 << 18):
        """An empty loop-search database (livo_std_reset)."""
        _check("livo_std_reset", self._L.livo_std_reset(self.h, C.byref(params or std_params()), max_descs,
                                                        max_frames, max_planes))

    def std_stage(self, descs: np.ndarray, planes: np.ndarray):
        """The current key frame: descriptors (STD_DESC_DTYPE) and plane cloud (STD_PLANE_DTYPE), uploaded once."""
        descs = np.ascontiguousarray(descs, STD_DESC_DTYPE)
        planes = np.ascontiguousarray(planes, STD_PLANE_DTYPE)
        _check("livo_std_stage", self._L.livo_std_stage(self.h, _ptr(descs) if descs.size else None, descs.size,
                                                        _ptr(planes) if planes.size else None, planes.size))

    def std_search(self, pair_cap: int | None = None) -> dict:
        """SearchLoop of the staged frame -> frame (-1: none), score, rot (3, 3), t, n_candidates, candidate,
        pairs (STD_PAIR_DTYPE, the winner's success list)."""
        r = StdResult()
        n = C.c_int64()
        cap = self.std_info()["staged_descs"] * 27 if pair_cap is None else pair_cap
        pairs = np.zeros(max(cap, 0), STD_PAIR_DTYPE)
        _check("livo_std_search", self._L.livo_std_search(self.h, C.byref(r), _ptr(pairs) if cap > 0 else None, cap,
                                                          C.byref(n)))
        if n.value > cap:  # (a cell's run may hold several matches of one source)
            return self.std_search(int(n.value))
        return {"frame": r.frame, "score": r.score, "rot": np.array(r.rot[:], np.float64).reshape(3, 3),
                "t": np.array(r.t[:], np.float64), "n_candidates": r.n_candidates, "candidate": r.candidate,
                "n_pairs": r.n_pairs, "pairs": pairs[:n.value].copy()}

    def std_commit(self) -> int:
        """AddSTDescs of the staged frame -> its frame index."""
        f = C.c_int32()
        _check("livo_std_commit", self._L.livo_std_commit(self.h, C.byref(f)))
        return f.value

    def std_candidates(self) -> np.ndarray:
        """The last search's candidates in candidate order (STD_CANDIDATE_DTYPE)."""
        n = C.c_int64()
        _check("livo_std_candidates", self._L.livo_std_candidates(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, STD_CANDIDATE_DTYPE)
        if n.value:
            _check("livo_std_candidates", self._L.livo_std_candidates(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def std_matches(self, candidate: int) -> np.ndarray:
        """One candidate's match list in the selector's order (STD_PAIR_DTYPE)."""
        n = C.c_int64()
        _check("livo_std_matches", self._L.livo_std_matches(self.h, candidate, None, 0, C.byref(n)))
        out = np.zeros(n.value, STD_PAIR_DTYPE)
        if n.value:
            _check("livo_std_matches", self._L.livo_std_matches(self.h, candidate, _ptr(out), n.value, C.byref(n)))
        return out

    def std_info(self) -> dict:
        info = StdInfo()
        _check("livo_std_info_get", self._L.livo_std_info_get(self.h, C.byref(info)))
        return _stats_dict(info)

    def std_dump(self, frame: int = -1):
        """-> the stored descriptors in insertion order, and the plane cloud of `frame` (empty for -1)."""
        nd, npl = C.c_int64(), C.c_int64()
        _check("livo_std_dump", self._L.livo_std_dump(self.h, None, 0, C.byref(nd), frame, None, 0, C.byref(npl)))
        descs = np.zeros(nd.value, STD_DESC_DTYPE)
        planes = np.zeros(npl.value if frame >= 0 else 0, STD_PLANE_DTYPE)
        _check("livo_std_dump", self._L.livo_std_dump(self.h, _ptr(descs) if descs.size else None, descs.size,
                                                      C.byref(nd), frame, _ptr(planes) if planes.size else None,
                                                      planes.size, C.byref(npl)))
        return descs, planes

    def std_key_add(self, scan_id: int = CLOUD_WORLD):
        """Appends a resident cloud (the published world cloud by default) to the key cloud, device to device."""
        _check("livo_std_key_add", self._L.livo_std_key_add(self.h, scan_id))

    def std_key_add_host(self, xyz: np.ndarray):
        """Appends host points (n x 3 or wider rows, float32; the first three columns) to the key cloud."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        xyz = xyz.reshape(-1, xyz.shape[-1] if xyz.ndim > 1 else 3)
        _check("livo_std_key_add_host", self._L.livo_std_key_add_host(self.h, _ptr(xyz) if xyz.size else None, xyz.shape[0],
                                                                      xyz.shape[1] * 4))

    def std_key_clear(self):
        _check("livo_std_key_clear", self._L.livo_std_key_clear(self.h))

    def std_key_count(self) -> int:
        n = C.c_int64()
        _check("livo_std_key_count", self._L.livo_std_key_count(self.h, C.byref(n)))
        return int(n.value)

    def std_generate(self, params: StdGenParams | None = None) -> dict:
        """GenerateSTDescs of the key cloud; its products become the staged frame.  -> the stages' counts."""
        st = StdGenStats()
        _check("livo_std_generate", self._L.livo_std_generate(self.h, C.byref(params or std_gen_params()), C.byref(st)))
        return _stats_dict(st)

    def std_staged(self):
        """-> the staged frame's descriptors, plane cloud and final corner list (STD_CORNER_DTYPE)."""
        nd, npl, nc = C.c_int64(), C.c_int64(), C.c_int64()
        _check("livo_std_staged", self._L.livo_std_staged(self.h, None, 0, C.byref(nd), None, 0, C.byref(npl), None, 0,
                                                          C.byref(nc)))
        descs = np.zeros(nd.value, STD_DESC_DTYPE)
        planes = np.zeros(npl.value, STD_PLANE_DTYPE)
        corners = np.zeros(nc.value, STD_CORNER_DTYPE)
        _check("livo_std_staged", self._L.livo_std_staged(
            self.h, _ptr(descs) if descs.size else None, descs.size, C.byref(nd), _ptr(planes) if planes.size else None,
            planes.size, C.byref(npl), _ptr(corners) if corners.size else None, corners.size, C.byref(nc)))
        return descs, planes, corners

    def std_gen_debug(self):
        """The last generate's voxels (visiting order: first point, count, plane flag) and jobs (voxel rank, plane
        voxel rank, projected points, 27 member ranks + 1)."""
        nv, nj = C.c_int64(), C.c_int64()
        _check("livo_std_gen_debug", self._L.livo_std_gen_debug(self.h, None, 0, C.byref(nv), None, 0, C.byref(nj)))
        vox = np.zeros((nv.value, 3), np.int32)
        jobs = np.zeros((nj.value, 30), np.int32)
        _check("livo_std_gen_debug", self._L.livo_std_gen_debug(self.h, _ptr(vox) if vox.size else None, nv.value,
                                                                C.byref(nv), _ptr(jobs) if jobs.size else None, nj.value,
                                                                C.byref(nj)))
        return vox, jobs

    def scan_inherit_neighbors(self, dst: int, src: int):
        _check("livo_scan_inherit_neighbors", self._L.livo_scan_inherit_neighbors(self.h, dst, src))

    def set_profiling(self, level):
        """0/False off, 1 first-search timing only, 2/True every stage (livo_ctx_set_profiling)."""
        level = 2 if level is True else int(level)
        _check("livo_ctx_set_profiling", self._L.livo_ctx_set_profiling(self.h, level))

    def last_timings(self) -> dict:
        t = Timings()
        _check("livo_last_timings", self._L.livo_last_timings(self.h, C.byref(t)))
        out = {}
        for f, _ in Timings._fields_:
            v = getattr(t, f)
            out[f] = list(v)[:t.n_evals] if f in ("eval_ms", "eval_searched") else v
        return out

    def sync(self):
        _check("livo_sync", self._L.livo_sync(self.h))
