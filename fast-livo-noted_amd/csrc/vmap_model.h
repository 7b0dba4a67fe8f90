// vmap_model.h — the arithmetic of one item of LidarSelector::addFromSparseMap
// (src/lidar_selection.cpp:332-593) with getWarpMatrixAffine, getBestSearchLevel,
// warpAffine and NCC (:224-318) and Point::getCloseViewObs (src/point.cpp:142-170):
// a cloud point's voxel key and depth pixel, a map point's bid for its grid cell,
// the depth-continuity test's one pixel, the view choice, the affine matrix and its
// search level, one warped sample, NCC and the squared error.  Everything compiles
// for host and device (SEL_HD), as cam_model.h, so tests/native/vmatch_point_check.cpp
// runs the kernels' code on the CPU.  Numerics: -ffp-contract=off, one IEEE operation
// per step in the order DESIGN.md §8.9 states; 3-term sums left to right.
//
// At the end, the arithmetic of one item of LidarSelector::addObservation
// (src/lidar_selection.cpp:905-962) with Point::getFurthestViewObs
// (src/point.cpp:211-239): the projection and its two skips, delta_p, the pixel
// distance and the observation to evict.  The reference's `delta_theta > 10`
// compares an acos (at most pi; NaN compares false) with 10: it never holds and
// is not computed.  tests/native/vobserve_point_check.cpp runs these on the CPU.
// vm_make_frame, vm_make_obs and vm_make_point build what the store holds of a
// frame, an observation and a new point: the host path (livo_vmap_add_frame,
// livo_vmap_add) and livo_vio_detect's kernels (k_vm_frame, k_vm_fresh) call the
// same functions; tests/native/vdetect_point_check.cpp runs them on the CPU.
#pragma once
#include "cam_model.h"

namespace livo {

constexpr int kVmMaxObs = 20;  // addObservation's cap (:945)

// A stored past frame: imgs_[id] and the features' T_f_w_.
struct VmFrame {
    int32_t id, pad_;
    double Rcw[9], Pcw[3];
    double pos[3];  // T_f_w_.inverse().translation() = -Rcw^T Pcw
};
// One observation (Feature) of a map point, as the device holds it.
struct alignas(8) VmObs {
    int32_t frame_id, level;
    int32_t slot, pad_;  // the frame's slot in the store
    double px[2];
    double f[3];
};
// One map point (Point).
struct alignas(8) VmPoint {
    double pos[3];
    float value;
    int32_t n_obs;
    int64_t voxel[3];  // AddPoint's VOXEL_KEY (vis_voxel_key)
};

SEL_HD double vm_norm3(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// -Rcw^T Pcw.
SEL_HD void vm_frame_pos(const double* Rcw, const double* Pcw, double* pos) {
    for (int k = 0; k < 3; k++) pos[k] = -((Rcw[0 * 3 + k] * Pcw[0] + Rcw[1 * 3 + k] * Pcw[1]) + Rcw[2 * 3 + k] * Pcw[2]);
}

// vikit PinholeCamera::cam2world of an undistorted camera: ((u - cx) / fx, (v - cy) / fy, 1) normalised.
SEL_HD void vm_cam2world(const CamIntrinsics& K, double u, double v, double* f) {
    const double x = (u - K.cx) / K.fx, y = (v - K.cy) / K.fy;
    const double n = sqrt((x * x + y * y) + 1.0);
    f[0] = x / n;
    f[1] = y / n;
    f[2] = 1.0 / n;
}

// The frame stored under `id` at camera C: its Rcw, Pcw and position.
SEL_HD VmFrame vm_make_frame(int32_t id, const FrameCam& C) {
    VmFrame f{};
    f.id = id;
    for (int k = 0; k < 9; k++) f.Rcw[k] = C.Rcw[k];
    for (int k = 0; k < 3; k++) f.Pcw[k] = C.Pcw[k];
    vm_frame_pos(f.Rcw, f.Pcw, f.pos);
    return f;
}

// The observation of pixel (u, v) from the frame stored in `slot` (Feature).
SEL_HD VmObs vm_make_obs(const CamIntrinsics& K, int32_t frame_id, int32_t slot, int32_t level, double u, double v) {
    VmObs o{};
    o.frame_id = frame_id;
    o.level = level;
    o.slot = slot;
    o.px[0] = u;
    o.px[1] = v;
    vm_cam2world(K, u, v, o.f);
    return o;
}

// A new map point from a selected record (addSparseMap's tail): the float
// position widened, value = score, the voxel key copied, one observation.
SEL_HD VmPoint vm_make_point(const livo_vis_point& r) {
    VmPoint q{};
    q.pos[0] = (double)r.x;
    q.pos[1] = (double)r.y;
    q.pos[2] = (double)r.z;
    q.value = r.score;
    q.n_obs = 1;
    for (int k = 0; k < 3; k++) q.voxel[k] = r.voxel[k];
    return q;
}

// isInFrame(px.cast<int>(), border) taken in double (a NaN fails it), as vis_project.
SEL_HD bool vm_in_frame(const CamIntrinsics& K, int border, const double* px) {
    const double b = (double)border;
    return px[0] >= b && px[0] < (double)(K.w - border) && px[1] >= b && px[1] < (double)(K.h - border);
}

// One cloud point of the depth pass (:367-401): its voxel key floor(p / 0.5) and,
// where it lands in the frame in front of the camera, its pixel and depth.  The
// pixel is fx * x / z + cx, left to right: not world2cam's fx * (x / z) + cx.
SEL_HD bool vm_cloud_point(const FrameCam& C, int border, float wx, float wy, float wz, int64_t* key, int64_t& pix,
                           float& depth) {
    const double pw[3] = {(double)wx, (double)wy, (double)wz};
    for (int j = 0; j < 3; j++) {
        const double q = floor(pw[j] / 0.5);
        key[j] = q >= -1e9 && q <= 1e9 ? (int64_t)q : INT64_MIN;  // (a NaN or a huge coordinate: in no set)
    }
    double pf[3];
    cam_w2f(C.Rcw, C.Pcw, pw, pf);
    if (!(pf[2] > 0)) return false;
    const double px[2] = {C.fx * pf[0] / pf[2] + C.cx, C.fy * pf[1] / pf[2] + C.cy};
    if (!vm_in_frame(C, border, px)) return false;
    pix = (int64_t)(int)px[1] * C.w + (int)px[0];
    depth = (float)pf[2];
    return true;
}

// A voxel key as one 64-bit word: 21 bits per axis around 2^20.  False outside
// that range (|p| >= 2^19 m): such a voxel is in no frame set.
SEL_HD bool vm_pack_key(const int64_t* key, unsigned long long& packed) {
    const int64_t off = (int64_t)1 << 20;
    packed = 0ull;
    for (int j = 0; j < 3; j++) {
        const int64_t k = key[j] + off;
        if (k < 0 || k >= 2 * off) return false;
        packed = (packed << 21) | (unsigned long long)k;
    }
    return true;
}
SEL_HD uint32_t vm_hash(unsigned long long k, int log2) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (uint32_t)(k & ((1ull << log2) - 1ull));
}

enum VmFate : int { kVmSkip = 0, kVmInFrame = 1, kVmOverflow = 2 };

// One map point of the map pass (:420-447) up to its cell and distance: skipped
// behind the camera (pt_cam.z < 0: a NaN passes) or outside the border.
SEL_HD int vm_map_point(const FrameCam& C, const VisGrid& G, const double* fpos, const double* pos, double* pf,
                        double* pc, int& index, float& dist) {
    cam_w2f(C.Rcw, C.Pcw, pos, pf);
    if (pf[2] < 0) return kVmSkip;
    vio_world2cam(C, pf, pc);
    if (!vm_in_frame(C, G.border, pc)) return kVmSkip;
    index = (int)(pc[0] / G.grid_size) * G.grid_n_height + (int)(pc[1] / G.grid_size);
    const double d[3] = {fpos[0] - pos[0], fpos[1] - pos[1], fpos[2] - pos[2]};
    dist = (float)vm_norm3(d);
    return index >= G.length ? kVmOverflow : kVmInFrame;
}

// A cell's bid: the least distance wins, the greatest point id among equals.
// kVmBidNone marks a cell whose points are all beyond 10000 m (or NaN).
constexpr unsigned long long kVmBidEmpty = ~0ull, kVmBidNone = 0xFFFFFFFEFFFFFFFFull;
SEL_HD unsigned long long vm_bid(float dist, uint32_t id) {
    if (!(dist <= 10000.0f)) return kVmBidNone;
    uint32_t b;
    memcpy(&b, &dist, 4);
    return ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - id);
}

// One pixel of the depth-continuity test (:484-490): true rejects.
SEL_HD bool vm_depth_breaks(double z, float depth) { return depth != 0.0f && fabs(z - (double)depth) > 1.5; }

// Point::getCloseViewObs: the first observation of the strictly greatest cosine
// above 0, else the first one; cosine = that maximum (0 if none exceeds it).
SEL_HD int vm_close_view(const double* fpos, const double* pos, const VmObs* obs, int n, const VmFrame* frames,
                         double& cosine) {
    double o[3] = {fpos[0] - pos[0], fpos[1] - pos[1], fpos[2] - pos[2]};
    const double on = vm_norm3(o);
    for (int k = 0; k < 3; k++) o[k] /= on;
    int best = 0;
    cosine = 0.0;
    for (int i = 0; i < n; i++) {
        const double* rp = frames[obs[i].slot].pos;
        double d[3] = {rp[0] - pos[0], rp[1] - pos[1], rp[2] - pos[2]};
        const double dn = vm_norm3(d);
        for (int k = 0; k < 3; k++) d[k] /= dn;
        const double c = (o[0] * d[0] + o[1] * d[1]) + o[2] * d[2];
        if (c > cosine) {
            cosine = c;
            best = i;
        }
    }
    return best;
}

// getWarpMatrixAffine (:236-245) at level_ref = pyramid_level = 0 for the
// undistorted pinhole: A row-major (a00, a01, a10, a11), its columns the images
// of the reference patch's half-axes.  T_cur_ref = (Rc Rr^T, Pc - R Pr).
SEL_HD void vm_warp_matrix(const FrameCam& C, const VmFrame& ref, const VmObs& o, const double* pos, int half,
                           double* A) {
    const double d[3] = {ref.pos[0] - pos[0], ref.pos[1] - pos[1], ref.pos[2] - pos[2]};
    const double depth_ref = vm_norm3(d);
    double R[9], t[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            R[i * 3 + j] = (C.Rcw[i * 3 + 0] * ref.Rcw[j * 3 + 0] + C.Rcw[i * 3 + 1] * ref.Rcw[j * 3 + 1]) +
                           C.Rcw[i * 3 + 2] * ref.Rcw[j * 3 + 2];
    for (int i = 0; i < 3; i++)
        t[i] = C.Pcw[i] - ((R[i * 3 + 0] * ref.Pcw[0] + R[i * 3 + 1] * ref.Pcw[1]) + R[i * 3 + 2] * ref.Pcw[2]);
    double x[3][3];  // xyz_ref, xyz_du_ref, xyz_dv_ref
    for (int k = 0; k < 3; k++) x[0][k] = o.f[k] * depth_ref;
    vm_cam2world(C, o.px[0] + (double)half, o.px[1], x[1]);
    vm_cam2world(C, o.px[0], o.px[1] + (double)half, x[2]);
    for (int m = 1; m < 3; m++) {
        const double s = x[0][2] / x[m][2];
        for (int k = 0; k < 3; k++) x[m][k] *= s;
    }
    double px[3][2];
    for (int m = 0; m < 3; m++) {
        double y[3];
        cam_w2f(R, t, x[m], y);
        vio_world2cam(C, y, px[m]);
    }
    A[0] = (px[1][0] - px[0][0]) / (double)half;
    A[2] = (px[1][1] - px[0][1]) / (double)half;
    A[1] = (px[2][0] - px[0][0]) / (double)half;
    A[3] = (px[2][1] - px[0][1]) / (double)half;
}

SEL_HD double vm_det2(const double* A) { return A[0] * A[3] - A[2] * A[1]; }

// getBestSearchLevel (:309-316).
SEL_HD int vm_search_level(const double* A, int max_level) {
    int level = 0;
    double D = vm_det2(A);
    while (D > 3.0 && level < max_level) {
        level += 1;
        D *= 0.25;
    }
    return level;
}

// A_cur_ref.inverse().cast<float>(): 1 / det times the adjugate, in double.
SEL_HD void vm_inverse2f(const double* A, float* Ai) {
    const double invdet = 1.0 / vm_det2(A);
    Ai[0] = (float)(A[3] * invdet);
    Ai[1] = (float)(-A[1] * invdet);
    Ai[2] = (float)(-A[2] * invdet);
    Ai[3] = (float)(A[0] * invdet);
}

// One value of warpAffine (:265-281), element e = y * ps + x of the level-0 patch
// (ps even), sampled from the observation's own image of w x h: 0 outside
// [0, w - 1) x [0, h - 1) (and for a NaN position, undefined in the reference),
// else vikit's interpolateMat_8u.
SEL_HD float vm_warp_sample(const float* Ai, const double* px_ref, int level, int ps, int e, const uint8_t* img,
                            int w, int h) {
    const int half = ps / 2, y = e / ps, x = e - y * ps;
    const float sc = (float)(1 << level);
    const float qx = (float)(x - half) * sc, qy = (float)(y - half) * sc;
    const float u = (Ai[0] * qx + Ai[1] * qy) + (float)px_ref[0];
    const float v = (Ai[2] * qx + Ai[3] * qy) + (float)px_ref[1];
    if (u < 0 || v < 0 || u >= (float)(w - 1) || v >= (float)(h - 1) || u != u || v != v) return 0.0f;
    const int xi = (int)floorf(u), yi = (int)floorf(v);
    const float sx = u - (float)xi, sy = v - (float)yi;
    const float w00 = (1.0f - sx) * (1.0f - sy), w01 = (1.0f - sx) * sy, w10 = sx * (1.0f - sy);
    const float w11 = ((1.0f - w00) - w01) - w10;
    const uint8_t* p = img + (int64_t)yi * w + xi;
    return ((w00 * (float)p[0] + w01 * (float)p[w]) + w10 * (float)p[1]) + w11 * (float)p[w + 1];
}

// LidarSelector::NCC (:285-302), in double, index order.
SEL_HD double vm_ncc(const float* ref, const float* cur, int n) {
    double sum_ref = 0.0, sum_cur = 0.0;
    for (int i = 0; i < n; i++) sum_ref += (double)ref[i];
    const double mean_ref = sum_ref / n;
    for (int i = 0; i < n; i++) sum_cur += (double)cur[i];
    const double mean_cur = sum_cur / n;
    double num = 0, den1 = 0, den2 = 0;
    for (int i = 0; i < n; i++) {
        const double a = (double)ref[i] - mean_ref, b = (double)cur[i] - mean_cur;
        num += a * b;
        den1 += a * a;
        den2 += b * b;
    }
    return num / sqrt(den1 * den2 + 1e-10);
}

// The patch error (:555-559): squared differences summed in float, index order.
SEL_HD float vm_error(const float* ref, const float* cur, int n) {
    float e = 0.0f;
    for (int i = 0; i < n; i++) e += (ref[i] - cur[i]) * (ref[i] - cur[i]);
    return e;
}

// ---- addObservation (:905-962) --------------------------------------------
enum VmObsFate : int { kVmObsIn = 0, kVmObsBehind = 1, kVmObsOutOfFrame = 2 };

// The item's pixel: skipped behind the camera (pt_cam.z <= 0: a NaN passes, and
// then fails the frame test) or outside the border under which vis_getpatch's
// taps are inside the image (the reference has no such test and reads outside).
SEL_HD int vm_observe_project(const FrameCam& C, int border, const double* pos, double* pc) {
    double pf[3];
    cam_w2f(C.Rcw, C.Pcw, pos, pf);
    if (pf[2] <= 0) return kVmObsBehind;
    vio_world2cam(C, pf, pc);
    return vm_in_frame(C, border, pc) ? kVmObsIn : kVmObsOutOfFrame;
}

// delta_p = |(pose_ref * pose_cur.inverse()).translation()| = |ref.Rcw cur.pos + ref.Pcw|.
SEL_HD double vm_observe_delta_p(const VmFrame& ref, const double* cur_pos) {
    double t[3];
    cam_w2f(ref.Rcw, ref.Pcw, cur_pos, t);
    return vm_norm3(t);
}

// (pc - last_px).norm().
SEL_HD double vm_pixel_dist(const double* pc, const double* px) {
    const double dx = pc[0] - px[0], dy = pc[1] - px[1];
    return sqrt(dx * dx + dy * dy);
}

// getFurthestViewObs's distance of one observation's frame from the current one.
SEL_HD double vm_view_dist(const double* ref_pos, const double* cur_pos) {
    const double d[3] = {ref_pos[0] - cur_pos[0], ref_pos[1] - cur_pos[1], ref_pos[2] - cur_pos[2]};
    return vm_norm3(d);
}

// getFurthestViewObs over the n distances in this map's list order (the
// reference's obs_ runs the other way: its front is index n - 1): from the
// highest index down, the first strictly above a maximum that starts at 0, so the
// newest among equal maxima, and index n - 1 if none exceeds 0 (all zero or NaN).
SEL_HD int vm_furthest_view(const double* dist, int n) {
    int best = n - 1;
    double maxdist = 0.0;
    for (int k = n - 1; k >= 0; k--)
        if (dist[k] > maxdist) {
            maxdist = dist[k];
            best = k;
        }
    return best;
}

}  // namespace livo
