// cam_model.h — the camera shared by the VIO update (vio_kernels.hip), the cloud
// colouring (rgb_kernels.hip) and the visual point selection (vis_kernels.hip):
// the intrinsics (CamIntrinsics) and the camera of one frame (FrameCam), each
// filled in one place from the C ABI's structs (cam_intrinsics, frame_cam); the
// frame pose from a state, vikit's pinhole world2cam, one point's colour as
// publish_frame_world_rgb computes it, and addSparseMap's score, patch and voxel
// key.  Everything compiles for host and device (SEL_HD, as ball_cells in
// livo_internal.h), so tests/native/rgb_point_check.cpp and vis_point_check.cpp
// run the same code on the CPU.  Numerics as the kernels: -ffp-contract=off, the
// reference's float / double expression order.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "livo.h"
#include "stl_select.h"  // SEL_HD

namespace livo {

// new_frame_->T_f_w_ from the state (lidar_selection.cpp:900-901):
// Rcw = Rci * Rwi^T, Pcw = -Rci * Rwi^T * Pwi + Pci.  Row-major.
SEL_HD void cam_pose(const double* Rci, const double* Pci, const double* Rwi, const double* Pwi, double* Rcw,
                     double* Pcw) {
    double RwiT[9];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) RwiT[a * 3 + b] = Rwi[b * 3 + a];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            Rcw[i * 3 + j] = (Rci[i * 3 + 0] * RwiT[0 * 3 + j] + Rci[i * 3 + 1] * RwiT[1 * 3 + j]) +
                             Rci[i * 3 + 2] * RwiT[2 * 3 + j];
    for (int k = 0; k < 3; k++)
        Pcw[k] = -((Rcw[k * 3 + 0] * Pwi[0] + Rcw[k * 3 + 1] * Pwi[1]) + Rcw[k * 3 + 2] * Pwi[2]) + Pci[k];
}

// Frame::w2f: pf = Rcw * p_w + Pcw, row sums left to right.
SEL_HD void cam_w2f(const double* Rcw, const double* Pcw, const double* pw, double* pf) {
    for (int k = 0; k < 3; k++)
        pf[k] = ((Rcw[k * 3 + 0] * pw[0] + Rcw[k * 3 + 1] * pw[1]) + Rcw[k * 3 + 2] * pw[2]) + Pcw[k];
}

// A pinhole camera at an image size (vikit PinholeCamera).
struct CamIntrinsics {
    double fx, fy, cx, cy, d[5];
    int32_t distortion;
    int32_t w, h;
};
// The camera of one frame: the intrinsics and new_frame_->T_f_w_.
struct FrameCam : CamIntrinsics {
    double Rcw[9], Pcw[3];
};

SEL_HD CamIntrinsics cam_intrinsics(const livo_cam& cam, int32_t w, int32_t h) {
    CamIntrinsics K;
    K.fx = cam.fx; K.fy = cam.fy; K.cx = cam.cx; K.cy = cam.cy;
    for (int k = 0; k < 5; k++) K.d[k] = cam.d[k];
    K.distortion = fabs(cam.d[0]) > 0.0000001 ? 1 : 0;  // vikit: distortion_ = |d0| > 1e-7
    K.w = w;
    K.h = h;
    return K;
}
// The camera of p (its cam at cam.width x cam.height, R_ci, P_ci) at a state.
SEL_HD FrameCam frame_cam(const livo_vio_params& p, const livo_state& s) {
    FrameCam C{cam_intrinsics(p.cam, p.cam.width, p.cam.height)};
    cam_pose(p.R_ci, p.P_ci, s.rot, s.pos, C.Rcw, C.Pcw);
    return C;
}

// vikit PinholeCamera::world2cam(xyz_c), the distortion branch included.
SEL_HD void vio_world2cam(const CamIntrinsics& P, const double* xyz, double* px) {
    const double u = xyz[0] / xyz[2], v = xyz[1] / xyz[2];  // project2d
    if (!P.distortion) {
        px[0] = P.fx * u + P.cx;
        px[1] = P.fy * v + P.cy;
        return;
    }
    const double x = u, y = v;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = 1 + P.d[0] * r2 + P.d[1] * r4 + P.d[4] * r6;
    const double xd = x * cdist + P.d[2] * a1 + P.d[3] * a2;
    const double yd = y * cdist + P.d[2] * a3 + P.d[3] * a1;
    px[0] = xd * P.fx + P.cx;
    px[1] = yd * P.fy + P.cy;
}

enum RgbFate : int { kRgbKept = 0, kRgbBehind = 1, kRgbOutOfFrame = 2 };

// Six image bytes from flat offset o (two neighbouring BGR pixels).  Inside the
// buffer they are fetched as one 4-byte and one 2-byte read; a byte outside
// [0, nbytes) reads as 0 and sets edge.
SEL_HD void rgb_span(const uint8_t* img, int64_t nbytes, int64_t o, float* I, bool& edge) {
    if (o >= 0 && o + 6 <= nbytes) {
        uint32_t a;
        uint16_t b;
        memcpy(&a, img + o, 4);
        memcpy(&b, img + o + 4, 2);
        I[0] = (float)(a & 255u);
        I[1] = (float)((a >> 8) & 255u);
        I[2] = (float)((a >> 16) & 255u);
        I[3] = (float)(a >> 24);
        I[4] = (float)(b & 255u);
        I[5] = (float)(b >> 8);
        return;
    }
    for (int k = 0; k < 6; k++) {
        const bool in = o + k >= 0 && o + k < nbytes;
        I[k] = in ? (float)img[o + k] : 0.0f;
        edge = edge || !in;
    }
}

// One point of publish_frame_world_rgb (laser_mapping.cpp:1361-1381) from its
// world coordinates as the published cloud holds them (floats): w2f, the
// p_cam.z > 0 test (a NaN fails it), w2c, isInFrame(pc.cast<int>(), 0) taken in
// double (the same answers wherever the cast is defined), then
// LidarSelector::getpixel (lidar_selection.cpp:1004-1022) on the 8-bit BGR
// image as a flat byte array of 3 * w * h bytes: the row wraps of u in (-1, 0)
// and [w - 1, w) read the neighbouring row as the reference does; taps outside
// the buffer (undefined there) read 0 and set edge.  rgba: r | g << 8 | b << 16
// | 255 << 24, the channels truncated as pointRGB.r = pixel[2] does.
SEL_HD int rgb_point(const FrameCam& C, const uint8_t* img, float wx, float wy, float wz, uint32_t& rgba, bool& edge) {
    rgba = 0u;
    edge = false;
    const double pw[3] = {(double)wx, (double)wy, (double)wz};  // V3D p_w(p.x, p.y, p.z)
    double pf[3], pc[2];
    cam_w2f(C.Rcw, C.Pcw, pw, pf);
    if (!(pf[2] > 0)) return kRgbBehind;
    vio_world2cam(C, pf, pc);
    if (!(pc[0] > -1.0 && pc[0] < (double)C.w && pc[1] > -1.0 && pc[1] < (double)C.h)) return kRgbOutOfFrame;
    const float u_ref = (float)pc[0], v_ref = (float)pc[1];
    const int u_ref_i = (int)floorf(u_ref), v_ref_i = (int)floorf(v_ref);
    const float su = u_ref - (float)u_ref_i, sv = v_ref - (float)v_ref_i;
    const float w_tl = (float)((1.0 - su) * (1.0 - sv)), w_tr = (float)(su * (1.0 - sv)),
                w_bl = (float)((1.0 - su) * sv), w_br = su * sv;
    const int64_t row = 3 * (int64_t)C.w, nbytes = row * C.h;
    const int64_t o = ((int64_t)v_ref_i * C.w + u_ref_i) * 3;
    float T[6], B[6];  // the taps of the upper and the lower row: (tl, tr) and (bl, br), B G R each
    rgb_span(img, nbytes, o, T, edge);
    rgb_span(img, nbytes, o + row, B, edge);
    uint32_t ch[3];
    for (int c = 0; c < 3; c++) {
        const float v = ((w_tl * T[c] + w_tr * T[c + 3]) + w_bl * B[c]) + w_br * B[c + 3];
        ch[c] = (uint32_t)(int)v & 255u;
    }
    rgba = ch[2] | (ch[1] << 8) | (ch[0] << 16) | (255u << 24);
    return kRgbKept;
}

// Ten image bytes from flat offset o of an 8-bit gray image, fetched as the four
// aligned 4-byte words that hold them (img 4-byte aligned, [o & ~3, (o & ~3) + 16)
// inside the buffer).
SEL_HD void vis_row10(const uint8_t* img, int64_t o, int* B) {
    const int64_t a = o & ~(int64_t)3;
    uint32_t d[4];
    memcpy(d, __builtin_assume_aligned(img + a, 4), 16);
    const int s = (int)(o - a) * 8;
    uint64_t lo = (uint64_t)d[0] | ((uint64_t)d[1] << 32), hi = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
    if (s) {
        lo = (lo >> s) | (hi << (64 - s));
        hi >>= s;
    }
    for (int k = 0; k < 8; k++) B[k] = (int)((lo >> (8 * k)) & 255u);
    B[8] = (int)(hi & 255u);
    B[9] = (int)((hi >> 8) & 255u);
}

// vikit's vk::shiTomasiScore(img, u, v) on an 8-bit gray image of w x h, row
// stride w: the smaller eigenvalue of the gradient matrix over the 8 x 8 box
// rows [v-4, v+4), columns [u-4, u+4), central differences, each sum divided by
// 2 * 64.  0 if the box is not inside the image by one pixel.  The sums are
// integers below 2^24 (exact in the reference's floats in any order); the rest
// is float, one rounding per operation, with the final 0.5 * (...) in double as
// the reference's `0.5 *` promotes it.  The discriminant cannot round below
// zero here: s is exact (the sums stay below 2^24), s * s >= 4 dXX dYY, and
// rounding is monotonic.
// vis_score_at takes the image at byte offset `base` of a 4-byte aligned buffer
// (a stored frame of the visual map, whose size need be no multiple of 4).
SEL_HD float vis_score_at(const uint8_t* img, int64_t base, int w, int h, int u, int v) {
    if (u - 4 < 1 || u + 4 >= w - 1 || v - 4 < 1 || v + 4 >= h - 1) return 0.0f;
    int R0[10], R1[10], R2[10];  // rows y - 1, y, y + 1; columns u - 5 .. u + 4
    const int64_t o = base + (int64_t)(v - 5) * w + (u - 5);
    vis_row10(img, o, R0);
    vis_row10(img, o + w, R1);
    int sxx = 0, syy = 0, sxy = 0;
    for (int r = 0; r < 8; r++) {
        vis_row10(img, o + (int64_t)(r + 2) * w, R2);
        for (int k = 1; k < 9; k++) {
            const int dx = R1[k + 1] - R1[k - 1], dy = R2[k] - R0[k];
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
        }
        for (int k = 0; k < 10; k++) {
            R0[k] = R1[k];
            R1[k] = R2[k];
        }
    }
    const float dXX = (float)sxx / 128.0f, dYY = (float)syy / 128.0f, dXY = (float)sxy / 128.0f;
    const float s = dXX + dYY;
    const float t = s * s - 4.0f * (dXX * dYY - dXY * dXY);
    const float r = sqrtf(t);
    return (float)(0.5 * (double)(s - r));
}
SEL_HD float vis_score(const uint8_t* img, int w, int h, int u, int v) { return vis_score_at(img, 0, w, h, u, v); }

// One value of LidarSelector::getpatch (lidar_selection.cpp:117-138): element k =
// x * ps + y of the level's ps x ps patch around pixel pc, x the row.  The
// reference's mixed precision: the anchor floorf((float)(pc / scale)) * scale, the
// sub-pixel offsets in float, w_tl / w_tr / w_bl through `1.0 - ...` in double
// and rounded to float, w_br in float, the four taps summed in float left to
// right.  Every tap must be inside the image: it is for a pc inside
// addSparseMap's border (ps / 2 + 1) * 8.
SEL_HD float vis_getpatch(const uint8_t* img, int w, const double* pc, int ps, int level, int k) {
    const float u_ref = (float)pc[0], v_ref = (float)pc[1];
    const int scale = 1 << level, half = ps / 2;
    const int u_ref_i = (int)(floorf((float)(pc[0] / scale)) * (float)scale);
    const int v_ref_i = (int)(floorf((float)(pc[1] / scale)) * (float)scale);
    const float su = (u_ref - (float)u_ref_i) / (float)scale, sv = (v_ref - (float)v_ref_i) / (float)scale;
    const float w_tl = (float)((1.0 - su) * (1.0 - sv)), w_tr = (float)(su * (1.0 - sv)),
                w_bl = (float)((1.0 - su) * sv), w_br = su * sv;
    const int x = k / ps, y = k - x * ps;
    const uint8_t* p = img + (int64_t)(v_ref_i - half * scale + x * scale) * w + (u_ref_i - half * scale + y * scale);
    return ((w_tl * (float)p[0] + w_tr * (float)p[scale]) + w_bl * (float)p[(int64_t)scale * w]) +
           w_br * (float)p[(int64_t)scale * w + scale];
}

// addSparseMap's grid (lidar_selection.cpp:140-165, reset_grid): cells of
// grid_size pixels, grid_n_height = height / grid_size of them per column,
// length = grid_n_width * grid_n_height in all; border = (ps / 2 + 1) * 8.
struct VisGrid {
    int32_t grid_size, grid_n_height, length, border, ps;
};

enum VisFate : int { kVisOutOfFrame = 0, kVisInFrame = 1, kVisOverflow = 2 };

// One cloud point of addSparseMap's first loop up to its grid index: w2c with no
// p_cam.z test (behind: inside the frame with p_cam.z > 0 false), isInFrame(
// pc.cast<int>(), border) taken in double (a NaN fails it), then index =
// (int)(pc.x / grid_size) * grid_n_height + (int)(pc.y / grid_size), which
// aliases into the next column where height - border > grid_n_height * grid_size;
// kVisOverflow: index >= length, the reference's out-of-bounds write.
SEL_HD int vis_project(const FrameCam& C, const VisGrid& G, float wx, float wy, float wz, double* pc, bool& behind,
                       int& index) {
    const double pw[3] = {(double)wx, (double)wy, (double)wz};  // V3D pt(p.x, p.y, p.z)
    double pf[3];
    cam_w2f(C.Rcw, C.Pcw, pw, pf);
    vio_world2cam(C, pf, pc);
    behind = false;
    index = -1;
    const double b = (double)G.border;
    if (!(pc[0] >= b && pc[0] < (double)(C.w - G.border) && pc[1] >= b && pc[1] < (double)(C.h - G.border)))
        return kVisOutOfFrame;
    behind = !(pf[2] > 0);
    index = (int)(pc[0] / G.grid_size) * G.grid_n_height + (int)(pc[1] / G.grid_size);
    return index >= G.length ? kVisOverflow : kVisInFrame;
}

// One coordinate of AddPoint's VOXEL_KEY (lidar_selection.cpp:195-208), 0.5 m
// voxels: the quotient stored as float, a negative one lowered by 1.0 (in
// double, stored as float again), then truncated: -1.0 m gives -3, not floor's -2.
SEL_HD int64_t vis_voxel_key(float pw) {
    float loc = (float)((double)pw / 0.5);
    if (loc < 0) loc = (float)((double)loc - 1.0);
    return (int64_t)loc;
}

}  // namespace livo
