// cam_model.h on the CPU: cam_pose and rgb_point (the per-point function of
// k_rgb_points, rgb_kernels.hip) over the cases tests/test_rgb_cloud_abi.py
// writes, one line per point for the test to compare with its restatement.
//
//   rgb_point_check CASES
// CASES (binary, native endianness): int32 width, height, n; double fx, fy, cx,
// cy, d[5], Rci[9], Pci[3], rot[9], pos[3]; uint8 bgr[3 * width * height];
// float xyz[3 * n] (world points).
// Output: "pose" and the 12 doubles of Rcw, Pcw as hex floats; then per point
// "fate r g b a edge".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cam_model.h"

using namespace livo;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    double cam[9], Rci[9], Pci[3], rot[9], pos[3];
    bool ok = std::fread(hdr, 4, 3, f) == 3 && std::fread(cam, 8, 9, f) == 9 && std::fread(Rci, 8, 9, f) == 9 &&
              std::fread(Pci, 8, 3, f) == 3 && std::fread(rot, 8, 9, f) == 9 && std::fread(pos, 8, 3, f) == 3;
    if (!ok || hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] < 0) return 2;
    const int32_t w = hdr[0], h = hdr[1], n = hdr[2];
    std::vector<uint8_t> img((size_t)3 * w * h);
    std::vector<float> xyz((size_t)3 * n);
    ok = std::fread(img.data(), 1, img.size(), f) == img.size() && std::fread(xyz.data(), 4, xyz.size(), f) == xyz.size();
    std::fclose(f);
    if (!ok) return 2;
    // the camera as livo_cloud_colorize fills it
    livo_vio_params vp{};
    livo_state st{};
    vp.cam.fx = cam[0]; vp.cam.fy = cam[1]; vp.cam.cx = cam[2]; vp.cam.cy = cam[3];
    for (int k = 0; k < 5; k++) vp.cam.d[k] = cam[4 + k];
    vp.cam.width = w;
    vp.cam.height = h;
    for (int k = 0; k < 9; k++) vp.R_ci[k] = Rci[k], st.rot[k] = rot[k];
    for (int k = 0; k < 3; k++) vp.P_ci[k] = Pci[k], st.pos[k] = pos[k];
    const FrameCam C = frame_cam(vp, st);
    std::printf("pose");
    for (int k = 0; k < 9; k++) std::printf(" %a", C.Rcw[k]);
    for (int k = 0; k < 3; k++) std::printf(" %a", C.Pcw[k]);
    std::printf("\n");
    for (int32_t i = 0; i < n; i++) {
        uint32_t rgba;
        bool edge;
        const int fate = rgb_point(C, img.data(), xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], rgba, edge);
        std::printf("%d %u %u %u %u %d\n", fate, rgba & 255u, (rgba >> 8) & 255u, (rgba >> 16) & 255u, rgba >> 24,
                    edge ? 1 : 0);
    }
    return 0;
}
