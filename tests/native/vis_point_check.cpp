// cam_model.h on the CPU: vis_score, vis_getpatch and vis_voxel_key (the
// per-point functions of k_vis_score / k_vis_emit, vis_kernels.hip) over the
// cases tests/test_vis_select_abi.py writes, for the test to compare with its
// restatement bit for bit.
//
//   vis_point_check CASES
// CASES (binary, native endianness): int32 width, height, patch_size, n_score,
// n_patch, n_key; uint8 gray[width * height]; int32 uv[2 * n_score]; double
// pc[2 * n_patch]; float w[n_key].
// Output: per score case "s <score bits>"; per patch case "p" and the 3 *
// patch_size^2 values' bits; per key case "k <key>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cam_model.h"

using namespace livo;

static unsigned bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[6];
    if (std::fread(hdr, 4, 6, f) != 6) return 2;
    const int32_t w = hdr[0], h = hdr[1], ps = hdr[2], ns = hdr[3], np = hdr[4], nk = hdr[5];
    if (w <= 0 || h <= 0 || ps < 1 || ps > 8 || ns < 0 || np < 0 || nk < 0) return 2;
    // (16-byte aligned storage, and slack for nothing: every read stays inside the image)
    std::vector<uint32_t> store(((size_t)w * h + 3) / 4);
    uint8_t* img = reinterpret_cast<uint8_t*>(store.data());
    std::vector<int32_t> uv((size_t)2 * ns);
    std::vector<double> pc((size_t)2 * np);
    std::vector<float> key((size_t)nk);
    const bool ok = std::fread(img, 1, (size_t)w * h, f) == (size_t)w * h &&
                    std::fread(uv.data(), 4, uv.size(), f) == uv.size() &&
                    std::fread(pc.data(), 8, pc.size(), f) == pc.size() &&
                    std::fread(key.data(), 4, key.size(), f) == key.size();
    std::fclose(f);
    if (!ok) return 2;
    for (int32_t i = 0; i < ns; i++) std::printf("s %u\n", bits(vis_score(img, w, h, uv[2 * i], uv[2 * i + 1])));
    for (int32_t i = 0; i < np; i++) {
        std::printf("p");
        for (int level = 0; level < 3; level++)
            for (int k = 0; k < ps * ps; k++)
                std::printf(" %u", bits(vis_getpatch(img, w, &pc[2 * i], ps, level, k)));
        std::printf("\n");
    }
    for (int32_t i = 0; i < nk; i++) std::printf("k %lld\n", (long long)vis_voxel_key(key[i]));
    return 0;
}
