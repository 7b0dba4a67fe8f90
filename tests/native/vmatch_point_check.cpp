// vmatch_point_check — runs vmap_model.h's per-item functions (the code of the
// livo_vio_match kernels) on the CPU.  Reads one command per line from the file
// given as argv[1]; numbers are C hex floats ("%a"), so every bit survives.  One
// output line per command, in the same notation.
//   I w h path                 load an 8-bit gray image (raw bytes)
//   A fx fy cx cy Rc[9] Pc[3] Rr[9] Pr[3] px[2] pos[3] half
//                              -> f[3] A[4] det level Ai[4] (floats) ref_pos[3]
//   L a00 a01 a10 a11          -> level
//   S Ai[4] px[2] level ps e   -> the warped sample (needs I)
//   N n ref[n] cur[n]          -> ncc error
//   C fx fy cx cy w h border Rcw[9] Pcw[3] x y z (floats)
//                              -> key[3] hit pix depth  px_cloud px_w2c
//   K x (float)                -> AddPoint's key, the floor key
//   M fx fy cx cy w h ps grid Rcw[9] Pcw[3] pos[3]
//                              -> fate index dist pc[2] z bid
//   V fpos[3] pos[3] n rpos[3n] -> best cosine
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "vmap_model.h"

using namespace livo;

static double rd(std::istringstream& in) {
    std::string t;
    in >> t;
    return strtod(t.c_str(), nullptr);
}
static void rdn(std::istringstream& in, double* v, int n) {
    for (int k = 0; k < n; k++) v[k] = rd(in);
}

static FrameCam read_cam(std::istringstream& in, bool size) {
    FrameCam C{};
    C.fx = rd(in); C.fy = rd(in); C.cx = rd(in); C.cy = rd(in);
    if (size) {
        C.w = (int)rd(in);
        C.h = (int)rd(in);
    }
    return C;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<uint8_t> img;
    int iw = 0, ih = 0;
    char* line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "I") {
            std::string path;
            in >> iw >> ih >> path;
            img.resize((size_t)iw * ih);
            FILE* g = fopen(path.c_str(), "rb");
            if (!g || fread(img.data(), 1, img.size(), g) != img.size()) return 3;
            fclose(g);
            printf("I\n");
        } else if (cmd == "A") {
            FrameCam C = read_cam(in, false);
            VmFrame ref{};
            VmObs o{};
            double pos[3];
            rdn(in, C.Rcw, 9); rdn(in, C.Pcw, 3); rdn(in, ref.Rcw, 9); rdn(in, ref.Pcw, 3);
            rdn(in, o.px, 2); rdn(in, pos, 3);
            const int half = (int)rd(in);
            vm_frame_pos(ref.Rcw, ref.Pcw, ref.pos);
            vm_cam2world(C, o.px[0], o.px[1], o.f);
            double A[4];
            vm_warp_matrix(C, ref, o, pos, half, A);
            float Ai[4];
            vm_inverse2f(A, Ai);
            printf("A %a %a %a %a %a %a %a %a %d %a %a %a %a %a %a %a\n", o.f[0], o.f[1], o.f[2], A[0], A[1], A[2], A[3],
                   vm_det2(A), vm_search_level(A, 2), (double)Ai[0], (double)Ai[1], (double)Ai[2], (double)Ai[3],
                   ref.pos[0], ref.pos[1], ref.pos[2]);
        } else if (cmd == "L") {
            double A[4];
            rdn(in, A, 4);
            printf("L %d\n", vm_search_level(A, 2));
        } else if (cmd == "S") {
            double a[4], px[2];
            rdn(in, a, 4); rdn(in, px, 2);
            const float Ai[4] = {(float)a[0], (float)a[1], (float)a[2], (float)a[3]};
            const int level = (int)rd(in), ps = (int)rd(in), e = (int)rd(in);
            printf("S %a\n", (double)vm_warp_sample(Ai, px, level, ps, e, img.data(), iw, ih));
        } else if (cmd == "N") {
            const int n = (int)rd(in);
            std::vector<float> a((size_t)n), b((size_t)n);
            for (float& v : a) v = (float)rd(in);
            for (float& v : b) v = (float)rd(in);
            printf("N %a %a\n", vm_ncc(a.data(), b.data(), n), (double)vm_error(a.data(), b.data(), n));
        } else if (cmd == "C") {
            FrameCam C = read_cam(in, true);
            const int border = (int)rd(in);
            rdn(in, C.Rcw, 9); rdn(in, C.Pcw, 3);
            const float x = (float)rd(in), y = (float)rd(in), z = (float)rd(in);
            int64_t key[3], pix = -1;
            float depth = 0.0f;
            const bool hit = vm_cloud_point(C, border, x, y, z, key, pix, depth);
            const double pw[3] = {(double)x, (double)y, (double)z};
            double pf[3], pc[2];
            cam_w2f(C.Rcw, C.Pcw, pw, pf);
            vio_world2cam(C, pf, pc);
            printf("C %lld %lld %lld %d %lld %a %a %a\n", (long long)key[0], (long long)key[1], (long long)key[2],
                   (int)hit, (long long)pix, (double)depth, C.fx * pf[0] / pf[2] + C.cx, pc[0]);
        } else if (cmd == "K") {
            const float x = (float)rd(in);
            const double q = floor((double)x / 0.5);
            printf("K %lld %lld\n", (long long)vis_voxel_key(x), (long long)q);
        } else if (cmd == "M") {
            FrameCam C = read_cam(in, true);
            VisGrid G{};
            G.ps = (int)rd(in);
            G.grid_size = (int)rd(in);
            G.border = (G.ps / 2 + 1) * 8;
            G.grid_n_height = C.h / G.grid_size;
            G.length = (C.w / G.grid_size) * G.grid_n_height;
            double pos[3], fpos[3], pf[3] = {0, 0, 0}, pc[2] = {0, 0};
            rdn(in, C.Rcw, 9); rdn(in, C.Pcw, 3); rdn(in, pos, 3);
            vm_frame_pos(C.Rcw, C.Pcw, fpos);
            int index = -1;
            float dist = 0.0f;
            const int fate = vm_map_point(C, G, fpos, pos, pf, pc, index, dist);
            printf("M %d %d %a %a %a %a %llu\n", fate, index, (double)dist, pc[0], pc[1], pf[2],
                   (unsigned long long)vm_bid(dist, 7u));
        } else if (cmd == "V") {
            double fpos[3], pos[3];
            rdn(in, fpos, 3); rdn(in, pos, 3);
            const int n = (int)rd(in);
            std::vector<VmFrame> frames((size_t)n);
            std::vector<VmObs> obs((size_t)n);
            for (int k = 0; k < n; k++) {
                rdn(in, frames[(size_t)k].pos, 3);
                obs[(size_t)k].slot = k;
            }
            double cosine = -1.0;
            const int best = vm_close_view(fpos, pos, obs.data(), n, frames.data(), cosine);
            printf("V %d %a\n", best, cosine);
        } else if (!cmd.empty()) {
            return 4;
        }
    }
    free(line);
    fclose(f);
    return 0;
}
