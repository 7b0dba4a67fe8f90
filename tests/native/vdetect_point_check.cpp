// vdetect_point_check — runs on the CPU the functions that livo_vio_detect's small
// kernels share with the host path (vmap_model.h): the stored frame of a state
// (k_vm_frame, livo_vmap_add_frame) and a selected record's new point with its
// observation (k_vm_fresh, livo_vmap_add).  Reads one command per line from the
// file given as argv[1]; numbers are C hex floats ("%a"), so every bit survives.
//   F id fx fy cx cy w h Rci[9] Pci[3] rot[9] pos[3]  -> id Rcw[9] Pcw[3] pos[3]
//   N fx fy cx cy frame_id slot x y z score u v       -> pos[3] value n_obs voxel[3] frame_id level slot px[2] f[3]
//     (x, y, z, score are rounded to float; the record's voxel key is vis_voxel_key of them, as the select writes it)
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>

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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char* line = nullptr;
    size_t cap = 0;
    while (getline(&line, &cap, f) > 0) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "F") {
            const int id = (int)rd(in);
            livo_vio_params p{};
            livo_state s{};
            p.cam.fx = rd(in); p.cam.fy = rd(in); p.cam.cx = rd(in); p.cam.cy = rd(in);
            p.cam.width = (int)rd(in);
            p.cam.height = (int)rd(in);
            rdn(in, p.R_ci, 9); rdn(in, p.P_ci, 3); rdn(in, s.rot, 9); rdn(in, s.pos, 3);
            const VmFrame fr = vm_make_frame(id, frame_cam(p, s));
            printf("F %d", fr.id);
            for (int k = 0; k < 9; k++) printf(" %a", fr.Rcw[k]);
            for (int k = 0; k < 3; k++) printf(" %a", fr.Pcw[k]);
            for (int k = 0; k < 3; k++) printf(" %a", fr.pos[k]);
            printf("\n");
        } else if (cmd == "N") {
            CamIntrinsics K{};
            K.fx = rd(in); K.fy = rd(in); K.cx = rd(in); K.cy = rd(in);
            const int frame_id = (int)rd(in), slot = (int)rd(in);
            livo_vis_point r{};
            r.x = (float)rd(in); r.y = (float)rd(in); r.z = (float)rd(in);
            r.score = (float)rd(in);
            r.u = rd(in); r.v = rd(in);
            r.voxel[0] = vis_voxel_key(r.x); r.voxel[1] = vis_voxel_key(r.y); r.voxel[2] = vis_voxel_key(r.z);
            const VmPoint q = vm_make_point(r);
            const VmObs o = vm_make_obs(K, frame_id, slot, 0, r.u, r.v);
            printf("N %a %a %a %a %d %lld %lld %lld %d %d %d %a %a %a %a %a\n", q.pos[0], q.pos[1], q.pos[2],
                   (double)q.value, q.n_obs, (long long)q.voxel[0], (long long)q.voxel[1], (long long)q.voxel[2],
                   o.frame_id, o.level, o.slot, o.px[0], o.px[1], o.f[0], o.f[1], o.f[2]);
        } else if (!cmd.empty()) {
            return 4;
        }
    }
    free(line);
    fclose(f);
    return 0;
}
