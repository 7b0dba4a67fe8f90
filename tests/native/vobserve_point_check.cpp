// vobserve_point_check — runs vmap_model.h's addObservation functions (the code
// of k_vm_observe) on the CPU.  Reads one command per line from the file given as
// argv[1]; numbers are C hex floats ("%a"), so every bit survives.  One output
// line per command, in the same notation.
//   P fx fy cx cy w h border Rcw[9] Pcw[3] pos[3]  -> fate pc[2]   (pc 0 0 unless fate is 0)
//   D Rr[9] Pr[3] cpos[3]                          -> delta_p flag
//   X pc[2] px[2]                                  -> pixel_dist flag
//   F cpos[3] n rpos[3n]                           -> index dist[n]
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
        if (cmd == "P") {
            FrameCam C{};
            C.fx = rd(in); C.fy = rd(in); C.cx = rd(in); C.cy = rd(in);
            C.w = (int)rd(in);
            C.h = (int)rd(in);
            const int border = (int)rd(in);
            double pos[3], pc[2] = {0.0, 0.0};
            rdn(in, C.Rcw, 9); rdn(in, C.Pcw, 3); rdn(in, pos, 3);
            const int fate = vm_observe_project(C, border, pos, pc);
            if (fate != kVmObsIn) pc[0] = pc[1] = 0.0;
            printf("P %d %a %a\n", fate, pc[0], pc[1]);
        } else if (cmd == "D") {
            VmFrame ref{};
            double cpos[3];
            rdn(in, ref.Rcw, 9); rdn(in, ref.Pcw, 3); rdn(in, cpos, 3);
            const double d = vm_observe_delta_p(ref, cpos);
            printf("D %a %d\n", d, (int)(d > 0.5));
        } else if (cmd == "X") {
            double pc[2], px[2];
            rdn(in, pc, 2); rdn(in, px, 2);
            const double d = vm_pixel_dist(pc, px);
            printf("X %a %d\n", d, (int)(d > 40.0));
        } else if (cmd == "F") {
            double cpos[3];
            rdn(in, cpos, 3);
            const int n = (int)rd(in);
            std::vector<double> dist((size_t)n);
            for (int k = 0; k < n; k++) {
                double rp[3];
                rdn(in, rp, 3);
                dist[(size_t)k] = vm_view_dist(rp, cpos);
            }
            printf("F %d", vm_furthest_view(dist.data(), n));
            for (int k = 0; k < n; k++) printf(" %a", dist[(size_t)k]);
            printf("\n");
        } else if (!cmd.empty()) {
            return 4;
        }
    }
    free(line);
    fclose(f);
    return 0;
}
