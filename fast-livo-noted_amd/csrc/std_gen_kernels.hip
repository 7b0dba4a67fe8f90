// std_gen_kernels.hip — CDNA4 (gfx950) kernels of STDescManager::GenerateSTDescs
// (include/STD/STDesc.cpp:264-297: init_voxel_map :376-422, init_plane :1367-1409, getPlane
// :492-507, build_connection :424-490, corner_extractor :509-617, extract_corner :619-781,
// non_maxi_suppression :783-822, build_stdesc :824-958).  DESIGN.md §8.17 has the four pinned
// choices (visiting order, normal sign, ties at the cut, missing neighbours).
//
//   k_gen_keys       a point's voxel key, (int64)(double(p) / voxel_size) with 1.0 taken off a
//       negative quotient, 21 bits an axis; the host sorts (key, input index) stably.
//   k_gen_heads / k_gen_voxels / k_gen_rank   the points gathered in sorted order, a voxel's
//       run, its first input index (the visiting order is the sort by it) and its rank.
//   k_gen_plane      init_plane, one thread a voxel: sums in input order, a cyclic Jacobi
//       eigen-solve of the 3 x 3 covariance, the normal with its largest component positive.
//   k_gen_connect    build_connection as a gather: connect_, is_check_connect_ and the
//       neighbour's index per voxel and direction.
//   k_gen_jobs<EMIT> the jobs (V, i) in visiting order, then i.
//   k_gen_members    one wave per non-plane voxel W: the greedy walk over its candidate jobs in
//       job order (a 27-way merge of the job ranges of the voxels round W).
//   k_gen_extract    extract_corner, one block a job: bounding box, cell counts in LDS
//       (integer atomics), the maximum of each 5 x 5 segment, and a winner cell's coordinate
//       sums by one thread in point order, as the reference adds them.
//   k_gen_concat / k_gen_nms / k_gen_keep / k_gen_pick   corners in job order, suppression
//       (one wave a corner), the survivors compacted, the cut's gather.
//   k_gen_knn / k_gen_cand / k_gen_surv / k_gen_emit   build_stdesc: brute-force k-NN, one
//       thread a (i, m, n) candidate, first-come de-duplication through a sort of (key,
//       candidate index), the survivors as livo_std_desc records in candidate order.
//
// Every store is a plain vector store; the only atomics are integer ones (LDS cell counts,
// error flags).  Numerics: -ffp-contract=off, correctly rounded sqrt and division, every sum in
// the restatement's order (tests/std_gen_cases.py).
#include <hip/hip_runtime.h>
#include <math.h>

#include "livo_internal.h"

namespace livo {

static_assert(sizeof(livo_std_corner) == 32, "corner");
constexpr int kGenBlock = 256;
constexpr int kGenWaves = kGenBlock / 64;
constexpr uint32_t kGenNone = 0xFFFFFFFFu;
constexpr unsigned long long kGenNoKey = ~0ull;

__device__ __forceinline__ unsigned long long gen_pack(long long x, long long y, long long z) {
    return ((unsigned long long)(x + kStdCellBias) << 42) | ((unsigned long long)(y + kStdCellBias) << 21) |
           (unsigned long long)(z + kStdCellBias);
}
__device__ __forceinline__ void gen_unpack(unsigned long long k, long long* x, long long* y, long long* z) {
    *x = (long long)((k >> 42) & 0x1FFFFFull) - kStdCellBias;
    *y = (long long)((k >> 21) & 0x1FFFFFull) - kStdCellBias;
    *z = (long long)(k & 0x1FFFFFull) - kStdCellBias;
}

// the voxel of a key: its index in the sorted keys, kGenNone where there is none
__device__ __forceinline__ uint32_t gen_find(const unsigned long long* __restrict__ vkey, uint32_t nv,
                                             unsigned long long key) {
    uint32_t lo = 0, hi = nv;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (vkey[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < nv && vkey[lo] == key) ? lo : kGenNone;
}

__device__ __forceinline__ double gen_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// |a - b| < thre or |a + b| < thre (:464-471, :569-573)
__device__ __forceinline__ bool gen_same_normal(const double* a, const double* b, double thre) {
    const double d = gen_norm3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
    const double s = gen_norm3(a[0] + b[0], a[1] + b[1], a[2] + b[2]);
    return d < thre || s < thre;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_keys(const StdGen g) {
    const int64_t i = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (i >= g.n) return;
    long long c[3] = {0, 0, 0};
    unsigned err = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float p = g.pts[i * 3 + k];
        if (!isfinite(p)) {
            err |= 1u;
            continue;
        }
        double q = (double)p / g.prm.voxel_size;
        if (q < 0) q -= 1.0;
        if (!(q > -(double)kStdGenCoordMax && q < (double)kStdGenCoordMax)) {
            err |= 2u;
            continue;
        }
        c[k] = (long long)q;
    }
    if (err) atomicOr(g.ctr + kGenCtrErr, err);
    g.pkey[i] = err ? 0ull : gen_pack(c[0], c[1], c[2]);
    g.piota[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_heads(const StdGen g) {
    const int64_t i = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (i >= g.n) return;
    g.head[i] = (i == 0 || g.skey[i] != g.skey[i - 1]) ? 1u : 0u;
    const int64_t s = g.sidx[i];
#pragma unroll
    for (int k = 0; k < 3; k++) g.spts[i * 3 + k] = g.pts[s * 3 + k];
}

__global__ __launch_bounds__(kGenBlock) void k_gen_voxels(const StdGen g) {
    const int64_t i = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t v = g.hpos[i];
    if (g.head[i]) {
        g.vkey[v] = g.skey[i];
        g.vstart[v] = (uint32_t)i;
        g.vfirst[v] = g.sidx[i];  // (the sort is stable: a run is in input order)
        g.viota[v] = v;
    }
    if (i == g.n - 1) g.vstart[v + g.head[i]] = (uint32_t)g.n;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_rank(const StdGen g) {
    const int64_t r = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (r < g.nv) g.rank[g.order[r]] = (uint32_t)r;
}

// One Jacobi rotation of the symmetric a that zeroes a[P][Q]; R is the third index.
template <int P, int Q, int R>
__device__ __forceinline__ void gen_rotate(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

__global__ __launch_bounds__(kGenBlock) void k_gen_plane(const StdGen g) {
    const int64_t v = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (v >= g.nv) return;
    const uint32_t b = g.vstart[v], e = g.vstart[v + 1];
    uint32_t plane = 0u;
    double nrm[3] = {0, 0, 0}, cen[3] = {0, 0, 0};
    if ((int64_t)(e - b) > (int64_t)g.prm.voxel_init_num) {
        double a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (uint32_t i = b; i < e; i++) {
            const double p[3] = {(double)g.spts[(int64_t)i * 3], (double)g.spts[(int64_t)i * 3 + 1],
                                 (double)g.spts[(int64_t)i * 3 + 2]};
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) a[r][c] += p[r] * p[c];
                cen[r] += p[r];
            }
        }
        const double cnt = (double)(e - b);
#pragma unroll
        for (int r = 0; r < 3; r++) cen[r] = cen[r] / cnt;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) a[r][c] = a[r][c] / cnt - cen[r] * cen[c];
        double w[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int sweep = 0; sweep < kStdGenSweeps; sweep++) {
            gen_rotate<0, 1, 2>(a, w);
            gen_rotate<0, 2, 1>(a, w);
            gen_rotate<1, 2, 0>(a, w);
        }
        // the least eigenvalue, the first of equal ones
        double ev = a[0][0];
        nrm[0] = w[0][0], nrm[1] = w[1][0], nrm[2] = w[2][0];
        if (a[1][1] < ev) ev = a[1][1], nrm[0] = w[0][1], nrm[1] = w[1][1], nrm[2] = w[2][1];
        if (a[2][2] < ev) ev = a[2][2], nrm[0] = w[0][2], nrm[1] = w[1][2], nrm[2] = w[2][2];
        if (ev < g.prm.plane_detection_thre) {
            plane = 1u;
            // pin 2: the component of largest magnitude is positive, the first of equal ones
            double big = nrm[0];
            if (fabs(nrm[1]) > fabs(big)) big = nrm[1];
            if (fabs(nrm[2]) > fabs(big)) big = nrm[2];
            if (big < 0) nrm[0] = -nrm[0], nrm[1] = -nrm[1], nrm[2] = -nrm[2];
        }
    }
    g.vplane[v] = plane;
    g.pflag[g.rank[v]] = plane;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        g.vnorm[v * 3 + k] = plane ? nrm[k] : 0.0;
        g.vcen[v * 3 + k] = plane ? cen[k] : 0.0;
    }
}

__global__ __launch_bounds__(kGenBlock) void k_gen_planes_out(const StdGen g) {
    const int64_t r = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (r >= g.nv || !g.pflag[r]) return;
    const int64_t v = g.order[r];
    livo_std_plane o;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.xyz[k] = (float)g.vcen[v * 3 + k];
        o.normal[k] = (float)g.vnorm[v * 3 + k];
    }
    g.planes_out[g.ppos[r]] = o;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_connect(const StdGen g) {
    const int64_t v = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (v >= g.nv) return;
    long long x, y, z;
    gen_unpack(g.vkey[v], &x, &y, &z);
    const bool plane = g.vplane[v] != 0u;
    double n0[3] = {g.vnorm[v * 3], g.vnorm[v * 3 + 1], g.vnorm[v * 3 + 2]};
    uint32_t mask = 0u;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const long long d = i < 3 ? 1 : -1;
        const int ax = i % 3;
        const uint32_t nb = gen_find(g.vkey, (uint32_t)g.nv, gen_pack(x + (ax == 0 ? d : 0), y + (ax == 1 ? d : 0),
                                                                      z + (ax == 2 ? d : 0)));
        g.cidx[v * 6 + i] = nb;
        if (plane) mask |= 0x100u << i;  // checked, whether the neighbour exists or not
        if (nb == kGenNone) continue;
        const bool nplane = g.vplane[nb] != 0u;
        if (plane && nplane) {
            const double n1[3] = {g.vnorm[(int64_t)nb * 3], g.vnorm[(int64_t)nb * 3 + 1], g.vnorm[(int64_t)nb * 3 + 2]};
            if (gen_same_normal(n0, n1, g.prm.plane_merge_normal_thre)) mask |= 1u << i;
        } else if (!plane && nplane) {
            mask |= (1u | 0x100u) << i;  // written by the plane neighbour (:481-483)
        }
    }
    g.conn[v] = mask;
}

// The jobs of the voxel of rank r: V is no plane and has more than 10 points, connect_[i], and the
// connected plane voxel has a connected plane of its own (:529-552).
template <bool EMIT>
__global__ __launch_bounds__(kGenBlock) void k_gen_jobs(const StdGen g) {
    const int64_t r = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (r >= g.nv) return;
    const int64_t v = g.order[r];
    uint32_t cnt = 0u;
    if (!g.vplane[v] && g.vstart[v + 1] - g.vstart[v] > 10u) {
        const uint32_t mask = g.conn[v];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (!(mask >> i & 1u)) continue;
            const uint32_t c = g.cidx[v * 6 + i];
            const uint32_t cm = g.conn[c];
            if (!((cm >> 8) & cm & 0x3Fu)) continue;
            if (EMIT) {
                g.job_v[g.jpos[r] + cnt] = (uint32_t)v;
                g.job_c[g.jpos[r] + cnt] = c;
            }
            cnt++;
        }
    }
    if (!EMIT) g.jcnt[r] = cnt;
}

// One wave (a block of 64) per voxel W.  Lane l < 27 holds the job range of V = W - voxel_round[l],
// in whose round W sits at slot l.  The jobs that reach W come out of the 27 ranges in ascending
// job index; W joins a job unless a job it joined before has a normal within 0.5 (:565-584).
__global__ __launch_bounds__(64) void k_gen_members(const StdGen g) {
    __shared__ double acc[kStdGenReach][3];
    const int64_t w = blockIdx.x;
    const int lane = threadIdx.x;
    if (g.vplane[w]) return;
    uint32_t a = 0u, b = 0u;
    if (lane < 27) {
        long long x, y, z;
        gen_unpack(g.vkey[w], &x, &y, &z);
        const uint32_t v = gen_find(g.vkey, (uint32_t)g.nv, gen_pack(x - (lane / 9 - 1), y - (lane / 3 % 3 - 1), z - (lane % 3 - 1)));
        if (v != kGenNone) {
            const uint32_t r = g.rank[v];
            a = g.jpos[r];
            b = a + g.jcnt[r];
        }
    }
    int nacc = 0;
    for (;;) {
        const uint32_t cur = a < b ? a : kGenNone;
        uint32_t j = cur;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)j, off);
            j = o < j ? o : j;
        }
        if (j == kGenNone) break;
        const int slot = __ffsll((long long)__ballot(cur == j)) - 1;
        if (lane == slot) a++;
        const int64_t c = g.job_c[j];
        const double n[3] = {g.vnorm[c * 3], g.vnorm[c * 3 + 1], g.vnorm[c * 3 + 2]};
        bool skip = false;
        for (int k = lane; k < nacc; k += 64) skip = skip || gen_same_normal(n, acc[k], 0.5);
        if (__ballot(skip) != 0ull) continue;
        __syncthreads();  // (one wave: the reads of acc above end before lane 0 writes)
        if (lane == 0) {
            if (nacc < kStdGenReach) acc[nacc][0] = n[0], acc[nacc][1] = n[1], acc[nacc][2] = n[2];
            g.jslot[(int64_t)j * 27 + slot] = (uint32_t)w + 1u;
        }
        nacc++;
        __syncthreads();
    }
}

// extract_corner's plane frame and projection (:627-676)
struct GenFrame {
    double A, B, C, D, xa[3], ya[3], dx, dy, cen[3];
};
__device__ __forceinline__ GenFrame gen_frame(const double* nrm, const double* cen) {
    GenFrame f;
    f.A = nrm[0], f.B = nrm[1], f.C = nrm[2];
    f.D = -((f.A * cen[0] + f.B * cen[1]) + f.C * cen[2]);
    double x[3] = {1.0, 1.0, 0.0};
    if (f.C != 0) {
        x[2] = -(f.A + f.B) / f.C;
    } else if (f.B != 0) {
        x[1] = -f.A / f.B;
    } else {
        x[0] = 0.0;
        x[1] = 1.0;
    }
    const double xn = gen_norm3(x[0], x[1], x[2]);
    if (xn > 0)
        for (int k = 0; k < 3; k++) x[k] = x[k] / xn;
    double y[3] = {f.B * x[2] - f.C * x[1], f.C * x[0] - f.A * x[2], f.A * x[1] - f.B * x[0]};
    const double yn = gen_norm3(y[0], y[1], y[2]);
    if (yn > 0)
        for (int k = 0; k < 3; k++) y[k] = y[k] / yn;
    for (int k = 0; k < 3; k++) f.xa[k] = x[k], f.ya[k] = y[k], f.cen[k] = cen[k];
    f.dx = -((x[0] * cen[0] + x[1] * cen[1]) + x[2] * cen[2]);
    f.dy = -((y[0] * cen[0] + y[1] * cen[1]) + y[2] * cen[2]);
    return f;
}
__device__ __forceinline__ bool gen_project(const GenFrame& f, const float* __restrict__ p, double dmin, double dmax,
                                            double* px, double* py) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double A = f.A, B = f.B, C = f.C, D = f.D;
    const double dis = fabs(((x * A + y * B) + z * C) + D);
    if (dis < dmin || dis > dmax) return false;
    const double q = (A * A + B * B) + C * C;
    const double c0 = (-A * ((B * y + C * z) + D) + x * (B * B + C * C)) / q;
    const double c1 = (-B * ((A * x + C * z) + D) + y * (A * A + C * C)) / q;
    const double c2 = (-C * ((A * x + B * y) + D) + z * (A * A + B * B)) / q;
    *px = ((c0 * f.ya[0] + c1 * f.ya[1]) + c2 * f.ya[2]) + f.dy;
    *py = ((c0 * f.xa[0] + c1 * f.xa[1]) + c2 * f.xa[2]) + f.dx;
    return true;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_extract(const StdGen g) {
    __shared__ int img[kStdGenSide * kStdGenSide];
    __shared__ double red[kGenWaves][4];
    __shared__ int redn[kGenWaves];
    __shared__ uint32_t sb[27], se[27];
    __shared__ unsigned char win[kGenBlock];
    const int64_t j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < 27) {
        const uint32_t w = g.jslot[j * 27 + tid];
        sb[tid] = w ? g.vstart[w - 1] : 0u;
        se[tid] = w ? g.vstart[w] : 0u;
    }
    const int64_t c = g.job_c[j];
    const double nrm[3] = {g.vnorm[c * 3], g.vnorm[c * 3 + 1], g.vnorm[c * 3 + 2]};
    const double cen[3] = {g.vcen[c * 3], g.vcen[c * 3 + 1], g.vcen[c * 3 + 2]};
    const GenFrame f = gen_frame(nrm, cen);
    const double res = g.prm.proj_image_resolution, dmin = g.prm.proj_dis_min, dmax = g.prm.proj_dis_max;
    __syncthreads();
    // the bounding box from +-10 and the count of the projected points (:681-693)
    double mnx = 10, mxx = -10, mny = 10, mxy = -10;
    int cnt = 0;
    for (int s = 0; s < 27; s++)
        for (uint32_t i = sb[s] + tid; i < se[s]; i += kGenBlock) {
            double px, py;
            if (!gen_project(f, g.spts + (int64_t)i * 3, dmin, dmax, &px, &py)) continue;
            cnt++;
            mnx = px < mnx ? px : mnx;
            mxx = px > mxx ? px : mxx;
            mny = py < mny ? py : mny;
            mxy = py > mxy ? py : mxy;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double a = __shfl_xor(mnx, off), b = __shfl_xor(mxx, off), cc = __shfl_xor(mny, off), d = __shfl_xor(mxy, off);
        mnx = a < mnx ? a : mnx;
        mxx = b > mxx ? b : mxx;
        mny = cc < mny ? cc : mny;
        mxy = d > mxy ? d : mxy;
        cnt += __shfl_xor(cnt, off);
    }
    if (lane == 0) red[wv][0] = mnx, red[wv][1] = mxx, red[wv][2] = mny, red[wv][3] = mxy, redn[wv] = cnt;
    __syncthreads();
    cnt = 0;
#pragma unroll
    for (int k = 0; k < kGenWaves; k++) {
        mnx = red[k][0] < mnx ? red[k][0] : mnx;
        mxx = red[k][1] > mxx ? red[k][1] : mxx;
        mny = red[k][2] < mny ? red[k][2] : mny;
        mxy = red[k][3] > mxy ? red[k][3] : mxy;
        cnt += redn[k];
    }
    if (tid == 0) g.jpts[j] = (uint32_t)cnt;
    if (cnt <= 5) {
        if (tid == 0) g.ccnt[j] = 0u;
        return;
    }
    const double seglen = 5 * res;
    const int nxs = (int)((mxx - mnx) / seglen + 1), nys = (int)((mxy - mny) / seglen + 1);
    const int xlen = (int)((mxx - mnx) / res + 5), ylen = (int)((mxy - mny) / res + 5);
    // (the limits livo_std_generate checks keep the image inside the side and the segments inside
    // the block and the corner slots; a job that broke them would be counted, not run)
    if (xlen > kStdGenSide || ylen > kStdGenSide || nxs * nys > kGenBlock || nxs * nys > g.seg_max || nxs * 5 > xlen ||
        nys * 5 > ylen) {
        if (tid == 0) {
            g.ccnt[j] = 0u;
            atomicOr(g.ctr + kGenCtrErr, 4u);
        }
        return;
    }
    for (int i = tid; i < xlen * kStdGenSide; i += kGenBlock) img[i] = 0;
    __syncthreads();
    for (int s = 0; s < 27; s++)
        for (uint32_t i = sb[s] + tid; i < se[s]; i += kGenBlock) {
            double px, py;
            if (!gen_project(f, g.spts + (int64_t)i * 3, dmin, dmax, &px, &py)) continue;
            const int xi = (int)((px - mnx) / res), yi = (int)((py - mny) / res);
            if (xi >= 0 && xi < xlen && yi >= 0 && yi < ylen) atomicAdd(&img[xi * kStdGenSide + yi], 1);
        }
    __syncthreads();
    // the fullest cell of a 5 x 5 segment, the first of equal ones in x-then-y order (:722-746)
    int best = 0, bx = -1, by = -1;
    if (tid < nxs * nys) {
        const int sx = tid / nys, sy = tid % nys;
        for (int x = sx * 5; x < sx * 5 + 5; x++)
            for (int y = sy * 5; y < sy * 5 + 5; y++) {
                const int v = img[x * kStdGenSide + y];
                if (v > best) best = v, bx = x, by = y;
            }
    }
    const bool mine = best > 0 && (double)best >= g.prm.corner_thre;
    win[tid] = mine ? 1 : 0;
    __syncthreads();
    int pos = 0, total = 0;
    for (int k = 0; k < nxs * nys; k++) {
        pos += k < tid ? win[k] : 0;
        total += win[k];
    }
    if (tid == 0) g.ccnt[j] = (uint32_t)total;
    if (!mine) return;
    // the cell's coordinate sums in point order (:709-715), its mean, and the corner (:760-778)
    double sx = 0, sy = 0;
    for (int s = 0; s < 27; s++)
        for (uint32_t i = sb[s]; i < se[s]; i++) {
            double px, py;
            if (!gen_project(f, g.spts + (int64_t)i * 3, dmin, dmax, &px, &py)) continue;
            const int xi = (int)((px - mnx) / res), yi = (int)((py - mny) / res);
            if (xi == bx && yi == by) sx += px, sy += py;
        }
    const double px = sx / (double)best, py = sy / (double)best;
    livo_std_corner o;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.xyz[k] = (float)((py * f.xa[k] + px * f.ya[k]) + f.cen[k]);
        o.normal[k] = (float)nrm[k];
    }
    o.attached = (float)best;
    o.pad = 0.f;
    g.cbuf[j * g.seg_max + pos] = o;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_concat(const StdGen g) {
    const int64_t t = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (t >= g.nj * g.seg_max) return;
    const int64_t j = t / g.seg_max, k = t % g.seg_max;
    if (k < g.ccnt[j]) g.call[g.cpos[j] + k] = g.cbuf[t];
}

__device__ __forceinline__ float gen_d2(const livo_std_corner& a, const livo_std_corner& b) {
    const float dx = a.xyz[0] - b.xyz[0], dy = a.xyz[1] - b.xyz[1], dz = a.xyz[2] - b.xyz[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// A corner dies if another within the radius is attached to as many points or more (:795-814).
__global__ __launch_bounds__(kGenBlock) void k_gen_nms(const StdGen g) {
    const int64_t i = (int64_t)blockIdx.x * kGenWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= g.m) return;
    const livo_std_corner a = g.call[i];
    const float r2 = (float)(g.prm.non_max_suppression_radius * g.prm.non_max_suppression_radius);
    bool dead = false;
    for (int64_t k = lane; k < g.m; k += 64) {
        if (k == i) continue;
        const livo_std_corner b = g.call[k];
        dead = dead || (gen_d2(a, b) < r2 && a.attached <= b.attached);
    }
    const bool any = __ballot(dead) != 0ull;
    if (lane == 0) g.alive[i] = any ? 0u : 1u;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_keep(const StdGen g) {
    const int64_t i = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (i >= g.m || !g.alive[i]) return;
    const uint32_t p = g.apos[i];
    const livo_std_corner c = g.call[i];
    g.csup[p] = c;
    g.cutkey[p] = 0xFFFFFFFFu - (uint32_t)c.attached;  // pin 3: count descending, then index ascending
    g.cutval[p] = p;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_pick(const StdGen g) {
    const int64_t k = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (k < g.k) g.cfin[k] = g.csup[g.scutval[k]];
}

// The kf nearest corners of corner i by (float squared distance, index), itself among them.
__global__ __launch_bounds__(kGenBlock) void k_gen_knn(const StdGen g) {
    const int64_t i = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (i >= g.k) return;
    const livo_std_corner a = g.cfin[i];
    float ld = -1.f;
    int64_t lj = -1;
    for (int t = 0; t < g.kf; t++) {
        float bd = INFINITY;
        int64_t bj = g.k;
        for (int64_t j = 0; j < g.k; j++) {
            const float d = gen_d2(a, g.cfin[j]);
            const bool after = d > ld || (d == ld && j > lj);
            const bool before = d < bd || (d == bd && j < bj);
            if (after && before) bd = d, bj = j;
        }
        g.knn[i * LIVO_STD_GEN_MAX_NEAR + t] = (uint32_t)bj;
        ld = bd;
        lj = bj;
    }
}

// One candidate triangle of build_stdesc (:845-947): false if a length gate drops it.
__device__ __forceinline__ bool gen_triangle(const StdGen& g, int64_t cand, unsigned long long* key, livo_std_desc* out) {
    const int64_t i = cand / g.pairs;
    int q = (int)(cand % g.pairs), m = 1;
    while (q >= g.prm.descriptor_near_num - 1 - m) q -= g.prm.descriptor_near_num - 1 - m, m++;
    const int n = m + 1 + q;
    if (n >= g.kf) return false;  // pin 4: only the neighbours found
    const livo_std_corner p1 = g.cfin[i], p2 = g.cfin[g.knn[i * LIVO_STD_GEN_MAX_NEAR + m]],
                          p3 = g.cfin[g.knn[i * LIVO_STD_GEN_MAX_NEAR + n]];
    auto side = [](const livo_std_corner& u, const livo_std_corner& v) {
        const double dx = (double)(u.xyz[0] - v.xyz[0]), dy = (double)(u.xyz[1] - v.xyz[1]), dz = (double)(u.xyz[2] - v.xyz[2]);
        return sqrt((dx * dx + dy * dy) + dz * dz);
    };
    double a = side(p1, p2), b = side(p1, p3), c = side(p3, p2);
    const double lo = g.prm.descriptor_min_len, hi = g.prm.descriptor_max_len;
    if (a > hi || b > hi || c > hi || a < lo || b < lo || c < lo) return false;
    int l1[3] = {1, 2, 0}, l2[3] = {1, 0, 3}, l3[3] = {0, 2, 3};
    auto swap = [](double& x, double& y, int (&u)[3], int (&v)[3]) {
        const double t = x;
        x = y;
        y = t;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int s = u[k];
            u[k] = v[k];
            v[k] = s;
        }
    };
    if (a > b) swap(a, b, l1, l2);
    if (b > c) swap(b, c, l2, l3);
    if (a > c) swap(a, c, l1, l3);
    *key = gen_pack((long long)(float)(a * 1000) - kStdCellBias, (long long)(float)(b * 1000) - kStdCellBias,
                    (long long)(float)(c * 1000) - kStdCellBias);
    if (!out) return true;
    const int va = l1[0] == l2[0] ? 0 : (l1[1] == l2[1] ? 1 : 2);
    const int vb = l1[0] == l3[0] ? 0 : (l1[1] == l3[1] ? 1 : 2);
    const int vc = l2[0] == l3[0] ? 0 : (l2[1] == l3[1] ? 1 : 2);
    auto pick = [&](int v, float x1, float x2, float x3) { return (double)(v == 0 ? x1 : (v == 1 ? x2 : x3)); };
    const double scale = 1.0 / g.prm.std_side_resolution;
    out->side_length[0] = scale * a, out->side_length[1] = scale * b, out->side_length[2] = scale * c;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double A = pick(va, p1.xyz[k], p2.xyz[k], p3.xyz[k]), B = pick(vb, p1.xyz[k], p2.xyz[k], p3.xyz[k]),
                     C = pick(vc, p1.xyz[k], p2.xyz[k], p3.xyz[k]);
        out->vertex_A[k] = A, out->vertex_B[k] = B, out->vertex_C[k] = C;
        out->center[k] = ((A + B) + C) / 3;
    }
    out->vertex_attached[0] = pick(va, p1.attached, p2.attached, p3.attached);
    out->vertex_attached[1] = pick(vb, p1.attached, p2.attached, p3.attached);
    out->vertex_attached[2] = pick(vc, p1.attached, p2.attached, p3.attached);
    out->frame_id = g.frame_id;
    out->pad = 0u;
    return true;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_cand(const StdGen g) {
    const int64_t c = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (c >= g.nc) return;
    unsigned long long key = kGenNoKey;
    if (!gen_triangle(g, c, &key, nullptr)) key = kGenNoKey;
    g.ckey[c] = key;
    g.cval[c] = (uint32_t)c;
    g.surv[c] = 0u;
}

// The first candidate of each key's run survives (feat_map, :897-952).
__global__ __launch_bounds__(kGenBlock) void k_gen_surv(const StdGen g) {
    const int64_t s = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (s >= g.nc) return;
    const unsigned long long key = g.sckey[s];
    if (key != kGenNoKey && (s == 0 || g.sckey[s - 1] != key)) g.surv[g.scval[s]] = 1u;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_emit(const StdGen g) {
    const int64_t c = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (c >= g.nc || !g.surv[c]) return;
    unsigned long long key;
    livo_std_desc d;
    if (gen_triangle(g, c, &key, &d)) g.descs_out[g.spos[c]] = d;
}

__global__ __launch_bounds__(kGenBlock) void k_gen_append(const float* __restrict__ src, int64_t n, int stride, float* dst) {
    const int64_t i = (int64_t)blockIdx.x * kGenBlock + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 3; k++) dst[i * 3 + k] = src[i * stride + k];
}

static inline unsigned gen_blocks(int64_t n) { return (unsigned)((n + kGenBlock - 1) / kGenBlock); }
static inline int gen_rc() { return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP; }
#define GEN_LAUNCH(kernel, count)                                                                                  \
    do {                                                                                                           \
        if ((count) > 0)                                                                                           \
            hipLaunchKernelGGL(kernel, dim3(gen_blocks(count)), dim3(kGenBlock), 0, (hipStream_t)stream, g);       \
    } while (0)

int launch_std_gen_append(const float* src, int64_t n, int stride, float* dst, void* stream) {
    if (n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_gen_append, dim3(gen_blocks(n)), dim3(kGenBlock), 0, (hipStream_t)stream, src, n, stride, dst);
    return gen_rc();
}
int launch_std_gen_keys(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_keys, g.n);
    return gen_rc();
}
int launch_std_gen_heads(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_heads, g.n);
    return gen_rc();
}
int launch_std_gen_voxels(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_voxels, g.n);
    return gen_rc();
}
int launch_std_gen_planes(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_rank, g.nv);
    GEN_LAUNCH(k_gen_plane, g.nv);
    GEN_LAUNCH(k_gen_connect, g.nv);
    GEN_LAUNCH(k_gen_jobs<false>, g.nv);
    return gen_rc();
}
int launch_std_gen_planes_out(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_planes_out, g.nv);
    return gen_rc();
}
int launch_std_gen_jobs(const StdGen& g, void* stream) {
    if (g.nj <= 0) return LIVO_OK;
    GEN_LAUNCH(k_gen_jobs<true>, g.nv);
    hipLaunchKernelGGL(k_gen_members, dim3((unsigned)g.nv), dim3(64), 0, (hipStream_t)stream, g);
    hipLaunchKernelGGL(k_gen_extract, dim3((unsigned)g.nj), dim3(kGenBlock), 0, (hipStream_t)stream, g);
    return gen_rc();
}
int launch_std_gen_corners(const StdGen& g, void* stream) {
    if (g.m <= 0) return LIVO_OK;
    GEN_LAUNCH(k_gen_concat, g.nj * g.seg_max);
    hipLaunchKernelGGL(k_gen_nms, dim3((unsigned)((g.m + kGenWaves - 1) / kGenWaves)), dim3(kGenBlock), 0, (hipStream_t)stream,
                       g);
    return gen_rc();
}
int launch_std_gen_keep(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_keep, g.m);
    return gen_rc();
}
int launch_std_gen_pick(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_pick, g.k);
    return gen_rc();
}
int launch_std_gen_cands(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_knn, g.k);
    GEN_LAUNCH(k_gen_cand, g.nc);
    return gen_rc();
}
int launch_std_gen_surv(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_surv, g.nc);
    return gen_rc();
}
int launch_std_gen_emit(const StdGen& g, void* stream) {
    GEN_LAUNCH(k_gen_emit, g.nc);
    return gen_rc();
}

}  // namespace livo
