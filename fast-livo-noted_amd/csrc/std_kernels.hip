// std_kernels.hip — CDNA4 (gfx950) kernels of the loop search: the resident Stable
// Triangle Descriptor database and STDescManager::SearchLoop (include/STD/STDesc.cpp:
// AddSTDescs :355-374, candidate_selector :960-1099, candidate_verify :1102-1192,
// triangle_solver :1194-1219, plane_geometric_verify :1221-1280).
//
//   k_std_commit     the staged frame's descriptors split into the hot record (64 B: side
//       lengths, attached counts, frame) and the vertices, appended in insertion order, with
//       the cell key (int)(side_length + 0.5) of each; its plane cloud behind the others'.
//   k_std_merge      the new (key, sequence) pairs, sorted, merged into the sorted index: an
//       old entry moves up by the new keys below its own, a new one lands behind the old
//       entries of its key.  A cell's run is then in insertion order.
//   k_std_match<EMIT>  one wave per source descriptor over its 27 or fewer cells: the run of
//       each by bisection, walked 64 entries a step.  The count pass counts a source's matches
//       and votes per stored frame (integer atomics); behind the scan of the counts the emit
//       pass writes the matches in selector order (source, cell visit order, run order).
//   k_std_rank       the loop at :1066-1098 over the vote counts, one block: the largest
//       (votes, lowest frame) candidate_num times, kept from 5 votes.
//   k_std_keys       a match's sort key: its frame's candidate index.  A stable sort by it
//       leaves each candidate's list contiguous and in selector order.
//   k_std_verify_sample  one block per (candidate, sample): triangle_solver by a one-sided
//       Jacobi SVD in double (one lane, registers), then the vote over the candidate's list.
//   k_std_verify_final   one block per candidate: the first maximum, the success list in
//       list order, plane_geometric_verify by brute-force 3-NN over the target's planes.
//   k_std_best       SearchLoop's choice among the candidates, one thread.
//
// Every store is a plain vector store.  Numerics: -ffp-contract=off, correctly rounded sqrt and
// division; sums in the reference's order.
#include <hip/hip_runtime.h>
#include <math.h>

#include "livo_internal.h"

namespace livo {

static_assert(sizeof(livo_std_desc) == 152, "STDesc");
static_assert(sizeof(livo_std_plane) == 24, "plane point");
static_assert(sizeof(livo_std_pair) == 12, "pair");
constexpr int kStdBlock = 256;
constexpr int kStdWaves = kStdBlock / 64;

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// |c| < kStdCellBias on every axis (livo_std_stage refuses larger side lengths)
__device__ __forceinline__ unsigned long long cell_key(int x, int y, int z) {
    return ((unsigned long long)(unsigned)(x + kStdCellBias) << 42) | ((unsigned long long)(unsigned)(y + kStdCellBias) << 21) |
           (unsigned long long)(unsigned)(z + kStdCellBias);
}

// first index in [0, n) with a[i] >= key (UPPER: > key)
template <bool UPPER>
__device__ __forceinline__ int64_t key_bound(const unsigned long long* __restrict__ a, int64_t n, unsigned long long key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const unsigned long long v = a[mid];
        if (UPPER ? v <= key : v < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kStdBlock) void k_std_commit(const StdCommit c) {
    const int64_t i = (int64_t)blockIdx.x * kStdBlock + threadIdx.x;
    if (i < c.n) {
        const livo_std_desc d = c.src[i];
        StdHot h;
        StdVerts v;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            h.side[k] = d.side_length[k];
            h.att[k] = d.vertex_attached[k];
            v.A[k] = d.vertex_A[k];
            v.B[k] = d.vertex_B[k];
            v.C[k] = d.vertex_C[k];
            v.center[k] = d.center[k];
        }
        h.frame = d.frame_id;
        h.pad = 0u;
        c.hot[c.n0 + i] = h;
        c.verts[c.n0 + i] = v;
        c.nkey[i] = cell_key((int)(d.side_length[0] + 0.5), (int)(d.side_length[1] + 0.5), (int)(d.side_length[2] + 0.5));
        c.nseq[i] = (uint32_t)(c.n0 + i);
    }
    if (i < c.m) c.planes[c.p0 + i] = c.src_planes[i];
    if (i == 0) c.plane_off[c.frame + 1] = (uint32_t)(c.p0 + c.m);
}

__global__ __launch_bounds__(kStdBlock) void k_std_merge(const unsigned long long* __restrict__ okey,
                                                         const uint32_t* __restrict__ oseq, int64_t n0,
                                                         const unsigned long long* __restrict__ nkey,
                                                         const uint32_t* __restrict__ nseq, int64_t n,
                                                         unsigned long long* __restrict__ dkey, uint32_t* __restrict__ dseq) {
    const int64_t i = (int64_t)blockIdx.x * kStdBlock + threadIdx.x;
    if (i < n0) {
        const unsigned long long k = okey[i];
        const int64_t pos = i + key_bound<false>(nkey, n, k);
        dkey[pos] = k;
        dseq[pos] = oseq[i];
    } else if (i < n0 + n) {
        const int64_t j = i - n0;
        const unsigned long long k = nkey[j];
        const int64_t pos = j + key_bound<true>(okey, n0, k);
        dkey[pos] = k;
        dseq[pos] = nseq[j];
    }
}

__global__ __launch_bounds__(kStdBlock) void k_std_count_cells(const unsigned long long* __restrict__ skey, int64_t n,
                                                               unsigned* __restrict__ ctr) {
    const int64_t i = (int64_t)blockIdx.x * kStdBlock + threadIdx.x;
    const bool head = i < n && (i == 0 || skey[i] != skey[i - 1]);
    const int cnt = __syncthreads_count(head ? 1 : 0);
    if (threadIdx.x == 0 && cnt > 0) atomicAdd(ctr + kStdCtrCells, (unsigned)cnt);
}

__global__ __launch_bounds__(kStdBlock) void k_std_unpack(const StdHot* __restrict__ hot, const StdVerts* __restrict__ verts,
                                                          int64_t n, livo_std_desc* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kStdBlock + threadIdx.x;
    if (i >= n) return;
    const StdHot h = hot[i];
    const StdVerts v = verts[i];
    livo_std_desc d;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d.side_length[k] = h.side[k];
        d.vertex_attached[k] = h.att[k];
        d.vertex_A[k] = v.A[k];
        d.vertex_B[k] = v.B[k];
        d.vertex_C[k] = v.C[k];
        d.center[k] = v.center[k];
    }
    d.frame_id = h.frame;
    d.pad = 0u;
    out[i] = d;
}

// candidate_selector's step 2 (:988-1040) for source descriptor i, one wave
template <bool EMIT>
__global__ __launch_bounds__(kStdBlock) void k_std_match(const StdParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kStdWaves + (threadIdx.x >> 6);
    if (i >= p.n_src) return;  // (whole waves leave; the kernel has no block barrier)
    const livo_std_desc* s = p.src + i;
    const double s0 = s->side_length[0], s1 = s->side_length[1], s2 = s->side_length[2];
    const double a0 = s->vertex_attached[0], a1 = s->vertex_attached[1], a2 = s->vertex_attached[2];
    const uint32_t sframe = s->frame_id;
    const double dis_threshold = norm3(s0, s1, s2) * p.prm.rough_dis_threshold;
    const uint32_t base = EMIT ? p.off[i] : 0u;
    uint32_t total = 0;
    for (int c = 0; c < 27; c++) {
        const int px = (int)(s0 + (double)(c / 9 - 1)), py = (int)(s1 + (double)((c / 3) % 3 - 1)),
                  pz = (int)(s2 + (double)(c % 3 - 1));
        if (!(norm3(s0 - ((double)px + 0.5), s1 - ((double)py + 0.5), s2 - ((double)pz + 0.5)) < 1.5)) continue;
        const unsigned long long key = cell_key(px, py, pz);
        const int64_t lo = key_bound<false>(p.skey, p.n_db, key);
        int64_t hi = lo;
        if (lo < p.n_db && p.skey[lo] == key) hi = key_bound<true>(p.skey, p.n_db, key);
        for (int64_t b = lo; b < hi; b += 64) {  // a run longer than the wave: in steps
            const int64_t j = b + lane;
            bool ok = false;
            uint32_t seq = 0u, frame = 0u;
            if (j < hi) {
                seq = p.sseq[j];
                const StdHot h = p.hot[seq];
                frame = h.frame;
                if ((uint32_t)(sframe - frame) > (uint32_t)p.prm.skip_near_num) {  // unsigned, as written (:1007)
                    const double dis = norm3(s0 - h.side[0], s1 - h.side[1], s2 - h.side[2]);
                    if (dis < dis_threshold) {
                        const double diff = 2.0 * norm3(a0 - h.att[0], a1 - h.att[1], a2 - h.att[2]) /
                                            norm3(a0 + h.att[0], a1 + h.att[1], a2 + h.att[2]);
                        ok = diff < p.prm.vertex_diff_threshold;
                    }
                }
            }
            const unsigned long long mask = __ballot(ok);
            if (ok) {
                if (EMIT) {
                    livo_std_pair m;
                    m.src = i;
                    m.frame = (int32_t)frame;
                    m.db_index = (int32_t)seq;
                    p.matches[base + total + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = m;
                } else if (frame < (uint32_t)p.n_frames) {
                    atomicAdd(p.votes + frame, 1u);
                }
            }
            total += (uint32_t)__popcll(mask);
        }
    }
    if (!EMIT && lane == 0) p.cnt[i] = total;
}

// :1066-1098.  A frame that is picked and not kept (fewer than 5 votes) is not zeroed, so every
// later round picks it again: the loop ends there.
__global__ __launch_bounds__(1024) void k_std_rank(const StdParams p) {
    __shared__ unsigned long long s_best[16];
    __shared__ unsigned long long s_pick;
    const int tid = threadIdx.x;
    int n_cand = 0;
    uint32_t off = 0;
    for (int cnt = 0; cnt < p.prm.candidate_num; cnt++) {
        unsigned long long best = 0ull;  // votes << 32 | ~frame: the most votes, then the lowest frame
        for (int f = tid; f < p.n_frames; f += 1024) {
            const uint32_t v = p.votes[f];
            if (v > 1u) {
                const unsigned long long k = ((unsigned long long)v << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)f);
                best = k > best ? k : best;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if ((tid & 63) == 0) s_best[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 16; w++) best = s_best[w] > best ? s_best[w] : best;
            s_pick = best;
        }
        __syncthreads();
        const unsigned long long pick = s_pick;
        const uint32_t v = (uint32_t)(pick >> 32);
        if (v < 5u) break;  // (block-uniform)
        const uint32_t f = 0xFFFFFFFFu - (uint32_t)pick;
        if (tid == 0) {
            p.votes[f] = 0u;
            p.cand_of_frame[f] = n_cand;
            p.coff[n_cand] = off;
            livo_std_candidate c{};
            c.frame = (int32_t)f;
            c.votes = (int32_t)v;
            const int skip_len = (int)(v / 50u) + 1;
            c.use_size = (int)v / skip_len;
            p.cands[n_cand] = c;
        }
        off += v;
        n_cand++;
        __syncthreads();  // the zeroed vote before the next round reads it
    }
    if (tid == 0) {
        p.coff[n_cand] = off;
        p.ctr[kStdCtrCands] = (unsigned)n_cand;
        p.ctr[kStdCtrTotal] = p.n_src > 0 ? p.off[p.n_src - 1] + p.cnt[p.n_src - 1] : 0u;
    }
}

__global__ __launch_bounds__(kStdBlock) void k_std_keys(const StdParams p, int64_t total) {
    const int64_t m = (int64_t)blockIdx.x * kStdBlock + threadIdx.x;
    if (m >= total) return;
    const int32_t f = p.matches[m].frame;
    const int32_t k = (f >= 0 && f < p.n_frames) ? p.cand_of_frame[f] : -1;
    p.mkey[m] = k >= 0 ? (uint32_t)k : kStdNoCand;
    p.mval[m] = (uint32_t)m;
}

// One-sided Jacobi: columns of C rotated until orthogonal, C V = U S.  C has rank 2 (centred
// triangles), so U's third column is the cross product of the two that carry a singular value.
// rot = V U^T with V's matching column flipped when the determinant is negative (:1209-1217).
__device__ void triangle_solve(const double* sA, const double* sB, const double* sC, const double* sc, const double* rA,
                               const double* rB, const double* rC, const double* rc, double* R, double* t) {
    double src[3][3], ref[3][3];  // [row][col]
#pragma unroll
    for (int r = 0; r < 3; r++) {
        src[r][0] = sA[r] - sc[r];
        src[r][1] = sB[r] - sc[r];
        src[r][2] = sC[r] - sc[r];
        ref[r][0] = rA[r] - rc[r];
        ref[r][1] = rB[r] - rc[r];
        ref[r][2] = rC[r] - rc[r];
    }
    double c[3][3], v[3][3];  // column-major in the first index: c[col][row]
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            c[q][r] = src[r][0] * ref[q][0] + src[r][1] * ref[q][1] + src[r][2] * ref[q][2];  // src * ref^T
            v[q][r] = r == q ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 12; sweep++) {
        bool moved = false;
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int a = pq == 2 ? 1 : 0, b = pq == 0 ? 1 : 2;
            const double alpha = c[a][0] * c[a][0] + c[a][1] * c[a][1] + c[a][2] * c[a][2];
            const double beta = c[b][0] * c[b][0] + c[b][1] * c[b][1] + c[b][2] * c[b][2];
            const double gamma = c[a][0] * c[b][0] + c[a][1] * c[b][1] + c[a][2] * c[b][2];
            if (gamma == 0.0 || !(fabs(gamma) > 1e-17 * sqrt(alpha * beta))) continue;
            moved = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double ca = c[a][r], cb = c[b][r];
                c[a][r] = cs * ca - sn * cb;
                c[b][r] = sn * ca + cs * cb;
                const double va = v[a][r], vb = v[b][r];
                v[a][r] = cs * va - sn * vb;
                v[b][r] = sn * va + cs * vb;
            }
        }
        if (!moved) break;
    }
    // the column without a singular value: the shortest
    double nn[3];
#pragma unroll
    for (int q = 0; q < 3; q++) nn[q] = c[q][0] * c[q][0] + c[q][1] * c[q][1] + c[q][2] * c[q][2];
    const int z = (nn[0] <= nn[1] && nn[0] <= nn[2]) ? 0 : (nn[1] <= nn[2] ? 1 : 2);
    const int x = (z + 1) % 3, y = (z + 2) % 3;  // (x, y, z) a cyclic order: det [ux uy uz] = +1
    double u[3][3];
    const double nx = sqrt(nn[x]), ny = sqrt(nn[y]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        u[x][r] = c[x][r] / nx;
        u[y][r] = c[y][r] / ny;
    }
    u[z][0] = u[x][1] * u[y][2] - u[x][2] * u[y][1];
    u[z][1] = u[x][2] * u[y][0] - u[x][0] * u[y][2];
    u[z][2] = u[x][0] * u[y][1] - u[x][1] * u[y][0];
    // V is a product of rotations and det [ux uy uz] = +1, so V U^T is the proper rotation the
    // reference reaches by its flip (:1213-1217): vx <- ux, vy <- uy, vx x vy <- ux x uy
    const double sz = 1.0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) R[3 * r + q] = v[x][r] * u[x][q] + v[y][r] * u[y][q] + sz * v[z][r] * u[z][q];
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = (-R[3 * r] * sc[0] + -R[3 * r + 1] * sc[1] + -R[3 * r + 2] * sc[2]) + rc[r];
}

// dis_A, dis_B, dis_C < 3.0 (:1133-1143)
__device__ __forceinline__ bool pair_agrees(const double* R, const double* t, const livo_std_desc* s, const StdVerts* d) {
    const double* sv[3] = {s->vertex_A, s->vertex_B, s->vertex_C};
    const double* dv[3] = {d->A, d->B, d->C};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = sv[k][0], y = sv[k][1], z = sv[k][2];
        const double tx = (R[0] * x + R[1] * y + R[2] * z) + t[0], ty = (R[3] * x + R[4] * y + R[5] * z) + t[1],
                     tz = (R[6] * x + R[7] * y + R[8] * z) + t[2];
        ok = ok && norm3(tx - dv[k][0], ty - dv[k][1], tz - dv[k][2]) < 3.0;
    }
    return ok;
}

__global__ __launch_bounds__(kStdBlock) void k_std_verify_sample(const StdParams p) {
    __shared__ double s_rt[12];
    __shared__ unsigned s_vote;
    const int k = blockIdx.y, smp = blockIdx.x, tid = threadIdx.x;
    const int L = p.cands[k].votes, use_size = p.cands[k].use_size;
    if (smp >= use_size) return;  // (block-uniform)
    const int skip_len = L / 50 + 1;
    const uint32_t* list = p.sval + p.coff[k];
    if (tid == 0) {
        const livo_std_pair m = p.matches[list[smp * skip_len]];
        const livo_std_desc* s = p.src + m.src;
        const StdVerts* d = p.verts + m.db_index;
        double R[9], t[3];
        triangle_solve(s->vertex_A, s->vertex_B, s->vertex_C, s->center, d->A, d->B, d->C, d->center, R, t);
        double* out = p.sample_rt + ((size_t)k * kStdSamples + smp) * 12;
        for (int q = 0; q < 9; q++) s_rt[q] = out[q] = R[q];
        for (int q = 0; q < 3; q++) s_rt[9 + q] = out[9 + q] = t[q];
        s_vote = 0u;
    }
    __syncthreads();
    double R[9], t[3];
    for (int q = 0; q < 9; q++) R[q] = s_rt[q];
    for (int q = 0; q < 3; q++) t[q] = s_rt[9 + q];
    unsigned vote = 0;
    for (int j = tid; j < L; j += kStdBlock) {
        const livo_std_pair m = p.matches[list[j]];
        vote += pair_agrees(R, t, p.src + m.src, p.verts + m.db_index) ? 1u : 0u;
    }
    if (vote) atomicAdd(&s_vote, vote);
    __syncthreads();
    if (tid == 0) p.vote_list[k * kStdSamples + smp] = s_vote;
}

__global__ __launch_bounds__(kStdBlock) void k_std_verify_final(const StdParams p) {
    __shared__ double s_rt[12];
    __shared__ int s_max[2];
    __shared__ unsigned s_wave[kStdWaves];
    __shared__ unsigned s_count;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    livo_std_candidate rec = p.cands[k];
    const int L = rec.votes;
    if (tid == 0) {
        int max_vote = 0, max_index = 0;
        for (int i = 0; i < rec.use_size; i++) {
            const int v = (int)p.vote_list[k * kStdSamples + i];
            if (max_vote < v) {
                max_index = i;
                max_vote = v;
            }
        }
        s_max[0] = max_vote;
        s_max[1] = max_index;
        const double* rt = p.sample_rt + ((size_t)k * kStdSamples + max_index) * 12;
        for (int q = 0; q < 12; q++) s_rt[q] = max_vote >= 4 ? rt[q] : (q == 0 || q == 4 || q == 8 ? 1.0 : 0.0);
        s_count = 0u;
    }
    __syncthreads();
    rec.max_vote = s_max[0];
    rec.max_vote_index = s_max[1];
    double R[9], t[3];
    for (int q = 0; q < 9; q++) R[q] = rec.rot[q] = s_rt[q];
    for (int q = 0; q < 3; q++) t[q] = rec.t[q] = s_rt[9 + q];
    if (rec.max_vote < 4) {  // (block-uniform)
        if (tid == 0) {
            rec.score = -1.0;
            p.cands[k] = rec;
            p.n_succ[k] = 0u;
        }
        return;
    }
    // the success list, in list order (:1169-1184)
    const uint32_t* list = p.sval + p.coff[k];
    livo_std_pair* succ = p.succ + p.coff[k];
    unsigned n_succ = 0;
    for (int b = 0; b < L; b += kStdBlock) {
        const int j = b + tid;
        bool ok = false;
        livo_std_pair m{};
        if (j < L) {
            m = p.matches[list[j]];
            ok = pair_agrees(R, t, p.src + m.src, p.verts + m.db_index);
        }
        const unsigned long long mask = __ballot(ok);
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(mask);
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int w = 0; w < kStdWaves; w++) {
            before += w < wave ? s_wave[w] : 0u;
            all += s_wave[w];
        }
        if (ok) succ[n_succ + before + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = m;
        n_succ += all;
        __syncthreads();
    }
    // plane_geometric_verify (:1221-1280): source = the staged frame's planes, target = the candidate's
    const uint32_t t0 = p.plane_off[rec.frame], nt = p.plane_off[rec.frame + 1] - t0;
    const livo_std_plane* tgt = p.planes + t0;
    const double normal_threshold = p.prm.normal_threshold, dis_threshold = p.prm.dis_threshold;
    unsigned useful = 0;
    for (int i = tid; i < p.n_src_planes; i += kStdBlock) {
        const livo_std_plane sp = p.src_planes[i];
        const double x = (double)sp.xyz[0], y = (double)sp.xyz[1], z = (double)sp.xyz[2];
        const double pi[3] = {(R[0] * x + R[1] * y + R[2] * z) + t[0], (R[3] * x + R[4] * y + R[5] * z) + t[1],
                              (R[6] * x + R[7] * y + R[8] * z) + t[2]};
        const double nx = (double)sp.normal[0], ny = (double)sp.normal[1], nz = (double)sp.normal[2];
        const double ni[3] = {R[0] * nx + R[1] * ny + R[2] * nz, R[3] * nx + R[4] * ny + R[5] * nz,
                              R[6] * nx + R[7] * ny + R[8] * nz};
        const float qx = (float)pi[0], qy = (float)pi[1], qz = (float)pi[2];
        // the 3 nearest by float squared distance, ascending (ties: the lower index first)
        float bd[3] = {INFINITY, INFINITY, INFINITY};
        uint32_t bi[3] = {0u, 0u, 0u};
        for (uint32_t j = 0; j < nt; j++) {
            const float dx = qx - tgt[j].xyz[0], dy = qy - tgt[j].xyz[1], dz = qz - tgt[j].xyz[2];
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d < bd[2]) {
                if (d < bd[1]) {
                    bd[2] = bd[1];
                    bi[2] = bi[1];
                    if (d < bd[0]) {
                        bd[1] = bd[0];
                        bi[1] = bi[0];
                        bd[0] = d;
                        bi[0] = j;
                    } else {
                        bd[1] = d;
                        bi[1] = j;
                    }
                } else {
                    bd[2] = d;
                    bi[2] = j;
                }
            }
        }
        const uint32_t found = nt < 3u ? nt : 3u;  // only the neighbours that exist
        for (uint32_t j = 0; j < found; j++) {
            const livo_std_plane tp = tgt[bi[j]];
            const double tn[3] = {(double)tp.normal[0], (double)tp.normal[1], (double)tp.normal[2]};
            const double inc = norm3(ni[0] - tn[0], ni[1] - tn[1], ni[2] - tn[2]);
            const double add = norm3(ni[0] + tn[0], ni[1] + tn[1], ni[2] + tn[2]);
            const double ptp = fabs(tn[0] * (pi[0] - (double)tp.xyz[0]) + tn[1] * (pi[1] - (double)tp.xyz[1]) +
                                    tn[2] * (pi[2] - (double)tp.xyz[2]));
            if ((inc < normal_threshold || add < normal_threshold) && ptp < dis_threshold) {
                useful++;
                break;
            }
        }
    }
    if (useful) atomicAdd(&s_count, useful);
    __syncthreads();
    if (tid == 0) {
        rec.score = p.n_src_planes > 0 ? (double)s_count / (double)p.n_src_planes : (double)NAN;
        p.cands[k] = rec;
        p.n_succ[k] = n_succ;
    }
}

// SearchLoop's step 2 and result (:318-352)
__global__ void k_std_best(const StdParams p, int n_cand) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double best_score = 0.0;
    int best = -1;
    for (int k = 0; k < n_cand; k++) {
        const double s = p.cands[k].score;
        if (s > best_score) {  // (NaN never wins)
            best_score = s;
            best = k;
        }
    }
    livo_std_result r{};
    r.n_candidates = n_cand;
    r.frame = r.candidate = -1;
    r.rot[0] = r.rot[4] = r.rot[8] = 1.0;
    if (best >= 0 && best_score > p.prm.icp_threshold) {
        const livo_std_candidate c = p.cands[best];
        r.frame = c.frame;
        r.score = best_score;
        for (int q = 0; q < 9; q++) r.rot[q] = c.rot[q];
        for (int q = 0; q < 3; q++) r.t[q] = c.t[q];
        r.n_pairs = (int32_t)p.n_succ[best];
        r.candidate = best;
    }
    *p.result = r;
}

static inline unsigned std_blocks(int64_t n) { return (unsigned)((n + kStdBlock - 1) / kStdBlock); }
static inline int std_rc() { return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP; }

int launch_std_commit(const StdCommit& c, void* stream) {
    const int64_t n = c.n > c.m ? c.n : c.m;
    hipLaunchKernelGGL(k_std_commit, dim3(std_blocks(n > 1 ? n : 1)), dim3(kStdBlock), 0, (hipStream_t)stream, c);
    return std_rc();
}
int launch_std_merge(const unsigned long long* okey, const uint32_t* oseq, int64_t n0, const unsigned long long* nkey,
                     const uint32_t* nseq, int64_t n, unsigned long long* dkey, uint32_t* dseq, void* stream) {
    if (n0 + n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_std_merge, dim3(std_blocks(n0 + n)), dim3(kStdBlock), 0, (hipStream_t)stream, okey, oseq, n0, nkey,
                       nseq, n, dkey, dseq);
    return std_rc();
}
int launch_std_count_cells(const unsigned long long* skey, int64_t n, unsigned* ctr, void* stream) {
    if (n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_std_count_cells, dim3(std_blocks(n)), dim3(kStdBlock), 0, (hipStream_t)stream, skey, n, ctr);
    return std_rc();
}
int launch_std_unpack(const StdHot* hot, const StdVerts* verts, int64_t n, livo_std_desc* out, void* stream) {
    if (n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_std_unpack, dim3(std_blocks(n)), dim3(kStdBlock), 0, (hipStream_t)stream, hot, verts, n, out);
    return std_rc();
}
int launch_std_match(const StdParams& p, bool emit, void* stream) {
    if (p.n_src <= 0) return LIVO_OK;
    const dim3 grid((unsigned)((p.n_src + kStdWaves - 1) / kStdWaves));
    if (emit)
        hipLaunchKernelGGL(k_std_match<true>, grid, dim3(kStdBlock), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(k_std_match<false>, grid, dim3(kStdBlock), 0, (hipStream_t)stream, p);
    return std_rc();
}
int launch_std_rank(const StdParams& p, void* stream) {
    hipLaunchKernelGGL(k_std_rank, dim3(1), dim3(1024), 0, (hipStream_t)stream, p);
    return std_rc();
}
int launch_std_keys(const StdParams& p, int64_t total, void* stream) {
    if (total <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_std_keys, dim3(std_blocks(total)), dim3(kStdBlock), 0, (hipStream_t)stream, p, total);
    return std_rc();
}
int launch_std_verify(const StdParams& p, int n_cand, void* stream) {
    if (n_cand > 0) {
        hipLaunchKernelGGL(k_std_verify_sample, dim3(kStdSamples, (unsigned)n_cand), dim3(kStdBlock), 0, (hipStream_t)stream,
                           p);
        hipLaunchKernelGGL(k_std_verify_final, dim3((unsigned)n_cand), dim3(kStdBlock), 0, (hipStream_t)stream, p);
    }
    hipLaunchKernelGGL(k_std_best, dim3(1), dim3(64), 0, (hipStream_t)stream, p, n_cand);
    return std_rc();
}

}  // namespace livo
