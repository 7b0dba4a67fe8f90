// GPU unit check (tests/test_gpu_ivox.py): wave_nth (fast-livo-noted_amd/csrc/
// wave_select.h), the wave-parallel std::nth_element of the iVox search,
// against libstdc++'s std::nth_element on the host, element for element.
// One wave per case; cases of 1..kWRaw elements with many ties, and McIlroy
// adversaries (nth_adversary.h) that run each kernel into introselect's depth
// limit.  wave_nth / wave_nth_big return false there (their callers hand the
// query on): the returned status of every case must equal the host predicate
// that replays introselect's rounds, and only a case the predicate says reaches
// the limit is left unchecked element for element.  team_nth heap-selects on
// its lane 0: every case is compared element for element.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "nth_adversary.h"
#include "wave_select.h"

using namespace livo;

struct Case {
    int n, first, nth;
};

__global__ void k_check(const Case* cases, const float* d_in, float* d_out, uint32_t* id_out, int* status, int ncase) {
    __shared__ WaveLds lds[1];
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= ncase) return;
    WaveLds& L = lds[0];
    const Case k = cases[c];
    for (int p = lane; p < k.n; p += 64) {
        L.d[p] = d_in[c * kWRaw + p];
        L.id[p] = (uint32_t)p;
    }
    wave_sync();
    const bool ok = wave_nth(L, k.first, k.nth, k.n, lane);
    for (int p = lane; p < k.n; p += 64) {
        d_out[c * kWRaw + p] = L.d[p];
        id_out[c * kWRaw + p] = L.id[p];
    }
    if (lane == 0) status[c] = ok ? 1 : 0;
}

// wave_nth_big (lists past WaveLds, k_ivox_knn_big_wave): one wave per case,
// the list and its tables in dynamic LDS of kBigCap entries.
constexpr int kBigCap = 4096;
__global__ void k_check_big(const Case* cases, const float* d_in, float* d_out, uint32_t* id_out, int* status,
                            int ncase) {
    extern __shared__ uint32_t lds[];
    const BigList L{reinterpret_cast<float*>(lds), lds + kBigCap, reinterpret_cast<uint16_t*>(lds + 2 * kBigCap),
                    reinterpret_cast<uint16_t*>(lds + 2 * kBigCap) + kBigCap};
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= ncase) return;
    const Case k = cases[c];
    for (int p = lane; p < k.n; p += 64) {
        L.d[p] = d_in[(size_t)c * kBigCap + p];
        L.id[p] = (uint32_t)p;
    }
    wave_sync();
    const bool ok = wave_nth_big(L, k.first, k.nth, k.n, lane);
    for (int p = lane; p < k.n; p += 64) {
        d_out[(size_t)c * kBigCap + p] = L.d[p];
        id_out[(size_t)c * kBigCap + p] = L.id[p];
    }
    if (lane == 0) status[c] = ok ? 1 : 0;
}

// team_nth (k_ivox_knn_team): four teams a wave, one case each, lists of up to 128
constexpr int kTeamCap = 128;  // (k_ivox_knn_team's list capacity)
__global__ void k_check_team(const Case* cases, const float* d_in, uint32_t* id_out, int ncase) {
    __shared__ SelElem lst[4][kTeamCap];
    __shared__ uint8_t tabs[4][2][kTeamCap];
    const int lane = threadIdx.x, tl = lane & 15, team = lane >> 4;
    const int c = blockIdx.x * 4 + team;
    if (c >= ncase) return;  // (team-uniform)
    const Case k = cases[c];
    SelElem* L = lst[team];
    for (int p = tl; p < k.n; p += 16) L[p] = SelElem{d_in[(size_t)c * kTeamCap + p], (uint32_t)p};
    wave_sync();
    team_nth(L, tabs[team][0], tabs[team][1], k.first, k.nth, k.n, tl, lane);
    for (int p = tl; p < k.n; p += 16) id_out[(size_t)c * kTeamCap + p] = L[p].id;
}

struct DP {
    float d;
    uint32_t id;
    bool operator<(const DP& o) const { return d < o.d; }
};

// Adversarial cases appended to a set: ranges of `len` elements after `first` others, the 5 smallest
// (nth = first + 4, the selection the iVox search runs: pivot driven to the top) and nth = n - 5
// (pivot driven to the bottom); keys are the adversary's ranks.
static void add_adversaries(std::vector<Case>& cases, std::vector<float>& in, int cap, std::initializer_list<int> lens) {
    for (int len : lens)
        for (int first : {0, 5})
            for (int form = 0; form < 2; form++) {
                const int n = first + len;
                if (n > cap) continue;
                const int nth = form == 0 ? first + 4 : n - 5;
                const std::vector<int> v = nth_adversary::sequence(n, first, nth, form == 0);
                const size_t c = cases.size();
                cases.push_back(Case{n, first, nth});
                in.resize((c + 1) * (size_t)cap, 0.f);
                for (int p = 0; p < n; p++) in[c * (size_t)cap + p] = (float)v[(size_t)p];
            }
}

// One set's results against libstdc++: ids element for element, and (status != nullptr) the returned
// status against the host predicate.  Returns the mismatches; `limit` counts the cases the predicate
// says reach the depth limit.
static long compare(const char* name, const std::vector<Case>& cases, const std::vector<float>& in,
                    const std::vector<uint32_t>& ids, const int* status, int cap, long& limit) {
    long bad = 0;
    limit = 0;
    for (size_t c = 0; c < cases.size(); c++) {
        const Case k = cases[c];
        std::vector<DP> ref(k.n);
        std::vector<SelElem> keys(k.n);
        for (int p = 0; p < k.n; p++) {
            ref[p] = DP{in[c * (size_t)cap + p], (uint32_t)p};
            keys[p] = SelElem{ref[p].d, (uint32_t)p};
        }
        const bool lim = nth_adversary::depth_limit_reached(keys, k.first, k.nth, k.n);
        limit += lim;
        if (status) {
            if ((status[c] != 0) == lim) {  // true where the limit ran out, or false where it did not
                if (bad < 3) std::printf("%s case %zu n %d first %d nth %d: status %d, depth limit %s\n", name, c, k.n,
                                         k.first, k.nth, status[c], lim ? "reached" : "not reached");
                bad++;
                continue;
            }
            if (lim) continue;  // the caller's fallback finishes it: nothing to compare here
        }
        std::nth_element(ref.begin() + k.first, ref.begin() + k.nth, ref.begin() + k.n);
        for (int p = 0; p < k.n; p++)
            if (ids[c * (size_t)cap + p] != ref[p].id) {
                if (bad < 3) std::printf("%s case %zu n %d first %d nth %d: pos %d got %u want %u\n", name, c, k.n,
                                         k.first, k.nth, p, ids[c * (size_t)cap + p], ref[p].id);
                bad++;
                break;
            }
    }
    return bad;
}

int main(int argc, char** argv) {
    const int nrand = argc > 1 ? std::atoi(argv[1]) : 20000;
    std::mt19937 rng(99);
    std::vector<Case> cases(nrand);
    std::vector<float> din((size_t)nrand * kWRaw, 0.f);
    for (int c = 0; c < nrand; c++) {
        const int n = 1 + (int)(rng() % (c % 5 == 0 ? (unsigned)kWRaw : 140u));
        const int levels = 1 + (int)(rng() % 30u);
        for (int p = 0; p < n; p++)
            din[(size_t)c * kWRaw + p] = (c % 2) ? (float)(rng() % (unsigned)levels) * 0.25f
                                                 : std::ldexp((float)(rng() & 0xFFFFF), -20);
        const int first = (c % 4 == 0 && n > 1) ? (int)(rng() % (unsigned)n) : 0;
        const int nth = first + (int)(rng() % (unsigned)(n - first));
        cases[c] = Case{n, first, nth};
    }
    add_adversaries(cases, din, kWRaw, {24, 38, 64, 100, 128, 129, 200, 300, 400, 500, 507, 512});
    const int ncase = (int)cases.size();
    Case* dc;
    float *di, *dd;
    uint32_t* dids;
    int* dst;
    hipMalloc(&dc, sizeof(Case) * ncase);
    hipMalloc(&di, din.size() * 4);
    hipMalloc(&dd, din.size() * 4);
    hipMalloc(&dids, din.size() * 4);
    hipMalloc(&dst, 4 * ncase);
    hipMemcpy(dc, cases.data(), sizeof(Case) * ncase, hipMemcpyHostToDevice);
    hipMemcpy(di, din.data(), din.size() * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_check, dim3(ncase), dim3(64), 0, 0, dc, di, dd, dids, dst, ncase);
    if (hipDeviceSynchronize() != hipSuccess) {
        std::printf("kernel failed\n");
        return 2;
    }
    std::vector<uint32_t> idout(din.size());
    std::vector<int> st(ncase);
    hipMemcpy(idout.data(), dids, din.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(st.data(), dst, 4 * ncase, hipMemcpyDeviceToHost);
    long wlimit = 0;
    const long bad = compare("wave", cases, din, idout, st.data(), kWRaw, wlimit);
    std::printf("wave_nth: %d cases of up to %d, %ld mismatched, %ld reached the depth limit\n", ncase, kWRaw, bad,
                wlimit);
    // wave_nth_big: cases of 1..kBigCap elements (ties, narrow and wide value ranges)
    const int nbrand = std::max(200, nrand / 10);
    std::vector<Case> bcases(nbrand);
    std::vector<float> bin((size_t)nbrand * kBigCap, 0.f);
    for (int c = 0; c < nbrand; c++) {
        const int n = 1 + (int)(rng() % (c % 3 == 0 ? (unsigned)kBigCap : 2000u));
        const int levels = 1 + (int)(rng() % 200u);
        for (int p = 0; p < n; p++)
            bin[(size_t)c * kBigCap + p] = (c % 2) ? (float)(rng() % (unsigned)levels) * 0.25f
                                                   : std::ldexp((float)(rng() & 0xFFFFF), -20);
        const int first = (c % 4 == 0 && n > 1) ? (int)(rng() % (unsigned)n) : 0;
        const int nth = first + (int)(rng() % (unsigned)(n - first));
        bcases[c] = Case{n, first, nth};
    }
    add_adversaries(bcases, bin, kBigCap, {24, 128, 513, 600, 1000, 2048, 3000, 4091, 4096});
    const int nbig = (int)bcases.size();
    Case* bc;
    float *bi, *bd;
    uint32_t* bids;
    int* bst;
    hipMalloc(&bc, sizeof(Case) * nbig);
    hipMalloc(&bi, bin.size() * 4);
    hipMalloc(&bd, bin.size() * 4);
    hipMalloc(&bids, bin.size() * 4);
    hipMalloc(&bst, 4 * nbig);
    hipMemcpy(bc, bcases.data(), sizeof(Case) * nbig, hipMemcpyHostToDevice);
    hipMemcpy(bi, bin.data(), bin.size() * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_check_big, dim3(nbig), dim3(64), kBigCap * 12, 0, bc, bi, bd, bids, bst, nbig);
    if (hipDeviceSynchronize() != hipSuccess) {
        std::printf("big kernel failed\n");
        return 2;
    }
    std::vector<uint32_t> bout(bin.size());
    std::vector<int> bs(nbig);
    hipMemcpy(bout.data(), bids, bin.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(bs.data(), bst, 4 * nbig, hipMemcpyDeviceToHost);
    long blimit = 0;
    const long bbad = compare("big", bcases, bin, bout, bs.data(), kBigCap, blimit);
    std::printf("wave_nth_big: %d cases of up to %d, %ld mismatched, %ld reached the depth limit\n", nbig, kBigCap,
                bbad, blimit);
    // team_nth: 1..128 elements, mostly the 6..40 of an iVox grid's segment; ties
    // (few levels, incl. all equal) and wide ranges; the adversaries reach the
    // heap select on lane 0, on the range as the rounds before it narrowed it
    const int ntrand = std::max(4000, nrand);
    std::vector<Case> tcases(ntrand);
    std::vector<float> tin((size_t)ntrand * kTeamCap, 0.f);
    for (int c = 0; c < ntrand; c++) {
        const int n = 1 + (int)(rng() % (c % 3 == 0 ? (unsigned)kTeamCap : 40u));
        const int levels = 1 + (int)(rng() % (c % 7 == 0 ? 2u : 30u));
        for (int p = 0; p < n; p++)
            tin[(size_t)c * kTeamCap + p] = (c % 2) ? (float)(rng() % (unsigned)levels) * 0.25f
                                                    : std::ldexp((float)(rng() & 0xFFFFF), -20);
        const int first = (c % 4 == 0 && n > 1) ? (int)(rng() % (unsigned)n) : 0;
        const int nth = (c % 5 == 0) ? first + std::min(4, n - 1 - first)
                                     : first + (int)(rng() % (unsigned)(n - first));
        tcases[c] = Case{n, first, nth};
    }
    add_adversaries(tcases, tin, kTeamCap, {24, 25, 31, 32, 33, 38, 48, 64, 90, 100, 119, 123, 127, 128});
    const int nteam = (int)tcases.size();
    Case* tc;
    float* ti;
    uint32_t* tids;
    hipMalloc(&tc, sizeof(Case) * nteam);
    hipMalloc(&ti, tin.size() * 4);
    hipMalloc(&tids, tin.size() * 4);
    hipMemcpy(tc, tcases.data(), sizeof(Case) * nteam, hipMemcpyHostToDevice);
    hipMemcpy(ti, tin.data(), tin.size() * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_check_team, dim3((nteam + 3) / 4), dim3(64), 0, 0, tc, ti, tids, nteam);
    if (hipDeviceSynchronize() != hipSuccess) {
        std::printf("team kernel failed\n");
        return 2;
    }
    std::vector<uint32_t> tout(tin.size());
    hipMemcpy(tout.data(), tids, tin.size() * 4, hipMemcpyDeviceToHost);
    long tlimit = 0;
    const long tbad = compare("team", tcases, tin, tout, nullptr, kTeamCap, tlimit);
    std::printf("team_nth: %d cases of up to %d, %ld mismatched, %ld reached the depth limit\n", nteam, kTeamCap, tbad,
                tlimit);
    std::printf("%d cases, %ld mismatches\n", ncase + nbig + nteam, bad + bbad + tbad);
    std::printf("depth limit reached: wave_nth %ld wave_nth_big %ld team_nth %ld\n", wlimit, blimit, tlimit);
    if (wlimit == 0 || blimit == 0 || tlimit == 0) {
        std::printf("a kernel never reached the depth limit\n");
        return 1;
    }
    return (bad + bbad + tbad) == 0 ? 0 : 1;
}
