// Command-line front of nth_adversary.h for the Python tests
// (tests/ivox_cascade_cases.py builds it with g++).
//
//   nth_adversary_cli gen N FIRST NTH [MIRRORED=1]
//       line 1: the adversarial permutation of 0..N-1
//       line 2: depth_limit=<0|1> sel_matches_std=<0|1>
//   nth_adversary_cli check FIRST NTH K0 K1 ...
//       the same status line for std::nth_element(K + FIRST, K + NTH, K + n)
//       on the given float keys
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nth_adversary.h"

template <class K>
static int status(const std::vector<K>& keys, int first, int nth) {
    const int n = (int)keys.size();
    if (first < 0 || nth < first || nth >= n) {
        std::fprintf(stderr, "need 0 <= first <= nth < n\n");
        return 2;
    }
    std::printf("depth_limit=%d sel_matches_std=%d\n", (int)nth_adversary::depth_limit_reached_keys(keys, first, nth, n),
                (int)nth_adversary::sel_matches_std(keys, first, nth, n));
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 5 && std::strcmp(argv[1], "gen") == 0) {
        const int n = std::atoi(argv[2]), first = std::atoi(argv[3]), nth = std::atoi(argv[4]);
        const bool mirrored = argc > 5 ? std::atoi(argv[5]) != 0 : true;
        if (n < 1 || first < 0 || nth < first || nth >= n) {
            std::fprintf(stderr, "need 0 <= first <= nth < n\n");
            return 2;
        }
        const std::vector<int> v = nth_adversary::sequence(n, first, nth, mirrored);
        for (int i = 0; i < n; i++) std::printf(i ? " %d" : "%d", v[(size_t)i]);
        std::printf("\n");
        return status(v, first, nth);
    }
    if (argc >= 5 && std::strcmp(argv[1], "check") == 0) {
        const int first = std::atoi(argv[2]), nth = std::atoi(argv[3]);
        std::vector<float> keys;
        for (int i = 4; i < argc; i++) keys.push_back(std::strtof(argv[i], nullptr));
        return status(keys, first, nth);
    }
    std::fprintf(stderr, "usage: %s gen N FIRST NTH [MIRRORED] | check FIRST NTH K0 K1 ...\n", argv[0]);
    return 2;
}
