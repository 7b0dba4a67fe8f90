// nth_adversary.h — inputs that drive libstdc++'s std::nth_element to its
// introselect depth limit (2 floor(log2 n) rounds, then __heap_select), built
// against libstdc++ itself, and a predicate that says whether a given input
// gets there.  Host only, header only.
//
// The generator is McIlroy's adversary ("A Killer Adversary for Quicksort",
// 1999): std::nth_element runs on items whose values are undecided ("gas")
// until a comparison forces one; the comparator then freezes the item the
// algorithm is about to use as its pivot at an extreme value, so every
// partition cuts off only the pivot and a neighbour or two.  The original
// hands frozen values out from the bottom up (gas compares above everything),
// which keeps the pivot at the low end: the range shrinks from `first`, and
// the limit is only reached when nth is far from first.  Every long selection
// of the iVox search has nth = first + 4 (the 5 smallest), which needs the
// mirror image: gas compares BELOW every frozen value and frozen values are
// handed out from the top down, so the pivot lands near the top and the range
// shrinks from `last` one or two elements a round.
//
// The values are distinct, so replaying the finished sequence through any
// faithful nth_element takes exactly the comparisons the adversary answered.
#pragma once
#include <algorithm>
#include <vector>

#include "stl_select.h"

namespace nth_adversary {

// A permutation of the ranks 0..n-1: position i holds the rank of the i-th
// element.  std::nth_element(a + first, a + nth, a + n) on it is adversarial;
// positions before `first` take ranks the range does not use.  mirrored: the
// pivot is driven to the top (for nth near first); else to the bottom (for nth
// near n).
inline std::vector<int> sequence(int n, int first, int nth, bool mirrored = true) {
    struct State {
        std::vector<int> val;  // -1: gas
        int next, step, candidate;
        bool mirrored;
    } s{std::vector<int>((size_t)n, -1), mirrored ? n - 1 : 0, mirrored ? -1 : 1, -1, mirrored};
    auto freeze = [&s](int x) {
        s.val[(size_t)x] = s.next;
        s.next += s.step;
    };
    auto less = [&s, &freeze](int x, int y) {
        const bool gx = s.val[(size_t)x] < 0, gy = s.val[(size_t)y] < 0;
        if (gx && gy) freeze(x == s.candidate ? x : y);
        if (s.val[(size_t)x] < 0)
            s.candidate = x;
        else if (s.val[(size_t)y] < 0)
            s.candidate = y;
        const bool x_gas = s.val[(size_t)x] < 0, y_gas = s.val[(size_t)y] < 0;
        if (x_gas || y_gas) {
            // gas against frozen (never gas against gas here): mirrored, gas is the smaller
            return s.mirrored ? x_gas : y_gas;
        }
        return s.val[(size_t)x] < s.val[(size_t)y];
    };
    std::vector<int> items((size_t)n);
    for (int i = 0; i < n; i++) items[(size_t)i] = i;
    if (n > 0 && first >= 0 && first <= nth && nth < n)
        std::nth_element(items.begin() + first, items.begin() + nth, items.end(), less);
    // what stayed gas (and the positions outside the range) takes the ranks left over, in position
    // order: all of them on the side of every frozen value that the comparator answered with
    std::vector<char> used((size_t)n, 0);
    for (int i = 0; i < n; i++)
        if (s.val[(size_t)i] >= 0) used[(size_t)s.val[(size_t)i]] = 1;
    int r = 0;
    for (int i = 0; i < n; i++) {
        if (s.val[(size_t)i] >= 0) continue;
        while (used[(size_t)r]) r++;
        s.val[(size_t)i] = r++;
    }
    return s.val;
}

// Introselect's rounds replayed on keys a[first, last) with the public pieces
// of stl_select.h: true when depth == 0 is met before last - first <= 3, which
// is where libstdc++ switches to __heap_select.  (first, last) at that moment
// are returned through lo / hi when given.
inline bool depth_limit_reached(std::vector<livo::SelElem> a, int first, int nth, int last, int* lo = nullptr,
                                int* hi = nullptr) {
    if (first == last || nth == last) return false;
    int depth = 2 * livo::sel_lg(last - first);
    while (last - first > 3) {
        if (depth == 0) {
            if (lo) *lo = first;
            if (hi) *hi = last;
            return true;
        }
        --depth;
        const int mid = first + (last - first) / 2;
        livo::sel_move_median_to_first(a, first, first + 1, mid, last - 1);
        const int cut = livo::sel_unguarded_partition(a, first + 1, last, first);
        if (cut <= nth)
            first = cut;
        else
            last = cut;
    }
    return false;
}

template <class K>
inline bool depth_limit_reached_keys(const std::vector<K>& keys, int first, int nth, int last) {
    std::vector<livo::SelElem> a(keys.size());
    for (size_t i = 0; i < keys.size(); i++) a[i] = livo::SelElem{(float)keys[i], (uint32_t)i};
    return depth_limit_reached(a, first, nth, last);
}

// sel_nth_element against std::nth_element on the same keys (ids = positions), element for element.
template <class K>
inline bool sel_matches_std(const std::vector<K>& keys, int first, int nth, int last) {
    struct DP {
        float d;
        uint32_t id;
        bool operator<(const DP& o) const { return d < o.d; }
    };
    std::vector<DP> ref(keys.size());
    std::vector<livo::SelElem> dev(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        ref[i] = DP{(float)keys[i], (uint32_t)i};
        dev[i] = livo::SelElem{(float)keys[i], (uint32_t)i};
    }
    std::nth_element(ref.begin() + first, ref.begin() + nth, ref.begin() + last);
    livo::sel_nth_element(dev, first, nth, last);
    for (size_t i = 0; i < keys.size(); i++)
        if (dev[i].id != ref[i].id || dev[i].d != ref[i].d) return false;
    return true;
}

}  // namespace nth_adversary
