// upload_plan.h on the CPU.  upload_pass, the split of livo_scan_upload_batch_async's
// scans into build passes: scan counts, offsets, totals, largest scan and sort
// key bits against a straightforward recomputation; passes of empty scans; the
// 32-bit position limit on both sides.  scan_buf_bytes, the bytes of a scan's
// nine device arrays as scan_arrays lists them: equal to the formula the spare
// pool's budget was written by, at capacities around a block edge.
// Prints "ok"; exit code 1 and a line per failure otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

// (livo_internal.h, from which upload_plan.h takes its constants, names one HIP
// type: a pointer member of a kernel argument table that nothing here touches)
struct uint4;
#include "upload_plan.h"

using namespace livo;

static int failures = 0;
static void fail(const char* what, long long k) {
    std::printf("%s (%lld)\n", what, k);
    failures++;
}

// The passes of sizes N, each field recomputed the plain way.
static void check_split(const std::vector<int64_t>& N) {
    const int32_t n = (int32_t)N.size();
    for (int32_t b0 = 0; b0 < n; b0 += kFeSegMax) {
        UploadPass P;
        if (upload_pass(N.data(), n, b0, &P) != LIVO_OK) fail("a small pass is refused", b0);
        const int32_t m = n - b0 < kFeSegMax ? n - b0 : kFeSegMax;
        if (P.m != m) fail("scans in the pass", b0);
        int64_t tot = 0, max_n = 0;
        for (int32_t b = 0; b < m; b++) {
            if (P.off[b] != tot) fail("offset of scan", b0 + b);
            tot += N[(size_t)(b0 + b)];
            if (N[(size_t)(b0 + b)] > max_n) max_n = N[(size_t)(b0 + b)];
        }
        if (P.tot != tot) fail("total of the pass", b0);
        if (P.max_n != max_n) fail("largest scan of the pass", b0);
    }
}

static int key_bits(int32_t m) {
    const std::vector<int64_t> N((size_t)m, 1000);
    UploadPass P;
    if (upload_pass(N.data(), m, 0, &P) != LIVO_OK) fail("a small pass is refused", m);
    return P.key_bits;
}

int main() {
    // 18 ragged scans: 16 + 2
    std::vector<int64_t> N = {60000, 1, 40000, 0, 257, 30000, 5, 12345};
    for (int s = 0; s < 10; s++) N.push_back(20000 + 1000 * s);
    check_split(N);
    UploadPass P;
    upload_pass(N.data(), 18, 0, &P);
    if (P.m != 16) fail("the first pass holds 16 scans", P.m);
    upload_pass(N.data(), 18, 16, &P);
    if (P.m != 2 || P.off[0] != 0 || P.off[1] != 28000 || P.tot != 28000 + 29000 || P.max_n != 29000)
        fail("the second pass holds the last 2 scans", P.m);

    // 27 Morton bits and the scan index's
    if (key_bits(1) != 27) fail("key bits of 1 scan", key_bits(1));
    if (key_bits(2) != 28) fail("key bits of 2 scans", key_bits(2));
    if (key_bits(3) != 29) fail("key bits of 3 scans", key_bits(3));
    if (key_bits(16) != 31) fail("key bits of 16 scans", key_bits(16));

    // empty scans only: nothing to build, and no range error; then a pass that is not empty
    std::vector<int64_t> E(20, 0);
    E[17] = 9;
    if (upload_pass(E.data(), 20, 0, &P) != LIVO_OK || P.tot != 0 || P.max_n != 0 || P.m != 16) fail("an empty pass", 0);
    if (upload_pass(E.data(), 20, 16, &P) != LIVO_OK || P.tot != 9 || P.off[1] != 0 || P.off[2] != 9 || P.m != 4)
        fail("the pass after an empty one", 16);
    check_split(E);

    // 32-bit positions in the batch sort: 2^32 points are too many, 2^32 - 1 - kBlock are not
    const int64_t two32 = (int64_t)1 << 32;
    std::vector<int64_t> R(4, two32 / 4);
    if (upload_pass(R.data(), 4, 0, &P) != LIVO_E_RANGE) fail("2^32 points are accepted", 0);
    R[3] -= 1 + kBlock;
    if (upload_pass(R.data(), 4, 0, &P) != LIVO_OK || P.tot != two32 - 1 - kBlock) fail("2^32 - 1 - kBlock points are refused", 0);
    R[0] += 1;
    if (upload_pass(R.data(), 4, 0, &P) != LIVO_E_RANGE) fail("2^32 - kBlock points are accepted", 0);

    // a scan's bytes: the enumeration against the formula, written out
    const int64_t edge = (int64_t)kBlock * kPtsPerThread;
    for (const int64_t cap : {(int64_t)0, (int64_t)1, edge - 1, edge + 1, (int64_t)100000}) {
        const int64_t blocks = (cap + kBlock * kPtsPerThread - 1) / (kBlock * kPtsPerThread);
        const int64_t cblk = blocks < 1 ? 1 : blocks;
        // partial doubles: kIkCols per block of the plane pass or kRedCols per block of the fused evaluation
        const int64_t eblocks = (cap + kEvalBlock - 1) / kEvalBlock;
        const int64_t pa = cblk * kIkCols, pb = (eblocks < 1 ? 1 : eblocks) * kRedCols;
        const size_t pd = (size_t)(pa > pb ? pa : pb);
        if (partial_doubles(cap) != pd) fail("partial_doubles at capacity", cap);
        const size_t want = (size_t)cap * (16 + sizeof(NNRec) + 4 + 4 + 16 + 1) + pd * 8 +
                            (size_t)cblk * (kIkFewRows * 13 * 8 + 4);
        if (scan_buf_bytes(cap) != want) fail("scan_buf_bytes differs from the formula at capacity", cap);
        // and the list itself: nine arrays, none listed twice
        ScanArrays s;
        std::vector<void*> seen;
        scan_arrays(s, cap, [&](auto*& p, size_t) { seen.push_back((void*)&p); });
        if (seen.size() != 9) fail("a scan has nine arrays", (long long)seen.size());
        for (size_t a = 0; a < seen.size(); a++)
            for (size_t b = a + 1; b < seen.size(); b++)
                if (seen[a] == seen[b]) fail("an array is listed twice", (long long)a);
    }
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
