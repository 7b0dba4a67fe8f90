// carve.h on the CPU: for a few layouts (zero-count arrays, odd element sizes,
// counts that end on and off a 256-byte boundary) the sizing pass over a null
// base gives the total at which the pass over a real buffer ends, every array
// starts on a 256-byte boundary inside the buffer, and consecutive arrays do
// not overlap.  Every byte of every array is written, so the sanitizers this is
// built with see a total that is too small.  The same for every layout of
// host_layouts.h (the library's host scratch), at 0, 1, 63, 64 and 65 elements.
// Prints "ok"; exit code 1 and a line per failure otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "carve.h"
#include "host_layouts.h"

using livo::Carve;

struct Odd3 {
    char b[3];
};
struct Odd20 {
    float f[5];
};
struct Span {
    const char* p;
    size_t bytes;
};

static int failures = 0;
static void fail(const char* layout, const char* what, size_t k) {
    std::printf("%s: %s (array %zu)\n", layout, what, k);
    failures++;
}

template <class T>
static void take(Carve& k, size_t count, std::vector<Span>& out) {
    T* p = k.take<T>(count);
    out.push_back({reinterpret_cast<const char*>(p), count * sizeof(T)});
    if (p) std::memset(p, 0x5A, count * sizeof(T));
}

// One layout, written once and run twice, as the frame stages do.
typedef void (*Layout)(Carve&, std::vector<Span>&);

static void mixed(Carve& k, std::vector<Span>& s) {
    take<float>(k, 5 * 65, s);
    take<double>(k, 22, s);
    take<uint8_t>(k, 0, s);  // an empty array takes no room but keeps its boundary
    take<Odd3>(k, 7, s);
    take<uint32_t>(k, 64, s);  // exactly 256 bytes
    take<uint32_t>(k, 65, s);
    take<Odd20>(k, 13, s);
    take<unsigned long long>(k, 4, s);
}
static void empty(Carve&, std::vector<Span>&) {}
static void zeros(Carve& k, std::vector<Span>& s) {
    take<float>(k, 0, s);
    take<Odd3>(k, 0, s);
}
static void single(Carve& k, std::vector<Span>& s) { take<uint8_t>(k, 1, s); }
static void bytes(Carve& k, std::vector<Span>& s) {
    take<uint8_t>(k, 255, s);
    take<uint8_t>(k, 256, s);
    take<uint8_t>(k, 257, s);
    take<Odd3>(k, 85, s);  // 255 bytes
    take<Odd3>(k, 86, s);  // 258 bytes
}

static void check(const char* name, Layout layout) {
    std::vector<Span> sized, real;
    Carve a{nullptr};
    layout(a, sized);
    const size_t total = a.total();
    for (size_t k = 0; k < sized.size(); k++)
        if (sized[k].p) fail(name, "the sizing pass returned a pointer", k);
    if (total % 256) fail(name, "the total is no multiple of 256", 0);
    // exactly `total` bytes on a 256-byte boundary: a write past them is the sanitizer's to report
    char* buf = static_cast<char*>(std::aligned_alloc(256, total ? total : 256));
    if (!buf) std::exit(2);
    Carve b{buf};
    layout(b, real);
    if (b.total() != total) fail(name, "the two passes end at different offsets", real.size());
    const char* end = buf;
    for (size_t k = 0; k < real.size(); k++) {
        const Span& s = real[k];
        if (!s.p) fail(name, "null from a real base", k);
        if (reinterpret_cast<uintptr_t>(s.p) % 256) fail(name, "not 256-byte aligned", k);
        if (s.p < end) fail(name, "overlaps the array before it", k);
        if (s.p + s.bytes > buf + total) fail(name, "ends past the total", k);
        if (s.bytes != sized[k].bytes) fail(name, "sizes differ between the passes", k);
        end = s.p + s.bytes;
    }
    std::free(buf);
}

// The layouts of host_layouts.h at g_n elements: each array of the returned
// struct in the order the layout takes it (aliases are no arrays of their own;
// null in the sizing pass, as take returns it).
static size_t g_n = 0;
template <class T>
static void got(T* p, size_t count, std::vector<Span>& out) {
    out.push_back({reinterpret_cast<const char*>(p), count * sizeof(T)});
    if (p) std::memset(p, 0x5A, count * sizeof(T));
}
static void run_build(Carve& k, std::vector<Span>& s, bool ball) {
    const size_t n = g_n;
    const livo::RunBuild L = livo::run_build_layout(k, n, ball);
    got(L.rho, n, s);
    got(L.iota, n, s);
    got(L.srho, n, s);
    got(L.e1, n, s);
    got(L.e2, n, s);
    got(L.heads, n, s);
    got(L.starts, n + 1, s);
    got(L.keys, n, s);
    got(L.skeys, n, s);
    got(L.nruns, 1, s);
    if (ball) {
        got(L.pt, n, s);
        got(L.key1, n, s);
        got(L.plen, n + 1, s);
        if (L.runid != L.rho || L.pstart != L.srho) fail("run_build_ball", "an alias moved", 0);
    } else {
        got(L.runid, n, s);
        if (L.plen != L.rho || L.pstart != L.iota || L.pt || L.key1) fail("run_build_cell", "an alias moved", 0);
    }
}
static void run_build_cell(Carve& k, std::vector<Span>& s) { run_build(k, s, false); }
static void run_build_ball(Carve& k, std::vector<Span>& s) { run_build(k, s, true); }
static void scan_build(Carve& k, std::vector<Span>& s, size_t bound_words) {
    const livo::ScanBuild L = livo::scan_build_layout(k, g_n, bound_words);
    got(L.keys, g_n, s);
    got(L.skeys, g_n, s);
    got(L.iota, g_n, s);
    got(L.svals, g_n, s);
    got(L.bounds, bound_words, s);
}
static void scan_build_one(Carve& k, std::vector<Span>& s) { scan_build(k, s, 6); }
static void scan_build_batch(Carve& k, std::vector<Span>& s) { scan_build(k, s, 6 * 16); }
static void scan_upload(Carve& k, std::vector<Span>& s) {
    const livo::ScanUpload L = livo::scan_upload_layout(k, g_n, true);
    got(L.build.keys, g_n, s);
    got(L.build.skeys, g_n, s);
    got(L.build.iota, g_n, s);
    got(L.build.svals, g_n, s);
    got(L.build.bounds, 6, s);
    got(L.src, g_n * 3, s);
}
struct Rec64 {  // (the size of a neighbour record)
    char b[64];
};
static void knn_query(Carve& k, std::vector<Span>& s) {
    const livo::KnnQuery<Rec64> L = livo::knn_query_layout<Rec64>(k, g_n);
    got(L.q, g_n * 4, s);
    got(L.rec, g_n, s);
}
static void plane_tmp(Carve& k, std::vector<Span>& s) {
    const livo::PlaneTmp L = livo::plane_tmp_layout(k, g_n);
    got(L.plane, g_n * 4, s);
    got(L.pstate, g_n, s);
}
static void hshare_dbg(Carve& k, std::vector<Span>& s, bool ori) {
    const livo::HShareDbg L = livo::hshare_dbg_layout(k, g_n, ori);
    got(L.normvec, g_n * 4, s);
    got(L.world, g_n * 3, s);
    got(L.sel, g_n, s);
    if (ori) {
        got(L.flags, g_n, s);
        got(L.pos, g_n, s);
        got(L.ori, g_n * 3, s);
        got(L.corr, g_n * 4, s);
    } else if (L.flags || L.pos || L.ori || L.corr) {
        fail("hshare_dbg", "an array that was not asked for", 0);
    }
}
static void hshare_dbg_plain(Carve& k, std::vector<Span>& s) { hshare_dbg(k, s, false); }
static void hshare_dbg_ori(Carve& k, std::vector<Span>& s) { hshare_dbg(k, s, true); }
static void map_incr(Carve& k, std::vector<Span>& s) {
    const livo::MapIncr L = livo::map_incr_layout(k, g_n);
    got(L.ordered, 2 * g_n * 4, s);
    got(L.flags, 2 * g_n, s);
    got(L.pos, 2 * g_n, s);
    got(L.cat, g_n, s);
}

int main() {
    check("mixed", mixed);
    check("empty", empty);
    check("zeros", zeros);
    check("single", single);
    check("bytes", bytes);
    const struct {
        const char* name;
        Layout layout;
    } host[] = {{"run_build_cell", run_build_cell}, {"run_build_ball", run_build_ball},
                {"scan_build_one", scan_build_one}, {"scan_build_batch", scan_build_batch},
                {"scan_upload", scan_upload},       {"knn_query", knn_query},
                {"plane_tmp", plane_tmp},           {"hshare_dbg_plain", hshare_dbg_plain},
                {"hshare_dbg_ori", hshare_dbg_ori}, {"map_incr", map_incr}};
    // 63, 64, 65: a 4-byte array ends just before, on and just after a 256-byte boundary
    for (const size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65}) {
        g_n = n;
        for (const auto& h : host) check(h.name, h.layout);
        // carve_bytes, which the library allocates by, is the sizing pass
        Carve a{nullptr};
        livo::run_build_layout(a, n, true);
        if (livo::carve_bytes(livo::run_build_layout, n, true) != a.total()) fail("carve_bytes", "not the sizing pass", n);
    }
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
