// carve.h on the CPU: for a few layouts (zero-count arrays, odd element sizes,
// counts that end on and off a 256-byte boundary) the sizing pass over a null
// base gives the total at which the pass over a real buffer ends, every array
// starts on a 256-byte boundary inside the buffer, and consecutive arrays do
// not overlap.  Every byte of every array is written, so the sanitizers this is
// built with see a total that is too small.  Prints "ok"; exit code 1 and a
// line per failure otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "carve.h"

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

int main() {
    check("mixed", mixed);
    check("empty", empty);
    check("zeros", zeros);
    check("single", single);
    check("bytes", bytes);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
