// The layout of a device block, stated once: the piece workspaces, the kernel scratch (K3, K9, K10, K12, K15) and, under Stage
// (xc_stage.h), the staging arena of the host forms.  A launcher writes the blocks as one function lay(Carve) that takes them in order,
// fills the launcher's pointers and returns the carve's `at`, and runs it twice (lay_out, xc_capi.h): over Carve() to measure -- the total
// goes to grow(); every pointer comes back null, none is formed from the null base -- and over Carve(block) to place.  The bytes asked
// for and the bytes laid out are one statement.  Plain C++17, no HIP header (tests/test_carve_host.py runs it sanitized).
#pragma once
#include <stddef.h>

namespace xc {

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carve {                       // base == nullptr: measuring
    char* base; size_t at = 0;
    explicit Carve(void* b = nullptr) : base((char*)b) {}
    // n elements of T: every block is padded to a multiple of 256 bytes, so it starts 256-aligned; a block of no elements takes no bytes
    template <typename T> T* take(size_t n) { const size_t o = at; at += al(n * sizeof(T)); return base ? (T*)(base + o) : nullptr; }
    // with a later mark(): the bytes of the blocks taken between the two, padding included -- the length of one fill over all of them
    size_t mark() const { return at; }
};

}  // namespace xc
