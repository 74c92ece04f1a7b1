// gclm_args.h -- the one argument check of the entry points that take no handle (gclm_entry.hip).  Host code over
// include/gclm.h alone: no HIP header, no HIP call, no allocation (several of those entries sit on the 10 us single-image
// path), so a plain host compiler builds it and a stand-alone program walks it under a sanitizer (scripts/probes/args_walk.cpp).
//
// An entry returns on its plain conditions (the camera model among them: known_model), then states the ranges the call
// WRITES, then the ranges it READS, each as pointer, byte count and required alignment, and asks pass(): every non-null
// pointer is aligned, and every written range shares no byte with a read range or with another written range.  A null
// pointer names no range.
// Ranges are compared as integers -- no arithmetic on the caller's pointers -- and neither a byte count (floats) nor the end
// of a range wraps: both stop at the top of the address space.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gclm.h"

namespace gclm {

inline bool known_model(int camera_model) { return camera_model >= GCLM_PINHOLE && camera_model <= GCLM_SIMPLE_DIVISIONAL; }

inline bool is_aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }     // (null is aligned)

// a * b, or SIZE_MAX once the product no longer fits
inline size_t mul_sat(size_t a, size_t b) {
    size_t r;
    return __builtin_mul_overflow(a, b, &r) ? SIZE_MAX : r;
}

// Bytes of n0 * n1 * ... elements of type T.  A negative factor counts as a huge one: the entry refuses it by a condition of
// its own.
template <typename T, typename... N>
size_t elements(N... n) {
    size_t r = sizeof(T);
    ((r = mul_sat(r, (size_t)n)), ...);
    return r;
}

// ... of floats, which is what nearly every range holds.
template <typename... N>
size_t floats(N... n) {
    return elements<float>(n...);
}

// (GCLM_ARGS_INLINE: left to itself the compiler keeps writes() out of line, and the ranges then live in memory -- three times
// the cost of a call's checks)
#define GCLM_ARGS_INLINE __attribute__((always_inline))

class ArgCheck {
public:
    // A range the call writes: disjoint from every range registered before it.  Every write comes before the first read
    // (a write after a read refuses the call, whatever its arguments: no test of the entry would pass).
    GCLM_ARGS_INLINE void writes(const void* p, size_t bytes, size_t align = 1) {
        const Range r = check(p, bytes, align);
        if (!sealed_ && n_ < kMaxWrites) w_[n_++] = r; else ok_ = false;
    }
    // A range the call reads: disjoint from every written range; read ranges may share bytes with each other.  Not stored,
    // so a call may read any number of them (gclm_render_from_pano: one per source).
    GCLM_ARGS_INLINE void reads(const void* p, size_t bytes, size_t align = 1) {
        sealed_ = true;
        check(p, bytes, align);
    }
    bool pass() const { return ok_; }

    // Do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  (An empty range strictly inside the other one does.)
    static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
        return span(a, a_bytes).hits(span(b, b_bytes));
    }

private:
    struct Range {                            // [lo, hi)
        uintptr_t lo, hi;
        bool hits(const Range& o) const { return lo < o.hi && o.lo < hi; }
    };
    static constexpr int kMaxWrites = 5;      // gclm_pack_fields_bins: up, latitude, two confidences and sin(latitude)
    Range w_[kMaxWrites];
    int n_ = 0;
    bool ok_ = true, sealed_ = false;

    // [p, p + bytes), the end stopping at the top of the address space; a null pointer names the range that hits nothing
    static Range span(const void* p, size_t bytes) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        return {lo, !p ? 0 : (bytes > UINTPTR_MAX - lo ? UINTPTR_MAX : lo + bytes)};
    }
    // one range against its alignment and the written ranges (stored unconditionally, nulls too: after inlining their count
    // is a constant and the whole check stays in registers)
    GCLM_ARGS_INLINE Range check(const void* p, size_t bytes, size_t align) {
        const Range r = span(p, bytes);
        if (!ok_) return r;                   // (refused already: the rest of the call's ranges cost nothing)
        if (!is_aligned(p, align)) ok_ = false;
        for (int i = 0; i < n_; ++i)
            if (r.hits(w_[i])) ok_ = false;
        return r;
    }
};

}  // namespace gclm
