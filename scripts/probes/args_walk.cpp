// Build container: walks the argument check of the handle-free entry points (csrc/gclm_args.h) on the host, under sanitizers.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined,pointer-overflow -fno-sanitize-recover=all
//       scripts/probes/args_walk.cpp -o /tmp/args_walk && /tmp/args_walk
// The overlap predicate is compared with an oracle in 128-bit integers over every pair of ranges built from a set of
// starts (null, low addresses, the top of the address space) and byte counts (empty, one byte, abutting, nesting, counts
// that reach or pass the top); then the byte counts that saturate, the alignment rule and the write / read rules of ArgCheck.
// Prints one summary line; exit status 0 when every expectation held.
#include <cstdio>
#include <vector>

#include "../../geocalib_amd/csrc/gclm_args.h"

using namespace gclm;
typedef unsigned __int128 u128;

static long checks = 0, failed = 0;
#define EXPECT(c) do { ++checks; if (!(c)) { ++failed; std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

static const void* at(uintptr_t v) { return reinterpret_cast<const void*>(v); }

// the predicate without a word size: [a, a + n) and [b, b + m), ends cut at the top of the address space
static bool oracle(uintptr_t a, size_t n, uintptr_t b, size_t m) {
    if (!a || !b) return false;
    const u128 top = UINTPTR_MAX;
    u128 ea = (u128)a + n, eb = (u128)b + m;
    ea = ea > top ? top : ea;
    eb = eb > top ? top : eb;
    return (u128)a < eb && (u128)b < ea;
}

int main() {
    const uintptr_t T = UINTPTR_MAX;
    const std::vector<uintptr_t> starts = {0, 1, 2, 64, 100, 101, 127, 128, 129, 164, 4096, T - 4096, T - 129, T - 128, T - 64, T - 1, T};
    const std::vector<size_t> sizes = {0, 1, 2, 27, 28, 29, 63, 64, 65, 128, 4032, 4096, SIZE_MAX / 2, SIZE_MAX - 128, SIZE_MAX - 1, SIZE_MAX};
    long hits = 0;
    for (uintptr_t a : starts)
        for (size_t n : sizes)
            for (uintptr_t b : starts)
                for (size_t m : sizes) {
                    const bool got = ArgCheck::overlap(at(a), n, at(b), m);
                    EXPECT(got == oracle(a, n, b, m));
                    EXPECT(got == ArgCheck::overlap(at(b), m, at(a), n));
                    hits += got;
                }
    // the named cases: abutting, nesting, one shared byte, null, empty
    EXPECT(!ArgCheck::overlap(at(100), 28, at(128), 64));          // abut
    EXPECT(ArgCheck::overlap(at(100), 29, at(128), 64));           // share one byte
    EXPECT(ArgCheck::overlap(at(64), 4096, at(128), 1));           // nest
    EXPECT(!ArgCheck::overlap(nullptr, SIZE_MAX, at(128), 64));    // null names no range
    EXPECT(!ArgCheck::overlap(at(128), 0, at(128), 64));           // empty at the other's start
    EXPECT(ArgCheck::overlap(at(129), 0, at(128), 64));            // empty strictly inside: as the entries always answered
    EXPECT(!ArgCheck::overlap(at(128), 0, at(128), 0));
    EXPECT(ArgCheck::overlap(at(T - 64), SIZE_MAX, at(T - 1), 1)); // an end past the top stops there
    EXPECT(!ArgCheck::overlap(at(T - 64), 64, at(T), 1));          // ... and the last byte's end is the top itself

    // byte counts: exact below the top, SIZE_MAX from the first product that does not fit, 0 for an empty batch
    EXPECT(floats(2, 3, 48, 64) == (size_t)2 * 3 * 48 * 64 * 4);
    EXPECT(floats(0, 480, 640) == 0 && floats() == sizeof(float));
    EXPECT(floats(65535, 2147483647, 2147483647) == SIZE_MAX);
    EXPECT(floats((size_t)1 << 62) == SIZE_MAX && floats(((size_t)1 << 62) - 1) == SIZE_MAX - 3);
    EXPECT(floats(-1, 4, 4) == SIZE_MAX && floats(65535, 1 << 30, 1 << 30, 4, 0) == 0);
    EXPECT(mul_sat(SIZE_MAX, 1) == SIZE_MAX && mul_sat(SIZE_MAX, 2) == SIZE_MAX && mul_sat((size_t)1 << 32, (size_t)1 << 32) == SIZE_MAX);
    EXPECT(known_model(0) && known_model(3) && !known_model(-1) && !known_model(4));
    EXPECT(is_aligned(nullptr, 16) && is_aligned(at(32), 16) && !is_aligned(at(40), 16) && is_aligned(at(40), 8) && !is_aligned(at(41), 1 + 1));

    {   // written ranges keep off each other and off every read range; read ranges may share bytes
        ArgCheck a;
        a.writes(at(4096), 1024, 8);
        a.writes(nullptr, SIZE_MAX, 4);
        a.writes(at(8192), 1024, 4);
        a.reads(at(64), 4032);
        a.reads(at(64), 4032, 4);
        a.reads(at(5120), 3072);
        a.reads(nullptr, SIZE_MAX, 16);
        EXPECT(a.pass());
        ArgCheck b = a;
        b.reads(at(9215), 1);
        EXPECT(!b.pass());
        ArgCheck c = a;
        c.reads(at(64), 4033);
        EXPECT(!c.pass());
        ArgCheck d = a;
        d.reads(at(66), 2, 4);
        EXPECT(!d.pass());
        ArgCheck e = a;
        e.reads(at(16), floats(65535, 2147483647, 2147483647));
        EXPECT(!e.pass());
    }
    {   // two written ranges that share a byte; a misaligned write; a write after a read
        ArgCheck a, b, e;
        a.writes(at(4096), 1024);
        a.writes(at(5119), 1);
        b.writes(at(4100), 8, 8);
        e.reads(at(64), 8);
        e.writes(at(4096), 8);
        EXPECT(!a.pass() && !b.pass() && !e.pass());
        ArgCheck f;
        for (int i = 0; i < 5; ++i) f.writes(at(4096 + 64 * i), 64, 64);
        EXPECT(f.pass());
        f.writes(at(16384), 64);                                   // more written ranges than the object holds: refused
        EXPECT(!f.pass());
    }
    {   // ranges at the top of the address space
        ArgCheck a;
        a.writes(at(T - 4096), SIZE_MAX);
        a.reads(at(64), T - 4096 - 64);
        EXPECT(a.pass());
        a.reads(at(T - 1), 1);
        EXPECT(!a.pass());
    }
    std::printf("args_walk: %ld checks, %ld failed; %ld of %zu pairs overlap; sizeof(ArgCheck) = %zu\n", checks, failed, hits,
                starts.size() * sizes.size() * starts.size() * sizes.size(), sizeof(ArgCheck));
    return failed ? 1 : 0;
}
