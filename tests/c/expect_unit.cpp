// expect_unit.cpp -- CPU unit test of mirsha_expect_plan and
// mirsha::host::copy_kept_rows
// (mirbft_amd/csrc/mirsha_host.cpp, compiled here with g++: no HIP, no GPU):
// the bitmap and the per-word row bases of a mixed submission's expectations
// against a bit-by-bit restatement, guard entries behind both outputs, and
// the rejected index lists; the kept-rows walk of a retired mixed ticket
// against a row-by-row loop.  Prints "expect unit ok"; exit 1 with a message at
// the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "mirsha.h"
#include "mirsha_host.h"

static int fails = 0;
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
            fails++;                                             \
        }                                                        \
    } while (0)

static const uint64_t kGuard64 = 0xA5A5A5A5A5A5A5A5ull;
static const uint32_t kGuard32 = 0xA5A5A5A5u;

static void check(const std::vector<uint32_t>& of, uint32_t n, const char* what) {
    const uint32_t words = (uint32_t)(((uint64_t)n + 63u) >> 6);
    std::vector<uint64_t> has(words + 1, kGuard64);
    std::vector<uint32_t> base(words + 1, kGuard32);
    const int rc = mirsha_expect_plan(of.empty() ? nullptr : of.data(), (uint32_t)of.size(), n, has.data(), base.data());
    EXPECT(rc == MIRSHA_OK, "%s n=%u: rc %d", what, n, rc);
    EXPECT(has[words] == kGuard64 && base[words] == kGuard32, "%s n=%u: wrote past its outputs", what, n);
    std::vector<uint8_t> flag((size_t)words * 64, 0);
    for (uint32_t i : of) flag[i] = 1;
    uint32_t rows = 0;
    bool ok = true;
    for (uint32_t w = 0; w < words; w++) {
        ok &= base[w] == rows;
        for (uint32_t b = 0; b < 64; b++) {
            const bool set = (has[w] >> b) & 1u;
            ok &= set == (flag[(size_t)w * 64 + b] != 0);
            if (set) {  // the row formula the kernel uses
                const uint64_t below = has[w] & ((1ull << b) - 1ull);
                ok &= base[w] + (uint32_t)__builtin_popcountll(below) == rows && of[rows] == w * 64 + b;
                rows++;
            }
        }
    }
    EXPECT(ok && rows == of.size(), "%s n=%u: plan differs", what, n);
}

static void reject(const std::vector<uint32_t>& of, uint32_t n, const char* what) {
    const uint32_t words = (uint32_t)(((uint64_t)n + 63u) >> 6);
    std::vector<uint64_t> has(words + 1, kGuard64);
    std::vector<uint32_t> base(words + 1, kGuard32);
    const int rc = mirsha_expect_plan(of.data(), (uint32_t)of.size(), n, has.data(), base.data());
    EXPECT(rc == MIRSHA_EINVAL, "%s: rc %d, want MIRSHA_EINVAL", what, rc);
    EXPECT(has[words] == kGuard64 && base[words] == kGuard32, "%s: wrote past its outputs", what);
}

// mirsha::host::copy_kept_rows against a one-row-at-a-time loop.  Row i of src
// is filled with the byte i; dst holds exactly 32 n bytes (an overrun is the
// sanitizer's to see), pre-filled with a guard byte no row below 0xA5 equals,
// so both "row copied" and "row left alone" are checked for every i.
static const uint8_t kGuard8 = 0xA5;

static void kept(std::vector<uint64_t> has, std::vector<uint64_t> mis, uint32_t n, const char* what) {
    const uint32_t words = (uint32_t)(((uint64_t)n + 63u) >> 6);
    has.resize(words);
    mis.resize(words);
    uint8_t* src = (uint8_t*)malloc(32ull * n + 1);  // (+1: no zero-sized allocation)
    uint8_t* dst = (uint8_t*)malloc(32ull * n);
    for (uint32_t i = 0; i < n; i++) memset(src + 32ull * i, (int)i, 32);
    if (n) memset(dst, kGuard8, 32ull * n);
    mirsha::host::copy_kept_rows(has.data(), mis.data(), n, src, dst);
    uint32_t bad = n;
    for (uint32_t i = n; i-- > 0;) {
        const bool keep = ((~has[i >> 6] | mis[i >> 6]) >> (i & 63u)) & 1u;
        for (uint32_t b = 0; b < 32; b++)
            if (dst[32ull * i + b] != (keep ? (uint8_t)i : kGuard8)) bad = i;
    }
    EXPECT(bad == n, "copy_kept_rows %s n=%u: row %u", what, n, bad);
    free(src);
    free(dst);
}

// Bits [lo, hi] kept (has clear), every other one not (has set, no mismatch).
static std::vector<uint64_t> has_but(uint32_t lo, uint32_t hi) {
    std::vector<uint64_t> has(3, ~0ull);
    for (uint32_t i = lo; i <= hi; i++) has[i >> 6] &= ~(1ull << (i & 63u));
    return has;
}

static void kept_rows_cases() {
    std::mt19937_64 rng(11);
    const std::vector<uint64_t> none(3, 0ull), all(3, ~0ull), alt(3, 0x5555555555555555ull);
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 127u, 128u, 130u}) {  // (no row byte reaches the guard's 0xA5)
        kept(all, none, n, "nothing kept");
        kept(none, none, n, "everything kept (no expectation)");
        kept(all, all, n, "everything kept (every expectation wrong)");
        kept(alt, none, n, "alternating");
        kept(all, alt, n, "alternating mismatches");
        kept(has_but(60, 70), none, n, "a run from 60 to 70");
        kept(has_but(50, 63), none, n, "a run ending at 63");
        kept(has_but(64, 80), none, n, "a run starting at 64");
        kept(has_but(0, 129), none, n, "one run over every word");
        if (n) kept(has_but(n - 1, n - 1), none, n, "only the last row");
        if (n & 63u) {  // garbage at and above bit n of the last word is ignored
            const uint32_t w = n >> 6;
            const uint64_t above = ~0ull << (n & 63u);
            std::vector<uint64_t> has = all, mis = none;
            mis[w] |= above;
            kept(has, mis, n, "mismatch garbage above n");
            has[w] &= ~above;
            kept(has, none, n, "has clear above n");
            has = has_but(n - 1, n - 1);
            has[w] &= ~above;
            kept(has, mis, n, "the last row and garbage above n");
        }
        for (int k = 0; k < 200; k++) {
            std::vector<uint64_t> has(3), mis(3);
            for (int w = 0; w < 3; w++) {
                has[w] = rng() | (k % 3 ? rng() : 0ull);  // denser expectations: longer gaps between kept runs
                mis[w] = rng() & rng() & (k % 2 ? rng() : ~0ull);
            }
            kept(has, mis, n, "random");
        }
    }
}

int main() {
    kept_rows_cases();
    std::mt19937_64 rng(7);
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 128u, 1000u, 100003u, 600011u}) {  // the last: the parallel pass
        std::vector<uint32_t> full, alt, half;
        for (uint32_t i = 0; i < n; i++) {
            full.push_back(i);
            if (i % 2 == 0) alt.push_back(i);
            if (rng() & 1) half.push_back(i);
        }
        check({}, n, "empty");
        check(full, n, "full");
        check(alt, n, "alternating");
        check(half, n, "random half");
        if (n) check({0}, n, "only 0");
        if (n) check({n - 1}, n, "only n-1");
        if (n > 64) check({63, 64}, n, "63 and 64");
    }
    // no outputs are needed when there is no word
    EXPECT(mirsha_expect_plan(nullptr, 0, 0, nullptr, nullptr) == MIRSHA_OK, "n = 0 with NULL outputs");
    reject({3, 2}, 10, "not increasing");
    reject({2, 2}, 10, "duplicate index");
    reject({1, 10}, 10, "index == n");
    reject({0, 1, 2}, 2, "m > n");
    reject({0}, 0, "m > n = 0");
    {  // a bad index anywhere in a list long enough for the parallel pass
        std::vector<uint32_t> big(600011);
        for (uint32_t at : {0u, 37501u, 300000u, 600010u}) {
            for (uint32_t i = 0; i < big.size(); i++) big[i] = i;
            if (at) big[at] = big[at - 1];
            else big[0] = 1;  // equals big[1]
            reject(big, 600011, "duplicate in a long list");
            for (uint32_t i = 0; i < big.size(); i++) big[i] = i;
            big[at] = 600011;
            reject(big, 600011, "index == n in a long list");
        }
    }
    uint64_t h = 0;
    uint32_t b = 0;
    EXPECT(mirsha_expect_plan(nullptr, 1, 4, &h, &b) == MIRSHA_EINVAL, "NULL expect_of with m > 0");
    const uint32_t one = 0;
    EXPECT(mirsha_expect_plan(&one, 1, 4, nullptr, &b) == MIRSHA_EINVAL, "NULL has_out");
    EXPECT(mirsha_expect_plan(&one, 1, 4, &h, nullptr) == MIRSHA_EINVAL, "NULL base_out");
    if (fails) return 1;
    printf("expect unit ok\n");
    return 0;
}
