// expect_unit.cpp -- CPU unit test of mirsha_expect_plan
// (mirbft_amd/csrc/mirsha_host.cpp, compiled here with g++: no HIP, no GPU):
// the bitmap and the per-word row bases of a mixed submission's expectations
// against a bit-by-bit restatement, guard entries behind both outputs, and
// the rejected index lists.  Prints "expect unit ok"; exit 1 with a message at
// the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "mirsha.h"

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

int main() {
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
