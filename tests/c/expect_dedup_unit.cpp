// expect_dedup_unit.cpp -- CPU unit test of the host-only plan code of the
// deduplicated mixed submission (mirbft_amd/csrc/mirsha_host.cpp, compiled here
// with g++: no HIP, no GPU): mirsha_dedup_rows against a byte-for-byte
// restatement on ragged slice lists (empty requests, empty slices, requests
// that differ only in their slicing), a guard entry behind its output, its
// rejected arguments, mirsha::host::dedup_rows over hand-made launches, and the
// row formula of the select kernel over mirsha_expect_plan for the same cycle.
// Prints "expect dedup unit ok"; exit 1 with a message at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
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

static const uint32_t kGuard = 0xA5A5A5A5u;

// A cycle as slice arrays over heap copies of its bytes (each slice its own
// allocation, so that the sanitizer sees every read past a slice).
struct Cycle {
    std::vector<std::vector<std::string>> reqs;
    std::vector<std::vector<uint8_t>> store;
    std::vector<const uint8_t*> ptr;
    std::vector<uint64_t> len;
    std::vector<uint32_t> first;
    void build() {
        store.clear(), ptr.clear(), len.clear(), first.assign(1, 0u);
        for (const auto& r : reqs)
            for (const auto& s : r) store.emplace_back(s.begin(), s.end());
        size_t k = 0;
        for (const auto& r : reqs) {
            for (size_t j = 0; j < r.size(); j++, k++) {
                ptr.push_back(store[k].empty() ? nullptr : store[k].data());
                len.push_back(store[k].size());
            }
            first.push_back((uint32_t)ptr.size());
        }
    }
    std::string blob(size_t i) const {
        std::string b;
        for (const auto& s : reqs[i]) b += s;
        return b;
    }
};

static Cycle random_cycle(uint64_t seed, uint32_t n, uint32_t contents) {
    std::mt19937_64 rng(seed);
    std::vector<std::string> pool;
    for (uint32_t c = 0; c < contents; c++) {
        std::string b((size_t)(rng() % 200), '\0');
        for (auto& ch : b) ch = (char)rng();
        pool.push_back(b);
    }
    pool.push_back("");                                  // the empty content
    pool.push_back(pool[0] + "x");                       // a prefix relation
    pool.push_back(pool[1].empty() ? "y" : pool[1]);     // same length as pool[1], one byte apart
    if (!pool.back().empty()) pool.back().back() ^= 1;
    Cycle cy;
    for (uint32_t i = 0; i < n; i++) {
        const std::string& b = pool[rng() % pool.size()];
        std::vector<std::string> parts;
        size_t at = 0;
        const uint32_t cuts = (uint32_t)(rng() % 4);  // 0: no slice at all when the content is empty
        for (uint32_t c = 0; c < cuts && at < b.size(); c++) {
            const size_t k = rng() % (b.size() - at + 1);
            parts.push_back(b.substr(at, k));  // may be an empty slice
            at += k;
        }
        if (at < b.size() || (cuts && parts.empty())) parts.push_back(b.substr(at));
        cy.reqs.push_back(parts);
    }
    cy.build();
    return cy;
}

static void check(const Cycle& cy, const char* what) {
    const uint32_t n = (uint32_t)cy.reqs.size();
    std::vector<uint32_t> row(n + 1, kGuard), rep(n + 1, kGuard);
    uint32_t unique = kGuard, unique2 = kGuard;
    const int rc = mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), cy.first.data(), n, row.data(), &unique);
    EXPECT(rc == MIRSHA_OK, "%s: rc %d", what, rc);
    EXPECT(mirsha_dedup_plan(cy.ptr.data(), cy.len.data(), cy.first.data(), n, rep.data(), &unique2) == MIRSHA_OK,
           "%s: dedup_plan", what);
    EXPECT(row[n] == kGuard, "%s: wrote past row_out", what);
    std::map<std::string, uint32_t> where;  // content -> its row: first appearance takes the next one (one segment)
    bool ok = true;
    for (uint32_t i = 0; i < n; i++) {
        const auto it = where.emplace(cy.blob(i), (uint32_t)where.size()).first;
        ok &= row[i] == it->second && row[i] == row[rep[i]] && row[i] < unique;
    }
    EXPECT(ok, "%s: rows differ from the restatement", what);
    EXPECT(unique == where.size() && unique2 == unique, "%s: %u distinct, want %zu", what, unique, where.size());
}

int main() {
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 131u, 1000u})
        for (uint32_t contents : {1u, 9u, 400u}) {
            char what[64];
            snprintf(what, sizeof what, "n=%u contents=%u", n, contents);
            check(random_cycle(n * 131u + contents, n, contents), what);
        }
    {  // slicing does not matter; empty requests of every shape share a row
        Cycle cy;
        cy.reqs = {{"ab", "c"}, {"abc"}, {""}, {"a", "bc"}, {}, {"xyz"}, {"abd"}, {"", "abc", ""}, {"", ""}};
        cy.build();
        check(cy, "slicings");
        std::vector<uint32_t> row(9);
        uint32_t u = 0;
        mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), cy.first.data(), 9, row.data(), &u);
        const std::vector<uint32_t> want{0, 0, 1, 0, 1, 2, 3, 0, 1};
        EXPECT(row == want && u == 4, "slicings: rows");
    }
    {  // arguments
        Cycle cy;
        cy.reqs = {{"abc"}, {"abc"}, {"d"}};
        cy.build();
        std::vector<uint32_t> row(4, kGuard);
        uint32_t u = kGuard;
        EXPECT(mirsha_dedup_rows(nullptr, nullptr, nullptr, 0, nullptr, &u) == MIRSHA_OK && u == 0, "n = 0");
        EXPECT(mirsha_dedup_rows(nullptr, nullptr, nullptr, 0, nullptr, nullptr) == MIRSHA_OK, "n = 0, no count");
        EXPECT(mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), cy.first.data(), 3, row.data(), nullptr) == MIRSHA_OK &&
                   row[0] == 0 && row[1] == 0 && row[2] == 1 && row[3] == kGuard,
               "NULL n_unique_out");
        EXPECT(mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), cy.first.data(), 3, nullptr, &u) == MIRSHA_EINVAL,
               "NULL row_out");
        EXPECT(mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), nullptr, 3, row.data(), &u) == MIRSHA_EINVAL,
               "NULL slice_first");
        EXPECT(mirsha_dedup_rows(nullptr, cy.len.data(), cy.first.data(), 3, row.data(), &u) == MIRSHA_EINVAL,
               "NULL slice_ptr with slices");
        std::vector<uint32_t> bad = cy.first;
        bad[0] = 1;
        EXPECT(mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), bad.data(), 3, row.data(), &u) == MIRSHA_EINVAL,
               "slice_first[0] != 0");
        bad = cy.first;
        bad[1] = 3, bad[2] = 2;
        EXPECT(mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), bad.data(), 3, row.data(), &u) == MIRSHA_EINVAL,
               "slice_first not monotone");
        std::vector<const uint8_t*> holes = cy.ptr;
        holes[2] = nullptr;
        EXPECT(mirsha_dedup_rows(holes.data(), cy.len.data(), cy.first.data(), 3, row.data(), &u) == MIRSHA_EINVAL,
               "a NULL slice with bytes");
    }
    {  // mirsha::host::dedup_rows: two launches, a collision appended behind the later heads
        // requests:      0  1  2  3  4  5  6  7
        // contents:      A  B  A  C  B  D  C  D      first segment = [0, 3)
        const std::vector<uint32_t> rep{0, 1, 0, 3, 1, 5, 3, 5}, heads0{0, 1}, later{5, 3};
        std::vector<uint32_t> row(9, kGuard);
        const bool identity = mirsha::host::dedup_rows(rep.data(), heads0, later, 8, row.data());
        const std::vector<uint32_t> want{0, 1, 0, 3, 1, 2, 3, 2, kGuard};
        EXPECT(!identity && row == want, "two launches");
        const std::vector<uint32_t> rep2{0, 1, 2, 3}, h2{0, 1}, l2{2, 3};
        std::vector<uint32_t> row2(4, kGuard);
        EXPECT(mirsha::host::dedup_rows(rep2.data(), h2, l2, 4, row2.data()) && row2 == rep2, "identity");
        const std::vector<uint32_t> l3{3, 2};  // all distinct, but the second launch is out of origin order
        EXPECT(!mirsha::host::dedup_rows(rep2.data(), h2, l3, 4, row2.data()) && row2[2] == 3 && row2[3] == 2,
               "a permutation is not the identity");
    }
    {  // what the select kernel reads for lane i: digest row row[i], expectation row base + popcount
        const Cycle cy = random_cycle(77, 131, 9);
        const uint32_t n = 131, words = 3;
        std::vector<uint32_t> row(n), of;
        uint32_t u = 0;
        EXPECT(mirsha_dedup_rows(cy.ptr.data(), cy.len.data(), cy.first.data(), n, row.data(), &u) == MIRSHA_OK,
               "rows");
        for (uint32_t i = 0; i < n; i += 3) of.push_back(i);
        std::vector<uint64_t> has(words);
        std::vector<uint32_t> base(words);
        EXPECT(mirsha_expect_plan(of.data(), (uint32_t)of.size(), n, has.data(), base.data()) == MIRSHA_OK, "plan");
        bool ok = true;
        for (uint32_t k = 0; k < of.size(); k++) {
            const uint32_t i = of[k], w = i >> 6, b = i & 63u;
            ok &= ((has[w] >> b) & 1u) && base[w] + (uint32_t)__builtin_popcountll(has[w] & ((1ull << b) - 1ull)) == k;
            ok &= row[i] < u;
        }
        EXPECT(ok, "lane addressing");
    }
    if (fails) return 1;
    printf("expect dedup unit ok\n");
    return 0;
}
