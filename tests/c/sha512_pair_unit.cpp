// CPU unit test of mirbft_amd/csrc/sha512_pair.h (no HIP): the SHA-512
// compression split into a producer (schedule + K) and a consumer (rounds),
// driven through a two-slot ring in the order of the pair kernels of
// mirsha_sha512_pair.hip: the hand-over is a group of 16 rounds, the producer
// is one group ahead, the slots alternate, and a block of a lane that is no
// longer live is produced and consumed but not added.  The case file is that of
// tests/c/sha512_unit.cpp (tests/test_sha512_pair_unit.py writes it):
//   M <len> <digest hex>          message of <len> bytes, byte i = msg_byte(len, i)
//   S <message hex or -> <digest hex>   a literal message (the FIPS vectors)
//   L <n> <idx...> <digest hex>   a list of n entries (-1 = MIRSHA_NULL_INDEX)
//                                 over the table row r byte j = row_byte(r, j)
// Before the cases: produce_kw + consume_kw == sha512::compress on random
// states and words (and a block that is not live leaves the state alone).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sha512_pair.h"

namespace s5 = mirsha::sha512;

static uint8_t msg_byte(uint64_t len, uint64_t i) { return (uint8_t)(i * 131u + len * 7u + 13u); }
static uint8_t row_byte(uint32_t r, uint32_t j) { return (uint8_t)(r * 37u + j * 11u + 5u); }

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> b;
    if (h == "-") return b;
    for (size_t i = 0; i + 1 < h.size(); i += 2) b.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return b;
}

static void digest_bytes(const uint64_t st[8], uint8_t out[32]) {
    uint32_t d[8];
    s5::digest_words(st, d);
    memcpy(out, d, 32);
}

// ---- the kernels' loop on one lane -------------------------------------------

// A producer-side source: block(blk, w) fills the words of block blk (called
// for 0, 1, 2, ... in order) and returns whether the lane has that block.
struct Source {
    virtual ~Source() {}
    virtual bool block(uint32_t blk, uint64_t w[16]) = 0;
};

struct Ring {
    uint64_t kw[2][16];
    uint32_t live[2];  // [block & 1]
    uint32_t more[2];
    long barriers = 0;
};

template <int G>
static void put_group(uint64_t w[16], uint64_t slot[16]) {
    s5::produce_group<G>(w, slot);
}

static void open_block(Source& src, Ring& ring, uint32_t blk, uint32_t slot, uint32_t extra, uint64_t w[16]) {
    // `extra`: blocks that another lane of the wave still has, so this lane's
    // dead blocks run through the ring as well
    const bool has = src.block(blk, w);
    const bool any = has || blk < extra;
    ring.live[blk & 1u] = has ? 1u : 0u;
    ring.more[blk & 1u] = any ? 1u : 0u;
    if (any) put_group<0>(w, ring.kw[slot]);
}

template <int G>
static void pair_step(Source& src, Ring& ring, uint32_t blk, uint32_t extra, uint64_t w[16], uint64_t v[8]) {
    const uint32_t rd = (blk + (uint32_t)G) & 1u, wr = rd ^ 1u;
    // the consumer reads its slot before the producer's write could matter: the
    // two run concurrently on the device and must not touch the same slot
    uint64_t poison[16];
    for (auto& x : poison) x = 0xDEADBEEFDEADBEEFull;
    uint64_t mine[16];
    memcpy(mine, ring.kw[rd], sizeof mine);
    if constexpr (G + 1 < s5::kPairGroups)
        put_group<G + 1>(w, ring.kw[wr]);
    else
        open_block(src, ring, blk + 1u, wr, extra, w);
    if (memcmp(mine, ring.kw[rd], sizeof mine) != 0) {
        fprintf(stderr, "the producer wrote the slot being consumed\n");
        exit(1);
    }
    s5::consume_group(v, ring.kw[rd]);
    memcpy(ring.kw[rd], poison, sizeof poison);  // consumed: whoever reads it again reads garbage
    ring.barriers++;
}

static long run_pair(Source& src, uint32_t extra, uint64_t st[8]) {
    Ring ring;
    for (int i = 0; i < 8; i++) st[i] = s5::kH0[i];
    uint64_t w[16] = {}, v[8] = {};
    open_block(src, ring, 0u, 0u, extra, w);
    ring.barriers++;
    uint32_t blk = 0;
    for (; ring.more[blk & 1u]; blk++) {
        const bool live = ring.live[blk & 1u] != 0u;
        for (int i = 0; i < 8; i++) v[i] = st[i];
        pair_step<0>(src, ring, blk, extra, w, v);
        pair_step<1>(src, ring, blk, extra, w, v);
        pair_step<2>(src, ring, blk, extra, w, v);
        pair_step<3>(src, ring, blk, extra, w, v);
        pair_step<4>(src, ring, blk, extra, w, v);
        s5::finish_block(st, v, live);
    }
    if (ring.barriers != 1 + 5l * blk) {
        fprintf(stderr, "barriers %ld for %u blocks\n", ring.barriers, blk);
        exit(1);
    }
    return (long)blk;
}

// The request kernel's producer: the message lies in an arena, followed by
// bytes that are not its own; a block past the message's end (a finished lane)
// reads whatever lies there.
struct MsgSource : Source {
    std::vector<uint8_t> arena;
    uint32_t L, nb;
    MsgSource(const std::vector<uint8_t>& m, uint32_t extra) : L((uint32_t)m.size()), nb(s5::blocks_for_len(L)) {
        arena.assign(128ull * (nb > extra ? nb : extra) + 128u, 0xA5);
        if (L) memcpy(arena.data(), m.data(), L);
    }
    bool block(uint32_t blk, uint64_t w[16]) override {
        const uint32_t p = 128u * blk;
        uint32_t bw[32];
        for (int k = 0; k < 32; k++) {
            const uint8_t* b = arena.data() + p + 4 * k;
            bw[k] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        }
        if (blk < nb && (uint64_t)p + 128u > L) s5::pad_block(bw, p, L, blk + 1u == nb);
        s5::join_words(bw, w);
        return blk < nb;
    }
};

// The list kernel's producer: nulls skipped in the walk, four rows a block, the
// list ends in the first block that gets fewer than four.
struct ListSource : Source {
    std::vector<int64_t> idx;
    size_t e = 0;
    uint32_t d0 = 0;
    bool more = true;
    explicit ListSource(const std::vector<int64_t>& i) : idx(i) {}
    bool block(uint32_t, uint64_t w[16]) override {
        const bool has = more;
        uint32_t rows[4][8];
        for (auto& r : rows)
            for (auto& x : r) x = 0xDEADBEEFu;
        uint32_t filled = 0;
        while (more && filled < 4u && e < idx.size()) {
            if (idx[e] >= 0) {
                uint8_t row[32];
                for (uint32_t j = 0; j < 32; j++) row[j] = row_byte((uint32_t)idx[e], j);
                memcpy(rows[filled++], row, 32);
            }
            e++;
        }
        const bool last = filled < 4u;
        s5::list_block(rows, d0, d0 + filled, last, w);
        more = more && !last;
        d0 += 4u;
        return has;
    }
};

static int check(const char* what, const uint8_t got[32], const std::string& want_hex) {
    const std::vector<uint8_t> want = unhex(want_hex);
    if (want.size() == 32 && memcmp(got, want.data(), 32) == 0) return 0;
    fprintf(stderr, "%s: digest differs from %s\n", what, want_hex.c_str());
    return 1;
}

// A message alone in its wave, and beside a lane that has 2 more blocks.
static int hash_message(const char* what, const std::vector<uint8_t>& m, const std::string& want) {
    int bad = 0;
    const uint32_t nb = s5::blocks_for_len((uint32_t)m.size());
    for (uint32_t extra : {0u, nb + 2u}) {
        MsgSource src(m, extra);
        uint64_t st[8];
        const long trips = run_pair(src, extra, st);
        if (trips != (long)(extra > nb ? extra : nb)) {
            fprintf(stderr, "%s: %ld trips\n", what, trips);
            bad++;
        }
        uint8_t got[32];
        digest_bytes(st, got);
        bad += check(what, got, want);
    }
    return bad;
}

static int hash_list(const std::vector<int64_t>& idx, const std::string& want) {
    int bad = 0;
    for (uint32_t extra : {0u, 5u}) {
        ListSource src(idx);
        uint64_t st[8];
        run_pair(src, extra, st);
        uint8_t got[32];
        digest_bytes(st, got);
        bad += check("L", got, want);
    }
    return bad;
}

static uint64_t rnd(uint64_t& s) {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int split_equals_compress() {
    uint64_t seed = 0x6d69727368613531ull;
    for (int t = 0; t < 2000; t++) {
        uint64_t st[8], w[16];
        for (auto& x : st) x = rnd(seed);
        for (auto& x : w) x = rnd(seed);
        if (t == 0) memset(w, 0, sizeof w);
        if (t == 1) memset(w, 0xFF, sizeof w);
        uint64_t want[8], w1[16];
        memcpy(want, st, sizeof want);
        memcpy(w1, w, sizeof w1);
        s5::compress(want, w1);
        // whole blocks
        uint64_t got[8], dead[8], w2[16], kw[80];
        memcpy(got, st, sizeof got);
        memcpy(dead, st, sizeof dead);
        memcpy(w2, w, sizeof w2);
        s5::produce_kw(w2, kw);
        s5::consume_kw(got, kw, true);
        s5::consume_kw(dead, kw, false);
        if (memcmp(got, want, sizeof want) != 0 || memcmp(dead, st, sizeof dead) != 0 ||
            memcmp(w1, w2, sizeof w1) != 0) {  // (the window ends as compress leaves it)
            fprintf(stderr, "produce_kw + consume_kw differs from compress (trial %d)\n", t);
            return 1;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (split_equals_compress()) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char line[1 << 20];
    int bad = 0, cases = 0;
    while (fgets(line, sizeof line, f)) {
        std::vector<std::string> tok;
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        cases++;
        if (tok[0] == "M" && tok.size() == 3) {
            const uint64_t L = strtoull(tok[1].c_str(), nullptr, 10);
            std::vector<uint8_t> m(L);
            for (uint64_t i = 0; i < L; i++) m[i] = msg_byte(L, i);
            bad += hash_message(("M " + tok[1]).c_str(), m, tok[2]);
        } else if (tok[0] == "S" && tok.size() == 3) {
            bad += hash_message(("S " + tok[1]).c_str(), unhex(tok[1]), tok[2]);
        } else if (tok[0] == "L" && tok.size() >= 3) {
            const size_t n = strtoul(tok[1].c_str(), nullptr, 10);
            if (tok.size() != n + 3) return 2;
            std::vector<int64_t> idx(n);
            for (size_t i = 0; i < n; i++) idx[i] = strtoll(tok[2 + i].c_str(), nullptr, 10);
            bad += hash_list(idx, tok[n + 2]);
        } else {
            return 2;
        }
    }
    fclose(f);
    if (bad || !cases) return 1;
    printf("sha512 pair unit ok: %d cases\n", cases);
    return 0;
}
