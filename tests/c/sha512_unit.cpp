// CPU unit test of the host-compilable core of mirbft_amd/csrc/sha512_device.h
// (no HIP): the SHA-512/256 compression, the padding of a message's blocks and
// the blocks of a digest list, driven the way the two kernels of
// mirsha_sha512.hip drive them.  tests/test_sha512_unit.py writes the cases
// (expected digests from hashlib) to a file and passes its path:
//   M <len> <digest hex>          message of <len> bytes, byte i = msg_byte(len, i)
//   S <message hex or -> <digest hex>   a literal message (the FIPS vectors)
//   L <n> <idx...> <digest hex>   a list of n entries (-1 = MIRSHA_NULL_INDEX)
//                                 over the table row r byte j = row_byte(r, j)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sha512_device.h"

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
    memcpy(out, d, 32);  // the kernels store these dwords little-endian
}

// The request kernel's loop: the message lies in an arena, followed by bytes
// that are not its own; every block's 32 big-endian words are read from there
// and only pad_block decides what of them counts.
static void hash_message(const std::vector<uint8_t>& m, uint8_t out[32]) {
    const uint32_t L = (uint32_t)m.size();
    const uint32_t nb = s5::blocks_for_len(L);
    if (nb != (uint32_t)(((uint64_t)L + 16u) / 128u + 1u)) {
        fprintf(stderr, "blocks_for_len(%u) = %u\n", L, nb);
        exit(1);
    }
    std::vector<uint8_t> arena(128ull * nb, 0xA5);  // a neighbour's bytes behind the message
    if (L) memcpy(arena.data(), m.data(), L);
    uint64_t st[8];
    for (int i = 0; i < 8; i++) st[i] = s5::kH0[i];
    for (uint32_t blk = 0; blk < nb; blk++) {
        const uint32_t p = 128u * blk;
        uint32_t bw[32];
        for (int k = 0; k < 32; k++) {
            const uint8_t* b = arena.data() + p + 4 * k;
            bw[k] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        }
        if ((uint64_t)p + 128u > L) s5::pad_block(bw, p, L, blk + 1u == nb);
        uint64_t w[16];
        s5::join_words(bw, w);
        s5::compress(st, w);
    }
    digest_bytes(st, out);
}

// The list kernel's walk: null entries are skipped, four rows fill a block,
// the list ends in the first block that gets fewer than four.
static void hash_list(const std::vector<int64_t>& idx, uint8_t out[32]) {
    uint64_t st[8];
    for (int i = 0; i < 8; i++) st[i] = s5::kH0[i];
    size_t e = 0;
    for (uint32_t d0 = 0;; d0 += 4u) {
        uint32_t rows[4][8];
        for (auto& r : rows)
            for (auto& x : r) x = 0xDEADBEEFu;  // a slot past the list's end holds anything
        uint32_t filled = 0;
        while (filled < 4u && e < idx.size()) {
            if (idx[e] >= 0) {
                uint8_t row[32];
                for (uint32_t j = 0; j < 32; j++) row[j] = row_byte((uint32_t)idx[e], j);
                memcpy(rows[filled++], row, 32);
            }
            e++;
        }
        const bool last = filled < 4u;
        uint64_t w[16];
        s5::list_block(rows, d0, d0 + filled, last, w);
        s5::compress(st, w);
        if (last) break;
    }
    digest_bytes(st, out);
}

static int check(const char* what, const uint8_t got[32], const std::string& want_hex) {
    const std::vector<uint8_t> want = unhex(want_hex);
    if (want.size() == 32 && memcmp(got, want.data(), 32) == 0) return 0;
    fprintf(stderr, "%s: digest differs from %s\n", what, want_hex.c_str());
    return 1;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char line[1 << 20];
    int bad = 0, cases = 0;
    while (fgets(line, sizeof line, f)) {
        std::vector<std::string> tok;
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        uint8_t got[32];
        cases++;
        if (tok[0] == "M" && tok.size() == 3) {
            const uint64_t L = strtoull(tok[1].c_str(), nullptr, 10);
            std::vector<uint8_t> m(L);
            for (uint64_t i = 0; i < L; i++) m[i] = msg_byte(L, i);
            hash_message(m, got);
            bad += check(("M " + tok[1]).c_str(), got, tok[2]);
        } else if (tok[0] == "S" && tok.size() == 3) {
            hash_message(unhex(tok[1]), got);
            bad += check(("S " + tok[1]).c_str(), got, tok[2]);
        } else if (tok[0] == "L" && tok.size() >= 3) {
            const size_t n = strtoul(tok[1].c_str(), nullptr, 10);
            if (tok.size() != n + 3) return 2;
            std::vector<int64_t> idx(n);
            for (size_t i = 0; i < n; i++) idx[i] = strtoll(tok[2 + i].c_str(), nullptr, 10);
            hash_list(idx, got);
            bad += check("L", got, tok[n + 2]);
        } else {
            return 2;
        }
    }
    fclose(f);
    if (bad || !cases) return 1;
    printf("sha512 unit ok: %d cases\n", cases);
    return 0;
}
