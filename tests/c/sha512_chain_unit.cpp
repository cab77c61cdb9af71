// CPU unit test of the host-compilable step of a SHA-512/256 commit programme
// (mirbft_amd/csrc/sha512_chain.h, no HIP), driven the way the kernels of
// mirsha_sha512_chains.hip drive it: one lane state walks an entry list in
// steps, the step after the current one planned before the current one is
// hashed.  tests/test_sha512_chain_unit.py writes the cases to a file and
// passes its path; one case a line:
//   <U|C> <p> <n> <op...>    p digests (table rows 1000 .. 1000 + p) are written
//                            by an earlier walk; then the n ops are walked: a
//                            table row to write, or -1 = a checkpoint.
//                            U: one lane over the whole list.  C: the list cut
//                            behind every checkpoint, one lane a segment; only
//                            the first starts from the state, the others from
//                            Hasher(), and only the last one's state is kept.
// For every case one line goes to stdout: the checkpoint values in order, then
// Sum() of the state left behind, as hex words.  The table is
// row r byte j = row_byte(r, j).
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sha512_chain.h"

namespace s5 = mirsha::sha512;

static uint8_t row_byte(uint32_t r, uint32_t j) { return (uint8_t)(r * 37u + j * 11u + 5u); }

struct Lane {
    uint64_t st[8], pw[s5::kChainPendWords], n;
};

static void fresh(Lane& l) {  // Hasher(); the pending words of a fresh state hold anything
    for (int i = 0; i < 8; i++) l.st[i] = s5::kH0[i];
    for (auto& w : l.pw) w = 0xA5A5A5A5A5A5A5A5ull;
    l.n = 0;
}

struct Fetch {
    s5::ChainStep s;
    uint32_t rows[4][8];
};

// chain_fetch: every entry read is guarded by the lane's own [e, end).
static void fetch(const uint32_t* ent, uint32_t end, uint32_t& e, uint64_t& n, uint32_t x[4], Fetch& f) {
    f.s = s5::chain_plan(x, end - e, n);
    for (int sl = 0; sl < 4; sl++) {
        for (auto& v : f.rows[sl]) v = 0xDEADBEEFu;  // a slot that is not taken holds anything
        if (!((f.s.take >> sl) & 1u)) continue;
        uint8_t row[32];
        for (uint32_t j = 0; j < 32; j++) row[j] = row_byte(f.s.id[sl], j);
        memcpy(f.rows[sl], row, 32);
    }
    e += f.s.consumed;
    n = f.s.n_after;
    for (uint32_t i = 0; i < 4; i++) x[i] = e + i < end ? ent[e + i] : 0x7FFFFFFFu;
}

static void put_digest(const uint64_t st[8], std::string& line) {
    uint32_t d[8];
    s5::digest_words(st, d);
    uint8_t b[32];
    memcpy(b, d, 32);  // the kernels store these dwords little-endian
    char hex[65];
    for (int i = 0; i < 32; i++) snprintf(hex + 2 * i, 3, "%02x", b[i]);
    line += hex;
    line += ' ';
}

// chain_walk over ent[e, end): the entries are a heap copy of exactly that
// range's extent, so a read past it is the sanitizer's to find.
static void walk(Lane& l, const uint32_t* ent, uint32_t e, uint32_t end, std::string& line) {
    uint32_t x[4];
    for (uint32_t i = 0; i < 4; i++) x[i] = e + i < end ? ent[e + i] : 0x7FFFFFFFu;
    Fetch cur;
    fetch(ent, end, e, l.n, x, cur);
    while (cur.s.full || cur.s.cp || cur.s.keep) {
        Fetch nxt;
        fetch(ent, end, e, l.n, x, nxt);
        uint64_t w[16];
        s5::chain_block(l.pw, cur.rows, cur.s, w);
        if (cur.s.keep) s5::chain_keep(w, l.pw);
        if (cur.s.full || cur.s.cp) s5::compress(l.st, w);
        if (cur.s.cp) {
            put_digest(l.st, line);
            for (int i = 0; i < 8; i++) l.st[i] = s5::kH0[i];
        }
        cur = nxt;
    }
    if (e != end) {
        fprintf(stderr, "the walk stopped at entry %u of %u\n", e, end);
        exit(1);
    }
}

static void sum(const Lane& l, std::string& line) {  // sha512_chains_sum_kernel: from a copy
    uint64_t st[8], w[16];
    for (int i = 0; i < 8; i++) st[i] = l.st[i];
    uint32_t rows[4][8];
    for (auto& r : rows)
        for (auto& v : r) v = 0xDEADBEEFu;
    s5::chain_block(l.pw, rows, s5::chain_sum_step(l.n), w);
    s5::compress(st, w);
    put_digest(st, line);
}

static void walk_all(Lane& l, const std::vector<uint32_t>& ent, bool cut, std::string& line) {
    const uint32_t total = (uint32_t)ent.size();
    std::unique_ptr<uint32_t[]> heap(new uint32_t[total ? total : 1u]);
    if (total) memcpy(heap.get(), ent.data(), 4ull * total);
    if (!cut) {
        walk(l, heap.get(), 0, total, line);
        return;
    }
    uint32_t start = 0;
    bool first = true;
    for (uint32_t e = 0; e < total; e++) {
        if (e + 1 < total && !(ent[e] & s5::kChainCheckpoint)) continue;
        Lane seg;
        if (first) seg = l; else fresh(seg);
        walk(seg, heap.get(), start, e + 1, line);
        if (e + 1 == total) l = seg;  // LAST
        first = false;
        start = e + 1;
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char buf[1 << 16];
    while (fgets(buf, sizeof buf, f)) {
        std::vector<std::string> tok;
        for (char* t = strtok(buf, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        if (tok.size() < 3 || (tok[0] != "U" && tok[0] != "C")) return 2;
        const uint32_t p = (uint32_t)strtoul(tok[1].c_str(), nullptr, 10);
        const size_t n = strtoul(tok[2].c_str(), nullptr, 10);
        if (tok.size() != n + 3) return 2;
        Lane l;
        fresh(l);
        std::string line;
        std::vector<uint32_t> pre;
        for (uint32_t i = 0; i < p; i++) pre.push_back(1000u + i);
        walk_all(l, pre, false, line);  // a programme without a checkpoint, as mirsha_chains_absorb runs
        std::vector<uint32_t> ent;
        uint32_t rows = 0;
        for (size_t i = 0; i < n; i++) {
            const long v = strtol(tok[3 + i].c_str(), nullptr, 10);
            ent.push_back(v < 0 ? (s5::kChainCheckpoint | rows++) : (uint32_t)v);
        }
        walk_all(l, ent, tok[0] == "C", line);
        sum(l, line);
        sum(l, line);  // a sum leaves the state as it was
        puts(line.c_str());
    }
    fclose(f);
    return 0;
}
