// CPU unit test of the host-compilable step of a stream programme under
// SHA-512/256 (mirbft_amd/csrc/sha512_stream.h, no HIP), driven the way the
// kernels of mirsha_sha512_streams.hip drive it: one lane walks an entry list
// in steps of at most one compression, and the window of the step after the
// current one is loaded before the current one is hashed.
// tests/test_sha512_stream_unit.py writes the cases to a file and passes its
// path; one case a line:
//   <U|C> <shift> <arena_len> <n> {<kind> <off> <len>} x n
// The arena's byte j is arena_byte(j); it lies `shift` (0-3) bytes into a heap
// block of exactly span = (shift + arena_len + 3) & ~3 bytes, whose other bytes
// hold 0xEE, and the loader gives zero for every word outside [0, span), as the
// buffer descriptor does: a read outside the block is the sanitizer's to find.
// kind: 0 WRITE, 1 SUM, 2 SUM_RESET, 3 RESET on one stream that starts as
// Hasher().  U: one lane over the whole list.  C: the list cut behind every
// SUM_RESET / RESET, one lane a segment; only the first starts from the state,
// the others from Hasher().  Every step runs the compression, needed or not, as
// a wave does for its idle lanes.  For every case one line goes to stdout: the
// sums' values in order, as hex.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sha512_stream.h"

namespace s5 = mirsha::sha512;

static uint8_t arena_byte(uint64_t j) { return (uint8_t)(j * 131u + 7u + (j >> 8) * 17u); }

struct Entry {
    uint32_t kind, len, off_lo, off_hi;  // the 16-byte record of the device
};

struct Arena {
    std::unique_ptr<uint8_t[]> block;
    uint32_t shift, span;
};

static uint32_t load_word(const Arena& a, uint32_t o, bool live) {
    if (!live || o >= a.span) return 0u;  // the dead offset / outside the descriptor's range
    uint32_t v;
    memcpy(&v, a.block.get() + o, 4);
    return v;
}

static void load_window(const Arena& a, bool wr, uint32_t at, uint32_t d[s5::kStreamWindowWords]) {
    const uint32_t a0 = at & ~3u;
    for (int i = 0; i < s5::kStreamWindowWords; i++) d[i] = load_word(a, a0 + 4u * (uint32_t)i, wr);
}

struct Lane {
    uint64_t st[8], hs[8];
    uint32_t bw[32];
    s5::StreamWalk wk;
};

static void fresh(Lane& l) {  // Hasher(); the block of a fresh state holds anything
    for (int i = 0; i < 8; i++) l.st[i] = s5::kH0[i], l.hs[i] = 0x5A5A5A5A5A5A5A5Aull;
    for (auto& w : l.bw) w = 0xA5A5A5A5u;
    l.wk.n = 0, l.wk.pos = 0, l.wk.sum2 = 0;
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

// Sha512StreamLane's walk over ent[e0, e1): the entries are a heap copy of
// exactly the list's extent.
static void walk(Lane& l, const Arena& a, const Entry* ent, uint32_t e0, uint32_t e1, std::string& line) {
    const Entry* ep = ent + e0;
    uint32_t left = e1 - e0;
    uint32_t d[s5::kStreamWindowWords];
    Entry x = ep[0], xn;
    auto request = [&] {
        load_window(a, left != 0u && (x.kind & 3u) == s5::kStreamWrite, l.wk.window(x.off_lo + a.shift), d);
        xn = ep[left > 1u ? 1u : 0u];
    };
    request();
    uint64_t guard = 0;
    while (left != 0u) {
        const s5::StreamStep s = l.wk.plan(x.kind, x.len, left != 0u);
        s5::stream_merge(l.bw, d, l.wk.window(x.off_lo + a.shift) & 3u, s);
        uint64_t w[16], ts[8];
        s5::stream_block(l.bw, l.st, l.hs, l.wk.n, s, w, ts);
        l.wk.advance(s);
        ep += (s.adv && left > 1u) ? 1 : 0;
        left -= s.adv ? 1u : 0u;
        if (s.adv) x = xn;
        request();
        const uint32_t after = s5::stream_after(s);
        s5::compress(ts, w);  // on every step: a step without one must not let it show
        if (after & s5::kStreamFin) put_digest(ts, line);
        s5::stream_finish(l.st, l.hs, ts, after);
        if (++guard > (1u << 24)) {
            fprintf(stderr, "the walk does not end\n");
            exit(1);
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char buf[1 << 20];
    while (fgets(buf, sizeof buf, f)) {
        std::vector<std::string> tok;
        for (char* t = strtok(buf, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        if (tok.size() < 4 || (tok[0] != "U" && tok[0] != "C")) return 2;
        Arena a;
        a.shift = (uint32_t)strtoul(tok[1].c_str(), nullptr, 10);
        const uint64_t arena_len = strtoull(tok[2].c_str(), nullptr, 10);
        const size_t n = strtoul(tok[3].c_str(), nullptr, 10);
        if (a.shift > 3u || tok.size() != 3 * n + 4 || n == 0) return 2;
        a.span = arena_len ? (uint32_t)((a.shift + arena_len + 3u) & ~3ull) : 0u;
        a.block.reset(new uint8_t[a.span ? a.span : 1u]);
        memset(a.block.get(), 0xEE, a.span);
        for (uint64_t j = 0; j < arena_len; j++) a.block[a.shift + j] = arena_byte(j);
        std::unique_ptr<Entry[]> ent(new Entry[n]);
        for (size_t i = 0; i < n; i++) {
            const uint32_t kind = (uint32_t)strtoul(tok[4 + 3 * i].c_str(), nullptr, 10);
            const uint64_t off = strtoull(tok[5 + 3 * i].c_str(), nullptr, 10);
            const uint32_t len = (uint32_t)strtoul(tok[6 + 3 * i].c_str(), nullptr, 10);
            if (kind > 3u || (kind == 0u && (len == 0u || off + len > arena_len))) return 2;
            ent[i] = {kind | (uint32_t)i << 2, kind ? 0u : len, kind ? 0u : (uint32_t)off, 0u};
        }
        Lane l;
        fresh(l);
        std::string line;
        if (tok[0] == "U") {
            walk(l, a, ent.get(), 0, (uint32_t)n, line);
        } else {
            uint32_t start = 0;
            for (uint32_t e = 0; e < n; e++) {
                const uint32_t k = ent[e].kind & 3u;
                if (e + 1 < n && k != s5::kStreamSumReset && k != s5::kStreamReset) continue;
                Lane seg;
                if (start == 0) seg = l; else fresh(seg);
                walk(seg, a, ent.get(), start, e + 1, line);
                if (e + 1 == n) l = seg;  // LAST
                start = e + 1;
            }
        }
        puts(line.c_str());
    }
    fclose(f);
    return 0;
}
