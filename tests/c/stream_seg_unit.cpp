// stream_seg_unit.cpp -- CPU unit test of mirsha_stream_seg_plan
// (mirbft_amd/csrc/mirsha_host.cpp, compiled here with g++: no HIP, no GPU):
// the segments a stream submission of the ring sends to the device, against a
// restatement built from the ops directly, with guard entries behind every
// output, the entry arrays against mirsha_stream_plan's own, the segment
// count's formula, the rejected programmes, and a differential check of both
// stream plans on small random programmes; and mirsha::host::seg_straddle
// against its definition.  Prints "stream seg unit ok"; exit 1 with a message
// at the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
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

static const uint32_t kGuard = 0xA5A5A5A5u;
static const uint64_t kGuard64 = 0xA5A5A5A5A5A5A5A5ull;
static const uint32_t W = MIRSHA_STREAM_WRITE, S = MIRSHA_STREAM_SUM, SR = MIRSHA_STREAM_SUM_RESET,
                      R = MIRSHA_STREAM_RESET;

struct Op {
    uint32_t stream, kind;
    uint64_t off;
    uint32_t len;
};

struct Plan {
    std::vector<uint32_t> seg_stream, sfirst, flags;
    uint32_t active = 0, entries = 0;
};

static bool cuts(uint32_t kind) { return kind == SR || kind == R; }

// Per stream its ops in op order, zero-length writes dropped; each stream's
// list cut after every SUM_RESET / RESET.
static Plan restate(const std::vector<Op>& ops) {
    std::map<uint32_t, std::vector<uint32_t>> per;
    for (const Op& o : ops)
        if (o.kind != W || o.len) per[o.stream].push_back(o.kind);
    Plan p;
    p.active = (uint32_t)per.size();
    p.sfirst.push_back(0);
    for (const auto& kv : per) {
        bool first = true;
        for (size_t k = 0; k < kv.second.size(); k++) {
            p.entries++;
            const bool last = k + 1 == kv.second.size();
            if (cuts(kv.second[k]) || last) {
                p.seg_stream.push_back(kv.first);
                p.flags.push_back((first ? MIRSHA_STREAM_SEG_FIRST : 0u) | (last ? MIRSHA_STREAM_SEG_LAST : 0u));
                p.sfirst.push_back(p.entries);
                first = false;
            }
        }
    }
    return p;
}

struct Arrays {
    std::vector<uint32_t> s, k, l;
    std::vector<uint64_t> o;
    explicit Arrays(const std::vector<Op>& ops) {
        for (const Op& op : ops) {
            s.push_back(op.stream); k.push_back(op.kind); o.push_back(op.off); l.push_back(op.len);
        }
    }
};

static void check(const std::vector<Op>& ops, uint32_t n_streams, uint64_t arena_len, const char* what) {
    const uint32_t n = (uint32_t)ops.size();
    const Arrays a(ops);
    for (int pack = 0; pack < 2; pack++) {
        std::vector<uint32_t> seg_stream(n + 1, kGuard), sfirst(n + 2, kGuard), flags(n + 1, kGuard);
        std::vector<uint32_t> kind(n + 1, kGuard), len(n + 1, kGuard);
        std::vector<uint64_t> off(n + 1, kGuard64);
        uint32_t ns = kGuard, na = kGuard, ne = kGuard, nv = kGuard, bad = kGuard;
        uint64_t nb = kGuard64;
        const int rc = mirsha_stream_seg_plan(n ? a.s.data() : nullptr, n ? a.k.data() : nullptr,
                                              n ? a.o.data() : nullptr, n ? a.l.data() : nullptr, n, n_streams,
                                              arena_len, pack, seg_stream.data(), sfirst.data(), flags.data(),
                                              kind.data(), off.data(), len.data(), &ns, &na, &ne, &nv, &nb, &bad);
        EXPECT(rc == MIRSHA_OK && bad == UINT32_MAX, "%s: rc %d bad %u", what, rc, bad);
        if (rc != MIRSHA_OK) return;
        const Plan w = restate(ops);
        EXPECT(ns == w.seg_stream.size() && na == w.active && ne == w.entries, "%s: counts %u %u %u", what, ns, na, ne);
        if (ns != w.seg_stream.size() || ne != w.entries) return;
        EXPECT(seg_stream[ns] == kGuard && flags[ns] == kGuard && sfirst[ns + 1] == kGuard && kind[ne] == kGuard &&
                   len[ne] == kGuard && off[ne] == kGuard64,
               "%s: wrote past its outputs", what);
        bool ok = sfirst[ns] == ne;
        for (uint32_t s = 0; s < ns; s++)
            ok &= seg_stream[s] == w.seg_stream[s] && flags[s] == w.flags[s] && sfirst[s] == w.sfirst[s];
        EXPECT(ok, "%s: segments differ", what);
        // the entry arrays and the counts are mirsha_stream_plan's, unchanged
        std::vector<uint32_t> act(n + 1), efirst(n + 2), kind2(n + 1), len2(n + 1);
        std::vector<uint64_t> off2(n + 1);
        uint32_t na2 = 0, ne2 = 0, nv2 = 0;
        uint64_t nb2 = 0;
        EXPECT(mirsha_stream_plan(n ? a.s.data() : nullptr, n ? a.k.data() : nullptr, n ? a.o.data() : nullptr,
                                  n ? a.l.data() : nullptr, n, n_streams, arena_len, pack, act.data(), efirst.data(),
                                  kind2.data(), off2.data(), len2.data(), &na2, &ne2, &nv2, &nb2, nullptr) == MIRSHA_OK,
               "%s: the stream plan itself", what);
        ok = na == na2 && ne == ne2 && nv == nv2 && nb == nb2;
        for (uint32_t e = 0; e < ne && ok; e++) ok &= kind[e] == kind2[e] && off[e] == off2[e] && len[e] == len2[e];
        EXPECT(ok, "%s: entries differ from mirsha_stream_plan's", what);
        // n_seg = active streams + reset-kind entries that are not their stream's final entry
        uint32_t inner = 0, counted = 0;
        for (uint32_t s = 0; s < ns; s++) {
            if (!(flags[s] & MIRSHA_STREAM_SEG_LAST)) inner++;
            const bool ends_cut = cuts(kind[sfirst[s + 1] - 1] & 3u);
            if (ends_cut && !(flags[s] & MIRSHA_STREAM_SEG_LAST)) counted++;
            EXPECT(sfirst[s + 1] > sfirst[s], "%s: segment %u is empty", what, s);
            EXPECT(ends_cut || (flags[s] & MIRSHA_STREAM_SEG_LAST), "%s: segment %u ends nowhere", what, s);
            for (uint32_t e = sfirst[s]; e + 1 < sfirst[s + 1]; e++)
                EXPECT(!cuts(kind[e] & 3u), "%s: a reset inside segment %u", what, s);
        }
        EXPECT(ns == na + inner && inner == counted, "%s: n_seg %u != %u + %u", what, ns, na, inner);
    }
}

static void reject(const std::vector<Op>& ops, uint32_t n_streams, uint64_t arena_len, int want_rc, uint32_t want_bad,
                   const char* what) {
    const uint32_t n = (uint32_t)ops.size();
    const Arrays a(ops);
    std::vector<uint32_t> seg_stream(n + 1, kGuard), sfirst(n + 2, kGuard), flags(n + 1, kGuard);
    std::vector<uint32_t> kind(n + 1, kGuard), len(n + 1, kGuard);
    std::vector<uint64_t> off(n + 1, kGuard64);
    uint32_t ns = kGuard, na = kGuard, ne = kGuard, nv = kGuard, bad = kGuard;
    uint64_t nb = kGuard64;
    const int rc = mirsha_stream_seg_plan(a.s.data(), a.k.data(), a.o.data(), a.l.data(), n, n_streams, arena_len, 0,
                                          seg_stream.data(), sfirst.data(), flags.data(), kind.data(), off.data(),
                                          len.data(), &ns, &na, &ne, &nv, &nb, &bad);
    EXPECT(rc == want_rc && bad == want_bad, "%s: rc %d bad %u", what, rc, bad);
    EXPECT(ns == 0, "%s: n_seg %u after a failure", what, ns);
    EXPECT(seg_stream[n] == kGuard && flags[n] == kGuard && sfirst[n + 1] == kGuard && kind[n] == kGuard,
           "%s: wrote past its outputs", what);
    // the code and the bad op are mirsha_stream_plan's own
    std::vector<uint32_t> act(n + 1), efirst(n + 2);
    uint32_t bad2 = kGuard;
    const int rc2 = mirsha_stream_plan(a.s.data(), a.k.data(), a.o.data(), a.l.data(), n, n_streams, arena_len, 0,
                                       act.data(), efirst.data(), kind.data(), off.data(), len.data(), &na, &ne, &nv,
                                       &nb, &bad2);
    EXPECT(rc2 == rc && bad2 == bad, "%s: mirsha_stream_plan says rc %d bad %u", what, rc2, bad2);
}

// ---- Differential check of mirsha_stream_plan and mirsha_stream_seg_plan: every
// array (guards included: nothing is written before every op has passed),
// every count, the code and the bad op, against a plain restatement -- the
// argument checks in their order, a per-stream std::vector append in op
// order, then a cut; with `pack`, every distinct range once in entry order.
struct Out {
    int rc = 0;
    uint32_t ns = kGuard, na = kGuard, ne = kGuard, nv = kGuard, bad = kGuard;
    uint64_t nb = kGuard64;
    std::vector<uint32_t> act, efirst, seg_stream, sfirst, flags, kind, len;
    std::vector<uint64_t> off;
    explicit Out(uint32_t cap)
        : act(cap + 2, kGuard), efirst(cap + 2, kGuard), seg_stream(cap + 2, kGuard), sfirst(cap + 2, kGuard),
          flags(cap + 2, kGuard), kind(cap + 2, kGuard), len(cap + 2, kGuard), off(cap + 2, kGuard64) {}
    bool operator==(const Out& o) const {
        return rc == o.rc && ns == o.ns && na == o.na && ne == o.ne && nv == o.nv && bad == o.bad && nb == o.nb &&
               act == o.act && efirst == o.efirst && seg_stream == o.seg_stream && sfirst == o.sfirst &&
               flags == o.flags && kind == o.kind && len == o.len && off == o.off;
    }
};

struct OpArrays {  // any of them may be NULL
    const uint32_t *s, *k;
    const uint64_t* o;
    const uint32_t* l;
};

static Out model(bool seg, const OpArrays& a, uint32_t n, uint32_t n_streams, uint64_t arena_len, int pack,
                 bool outputs, uint32_t cap) {
    Out w(cap);
    w.bad = UINT32_MAX;
    w.na = w.ne = w.nv = 0;
    w.nb = 0;
    if (seg) w.ns = 0;
    std::vector<uint32_t>& first = seg ? w.sfirst : w.efirst;
    w.rc = MIRSHA_EINVAL;
    if (n > MIRSHA_STREAM_MAX_OPS) {
        w.rc = MIRSHA_ERANGE;
        return w;
    }
    if (n == 0) {
        w.rc = MIRSHA_OK;
        if (outputs) first[0] = 0;
        return w;
    }
    if (!a.s || !a.k) return w;
    bool writes = false;
    for (uint32_t i = 0; i < n; i++) writes |= a.k[i] == W;
    if (writes && (!a.o || !a.l)) return w;
    for (uint32_t i = 0; i < n; i++) {
        bool ok = a.s[i] < n_streams && a.k[i] <= R;
        if (ok && a.k[i] == W) ok = a.o[i] <= arena_len && a.l[i] <= arena_len - a.o[i];
        if (!ok) {
            w.bad = i;
            return w;
        }
    }
    if (!outputs) return w;
    struct Ent {
        uint32_t kind, len;
        uint64_t off;
    };
    std::vector<std::vector<Ent>> per(n_streams);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t k = a.k[i];
        if (k == W && a.l[i] == 0) continue;
        const bool sum = k == S || k == SR;
        per[a.s[i]].push_back({k | (sum ? w.nv++ << 2 : 0u), k == W ? a.l[i] : 0u, k == W ? a.o[i] : 0u});
    }
    w.rc = MIRSHA_OK;
    first[0] = 0;
    std::map<std::pair<uint64_t, uint32_t>, uint64_t> packed;  // range -> where its bytes lie
    for (uint32_t s = 0; s < n_streams; s++) {
        const uint32_t e0 = w.ne;
        for (size_t k = 0; k < per[s].size(); k++) {
            const Ent& e = per[s][k];
            w.kind[w.ne] = e.kind;
            w.len[w.ne] = e.len;
            w.off[w.ne] = e.off;
            if (!pack) {
                w.nb += e.len;
            } else if (e.len) {
                const auto it = packed.emplace(std::make_pair(e.off, e.len), w.nb);
                w.off[w.ne] = it.first->second;
                if (it.second) w.nb += e.len;
            }
            w.ne++;
            const bool last = k + 1 == per[s].size();
            if (!seg || !(cuts(e.kind & 3u) || last)) continue;
            w.seg_stream[w.ns] = s;
            // FIRST: no cut of this stream yet, so the segment begins at the stream's first entry
            w.flags[w.ns] = (w.sfirst[w.ns] == e0 ? MIRSHA_STREAM_SEG_FIRST : 0u) | (last ? MIRSHA_STREAM_SEG_LAST : 0u);
            w.sfirst[++w.ns] = w.ne;
        }
        if (per[s].empty()) continue;
        if (!seg) {
            w.act[w.na] = s;
            w.efirst[w.na + 1] = w.ne;
        }
        w.na++;
    }
    return w;
}

static void differ(const OpArrays& a, uint32_t n, uint32_t n_streams, uint64_t arena_len, bool outputs, uint32_t cap,
                   const char* what) {
    for (int seg = 0; seg < 2; seg++)
        for (int pack = 0; pack < 2; pack++) {
            Out g(cap);
            auto p = [&](std::vector<uint32_t>& v) { return outputs ? v.data() : nullptr; };
            uint64_t* po = outputs ? g.off.data() : nullptr;
            g.rc = seg ? mirsha_stream_seg_plan(a.s, a.k, a.o, a.l, n, n_streams, arena_len, pack, p(g.seg_stream),
                                                p(g.sfirst), p(g.flags), p(g.kind), po, p(g.len), &g.ns, &g.na, &g.ne,
                                                &g.nv, &g.nb, &g.bad)
                       : mirsha_stream_plan(a.s, a.k, a.o, a.l, n, n_streams, arena_len, pack, p(g.act), p(g.efirst),
                                            p(g.kind), po, p(g.len), &g.na, &g.ne, &g.nv, &g.nb, &g.bad);
            const Out w = model(seg != 0, a, n, n_streams, arena_len, pack, outputs, cap);
            EXPECT(g == w, "%s (%s plan, pack %d, %u ops): rc %d/%d bad %u/%u counts %u %u %u %u %llu / %u %u %u %u %llu",
                   what, seg ? "seg" : "stream", pack, n, g.rc, w.rc, g.bad, w.bad, g.ns, g.na, g.ne, g.nv,
                   (unsigned long long)g.nb, w.ns, w.na, w.ne, w.nv, (unsigned long long)w.nb);
        }
}

static void differential() {
    std::mt19937_64 rng(22);
    for (int round = 0; round < 4000; round++) {
        const uint32_t n_streams = 1 + (uint32_t)(rng() % 5);
        const uint64_t arena_len = rng() % 201;
        const uint32_t n = (uint32_t)(rng() % 41);
        std::vector<Op> ops(n);
        for (uint32_t i = 0; i < n; i++) {
            Op& o = ops[i];
            o.stream = (uint32_t)(rng() % n_streams);
            o.kind = (uint32_t)(rng() % 6);
            if (o.kind == W || o.kind > R) {
                o.kind = W;
                if (i && ops[i - 1].kind == W && rng() % 3 == 0) {  // the same range again
                    o.off = ops[i - 1].off, o.len = ops[i - 1].len;
                } else {
                    o.off = rng() % (arena_len + 1);
                    o.len = rng() % 5 == 0 ? 0u : (uint32_t)(rng() % (arena_len - o.off + 1));
                }
            } else {
                o.off = rng();  // ignored
                o.len = (uint32_t)rng();
            }
        }
        const uint32_t cls = (uint32_t)(rng() % 13), at = n ? (uint32_t)(rng() % n) : 0u;
        bool outputs = true;
        const char* what = "differential: a valid programme";
        if (n && cls == 6) ops[at].stream = n_streams + (uint32_t)(rng() % 3), what = "differential: a bad stream";
        if (n && cls == 7) ops[at].kind = R + 1u + (uint32_t)(rng() % 3), what = "differential: a bad kind";
        if (n && cls == 8) {
            what = "differential: a write out of range";
            ops[at].kind = W;
            ops[at].off = rng() % (arena_len + 3);
            ops[at].len = (uint32_t)(arena_len - std::min(arena_len, ops[at].off)) + 1u;
        }
        if (cls == 10) outputs = false, what = "differential: NULL outputs";
        if (cls == 11) {  // with a bad op: the inner plan's code and bad op come first
            outputs = false, what = "differential: NULL outputs and a bad op";
            if (n) ops[at].stream = n_streams;
        }
        const Arrays a(ops);
        OpArrays p = {a.s.data(), a.k.data(), a.o.data(), a.l.data()};
        if (cls == 9) {
            what = "differential: a NULL op array";
            const uint32_t which = (uint32_t)(rng() % 4);
            if (which == 0) p.s = nullptr;
            if (which == 1) p.k = nullptr;
            if (which == 2) p.o = nullptr;  // refused only when an op writes
            if (which == 3) p.l = nullptr;
        }
        differ(p, n, n_streams, arena_len, outputs, n, what);
    }
    const uint32_t one[1] = {0};
    const uint64_t one64[1] = {0};
    const OpArrays p = {one, one, one64, one};
    differ(p, MIRSHA_STREAM_MAX_OPS + 1u, 4, 3, true, 0, "differential: too many ops");  // refused before an array is read
    differ(p, MIRSHA_STREAM_MAX_OPS + 1u, 4, 3, false, 0, "differential: too many ops, NULL outputs");
}

// ---- mirsha::host::seg_straddle over the flags of owners with the given segment
// counts, against the definition: a LAST lane whose wave index differs from
// its owner's FIRST lane's.
static void straddle(const std::vector<uint32_t>& seg_counts, bool want, const char* what) {
    std::vector<uint32_t> flags;
    for (uint32_t k : seg_counts)
        for (uint32_t j = 0; j < k; j++)
            flags.push_back((j == 0 ? MIRSHA_STREAM_SEG_FIRST : 0u) | (j + 1 == k ? MIRSHA_STREAM_SEG_LAST : 0u));
    bool def = false;
    for (size_t s = 0, first = 0; s < flags.size(); s++) {
        if (flags[s] & MIRSHA_STREAM_SEG_FIRST) first = s;
        if ((flags[s] & MIRSHA_STREAM_SEG_LAST) && s / 64 != first / 64) def = true;
    }
    EXPECT(def == want, "%s: the definition says %d", what, (int)def);
    EXPECT(mirsha::host::seg_straddle(flags.data(), (uint32_t)flags.size(), 64) == want, "%s: not %d", what, (int)want);
}

static void straddles() {
    EXPECT(!mirsha::host::seg_straddle(nullptr, 0, 64), "no segments");
    straddle({1}, false, "one segment");
    straddle({64}, false, "one stream over exactly one wave");
    straddle({65}, true, "one stream over 65 lanes");
    straddle(std::vector<uint32_t>(64, 1), false, "64 streams of one segment");
    straddle(std::vector<uint32_t>(65, 1), false, "65 streams of one segment");
    std::vector<uint32_t> lead(63, 1);  // 63 one-segment streams: the next stream's FIRST is lane 63
    auto after63 = [&](uint32_t k) {
        std::vector<uint32_t> v = lead;
        v.push_back(k);
        return v;
    };
    straddle(after63(1), false, "FIRST and LAST at lane 63");
    straddle(after63(2), true, "FIRST at lane 63, LAST at lane 64");
    straddle(after63(66), true, "FIRST at lane 63, LAST at lane 128");
    straddle({60, 10}, true, "only the second stream straddles");
    straddle({64, 1}, false, "a single FIRST | LAST segment at lane 64");
}

int main() {
    check({}, 4, 9, "empty");
    check({{0, W, 0, 0}, {3, W, 5, 0}}, 4, 9, "zero-length writes only");
    check({{0, R, 0, 0}}, 1, 0, "a lone reset");
    check({{0, SR, 0, 0}}, 1, 0, "a lone sum-reset");
    check({{0, S, 0, 0}}, 1, 0, "a lone sum");
    check({{0, SR, 0, 0}, {0, SR, 0, 0}, {0, R, 0, 0}, {0, R, 0, 0}}, 1, 0, "consecutive resets");
    check({{0, W, 0, 3}, {0, W, 3, 2}, {0, R, 0, 0}}, 1, 5, "ends in a reset");
    check({{0, SR, 0, 0}, {0, W, 0, 3}, {0, W, 3, 2}}, 1, 5, "starts with a sum-reset");
    check({{0, W, 0, 3}, {0, S, 0, 0}, {0, W, 3, 2}, {0, S, 0, 0}}, 1, 5, "a plain sum does not cut");
    check({{1, W, 0, 1}, {0, SR, 0, 0}, {1, SR, 0, 0}, {0, W, 0, 2}, {1, W, 1, 1}}, 2, 2, "two streams interleaved");
    check({{0, W, 4, 4}, {1, W, 4, 4}, {2, W, 4, 4}, {0, SR, 0, 0}, {1, SR, 0, 0}, {2, SR, 0, 0}}, 3, 8,
          "three nodes, one range");
    // 0-3 writes before the first cut x none / 0-3 between two x 0-3 after, for both cutting kinds
    for (uint32_t cut : {SR, R})
        for (int a = 0; a < 4; a++)
            for (int m = -1; m < 4; m++)
                for (int b = 0; b < 4; b++) {
                    std::vector<Op> ops;
                    for (int k = 0; k < a; k++) ops.push_back({2, W, (uint64_t)k, 1});
                    ops.push_back({2, cut, 0, 0});
                    if (m >= 0) {
                        for (int k = 0; k < m; k++) ops.push_back({2, k ? W : S, (uint64_t)k, k ? 1u : 0u});
                        ops.push_back({2, cut, 0, 0});
                    }
                    for (int k = 0; k < b; k++) ops.push_back({2, W, (uint64_t)k, 1});
                    check(ops, 3, 4, "segment class");
                }
    std::mt19937_64 rng(12);
    for (int round = 0; round < 300; round++) {
        const uint32_t n_streams = 1 + (uint32_t)(rng() % 200);
        const uint64_t arena_len = rng() % 500;
        const uint32_t n_ops = (uint32_t)(rng() % 1500);
        const uint32_t p_write = (uint32_t)(rng() % 90), p_zero = (uint32_t)(rng() % 30);
        std::vector<Op> ops(n_ops);
        for (Op& o : ops) {
            o.stream = (uint32_t)(rng() % n_streams);
            if (rng() % 100 < p_write) {
                o.kind = W;
                o.off = rng() % (arena_len + 1);
                o.len = rng() % 100 < p_zero ? 0u : (uint32_t)(rng() % (arena_len - o.off + 1));
            } else {
                o.kind = 1u + (uint32_t)(rng() % 3);
                o.off = rng();  // ignored
                o.len = (uint32_t)rng();
            }
        }
        check(ops, n_streams, arena_len, "random");
    }
    reject({{0, S, 0, 0}, {4, W, 0, 1}, {1, S, 0, 0}}, 4, 8, MIRSHA_EINVAL, 1, "stream id == n_streams");
    reject({{0, S, 0, 0}, {1, R, 0, 0}, {2, 4, 0, 0}}, 4, 8, MIRSHA_EINVAL, 2, "an unknown kind");
    reject({{0, W, 7, 2}}, 4, 8, MIRSHA_EINVAL, 0, "a range past the arena");
    reject({{0, W, 9, 0}}, 4, 8, MIRSHA_EINVAL, 0, "a zero-length write past the end");
    reject({{0, W, UINT64_MAX, 2}}, 4, 8, MIRSHA_EINVAL, 0, "the sum must not wrap");
    reject({{0, S, 0, 0}}, 0, 0, MIRSHA_EINVAL, 0, "no streams at all");
    {
        const uint32_t s2[2] = {0, 0}, k2[2] = {W, SR}, l2[2] = {1, 0};
        const uint64_t o2[2] = {0, 0};
        uint32_t buf[8], cnt = 0;
        uint64_t buf64[8], nb = 0;
#define CALL(a0, a1, a2, a3, a4, a5, ns) \
    mirsha_stream_seg_plan(s2, k2, o2, l2, 2, 4, 3, 0, a0, a1, a2, a3, a4, a5, ns, &cnt, &cnt, &cnt, &nb, nullptr)
        EXPECT(CALL(nullptr, buf, buf, buf, buf64, buf, &cnt) == MIRSHA_EINVAL, "NULL seg_stream_out");
        EXPECT(CALL(buf, nullptr, buf, buf, buf64, buf, &cnt) == MIRSHA_EINVAL, "NULL sfirst_out");
        EXPECT(CALL(buf, buf, nullptr, buf, buf64, buf, &cnt) == MIRSHA_EINVAL, "NULL seg_flags_out");
        EXPECT(CALL(buf, buf, buf, nullptr, buf64, buf, &cnt) == MIRSHA_EINVAL, "NULL ent_kind_out");
        EXPECT(CALL(buf, buf, buf, buf, nullptr, buf, &cnt) == MIRSHA_EINVAL, "NULL ent_off_out");
        EXPECT(CALL(buf, buf, buf, buf, buf64, nullptr, &cnt) == MIRSHA_EINVAL, "NULL ent_len_out");
        EXPECT(CALL(buf, buf, buf, buf, buf64, buf, nullptr) == MIRSHA_EINVAL, "NULL n_seg_out");
#undef CALL
        EXPECT(mirsha_stream_seg_plan(nullptr, k2, o2, l2, 2, 4, 3, 0, buf, buf, buf, buf, buf64, buf, &cnt, &cnt, &cnt,
                                      &cnt, &nb, nullptr) == MIRSHA_EINVAL, "NULL op_stream");
        EXPECT(mirsha_stream_seg_plan(s2, k2, o2, l2, MIRSHA_STREAM_MAX_OPS + 1u, 4, 3, 0, buf, buf, buf, buf, buf64,
                                      buf, &cnt, &cnt, &cnt, &cnt, &nb, nullptr) == MIRSHA_ERANGE, "too many ops");
        // nothing to plan: no array is needed
        EXPECT(mirsha_stream_seg_plan(nullptr, nullptr, nullptr, nullptr, 0, 4, 3, 0, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, &cnt, &cnt, &cnt, &cnt, &nb, nullptr) == MIRSHA_OK &&
                   cnt == 0, "n_ops = 0 with NULL arrays");
    }
    differential();
    straddles();
    if (fails) return 1;
    printf("stream seg unit ok\n");
    return 0;
}
