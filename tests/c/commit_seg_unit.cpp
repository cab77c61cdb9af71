// commit_seg_unit.cpp -- CPU unit test of mirsha_commit_seg_plan
// (mirbft_amd/csrc/mirsha_host.cpp, compiled here with g++: no HIP, no GPU):
// the segments a commit submission of the ring sends to the device, against a
// restatement built from the ops directly, with guard entries behind every
// output, the segment count's formula, the rejected programmes, and a
// differential check of both commit plans on small random programmes; and
// mirsha::host::seg_straddle against its definition.  Prints
// "commit seg unit ok"; exit 1 with a message at the first mismatch.
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
static const uint32_t kFlag = MIRSHA_COMMIT_ENTRY_CHECKPOINT;

struct Plan {
    std::vector<uint32_t> seg_chain, sfirst, flags, ent;
    uint32_t active = 0, values = 0;
};

// Per chain its ops in op order, nulls dropped, checkpoint rows in op order
// across all chains; each chain's list cut after every checkpoint.
static Plan restate(const std::vector<uint32_t>& oc, const std::vector<uint32_t>& od) {
    std::map<uint32_t, std::vector<uint32_t>> per;
    Plan p;
    for (size_t i = 0; i < oc.size(); i++) {
        if (od[i] == MIRSHA_NULL_INDEX) continue;
        per[oc[i]].push_back(od[i] == MIRSHA_COMMIT_CHECKPOINT ? (kFlag | p.values++) : od[i]);
    }
    p.active = (uint32_t)per.size();
    p.sfirst.push_back(0);
    for (const auto& kv : per) {
        const std::vector<uint32_t>& e = kv.second;
        bool first = true;
        for (size_t k = 0; k < e.size(); k++) {
            p.ent.push_back(e[k]);
            const bool last = k + 1 == e.size();
            if ((e[k] & kFlag) || last) {
                p.seg_chain.push_back(kv.first);
                p.flags.push_back((first ? MIRSHA_COMMIT_SEG_FIRST : 0u) | (last ? MIRSHA_COMMIT_SEG_LAST : 0u));
                p.sfirst.push_back((uint32_t)p.ent.size());
                first = false;
            }
        }
    }
    return p;
}

static void check(const std::vector<uint32_t>& oc, const std::vector<uint32_t>& od, uint32_t n_chains,
                  uint32_t n_digests, const char* what) {
    const uint32_t n = (uint32_t)oc.size();
    std::vector<uint32_t> seg_chain(n + 1, kGuard), sfirst(n + 2, kGuard), flags(n + 1, kGuard), ent(n + 1, kGuard);
    uint32_t ns = kGuard, na = kGuard, ne = kGuard, nv = kGuard, bad = kGuard;
    const int rc = mirsha_commit_seg_plan(n ? oc.data() : nullptr, n ? od.data() : nullptr, n, n_chains, n_digests,
                                          seg_chain.data(), sfirst.data(), flags.data(), ent.data(), &ns, &na, &ne,
                                          &nv, &bad);
    EXPECT(rc == MIRSHA_OK && bad == UINT32_MAX, "%s: rc %d bad %u", what, rc, bad);
    if (rc != MIRSHA_OK) return;
    const Plan w = restate(oc, od);
    EXPECT(ns == w.seg_chain.size() && na == w.active && ne == w.ent.size() && nv == w.values,
           "%s: counts %u %u %u %u", what, ns, na, ne, nv);
    if (ns != w.seg_chain.size() || ne != w.ent.size()) return;
    EXPECT(seg_chain[ns] == kGuard && flags[ns] == kGuard && ent[ne] == kGuard && sfirst[ns + 1] == kGuard,
           "%s: wrote past its outputs", what);
    bool ok = true;
    for (uint32_t s = 0; s < ns; s++)
        ok &= seg_chain[s] == w.seg_chain[s] && flags[s] == w.flags[s] && sfirst[s] == w.sfirst[s];
    ok &= sfirst[ns] == ne;
    for (uint32_t e = 0; e < ne; e++) ok &= ent[e] == w.ent[e];
    EXPECT(ok, "%s: plan differs", what);
    // n_seg = active chains + checkpoint entries that are not their chain's final entry
    uint32_t inner = 0;
    for (uint32_t s = 0; s < ns; s++)
        if (!(flags[s] & MIRSHA_COMMIT_SEG_LAST)) inner++;
    uint32_t counted = 0;
    for (uint32_t s = 0; s < ns; s++) {
        const bool ends_cp = (ent[sfirst[s + 1] - 1] & kFlag) != 0;
        if (ends_cp && !(flags[s] & MIRSHA_COMMIT_SEG_LAST)) counted++;
        EXPECT(sfirst[s + 1] > sfirst[s], "%s: segment %u is empty", what, s);
        EXPECT(ends_cp || (flags[s] & MIRSHA_COMMIT_SEG_LAST), "%s: segment %u ends nowhere", what, s);
        for (uint32_t e = sfirst[s]; e + 1 < sfirst[s + 1]; e++)
            EXPECT(!(ent[e] & kFlag), "%s: a checkpoint inside segment %u", what, s);
    }
    EXPECT(ns == na + inner && inner == counted, "%s: n_seg %u != %u + %u", what, ns, na, inner);
}

static void reject(const std::vector<uint32_t>& oc, const std::vector<uint32_t>& od, uint32_t n_chains,
                   uint32_t n_digests, int want_rc, uint32_t want_bad, const char* what) {
    const uint32_t n = (uint32_t)oc.size();
    std::vector<uint32_t> seg_chain(n + 1, kGuard), sfirst(n + 2, kGuard), flags(n + 1, kGuard), ent(n + 1, kGuard);
    uint32_t ns = kGuard, na = kGuard, ne = kGuard, nv = kGuard, bad = kGuard;
    const int rc = mirsha_commit_seg_plan(oc.data(), od.data(), n, n_chains, n_digests, seg_chain.data(),
                                          sfirst.data(), flags.data(), ent.data(), &ns, &na, &ne, &nv, &bad);
    EXPECT(rc == want_rc && bad == want_bad, "%s: rc %d bad %u", what, rc, bad);
    EXPECT(ns == 0, "%s: n_seg %u after a failure", what, ns);
    EXPECT(seg_chain[n] == kGuard && flags[n] == kGuard && ent[n] == kGuard && sfirst[n + 1] == kGuard,
           "%s: wrote past its outputs", what);
}

// ---- Differential check of mirsha_commit_plan and mirsha_commit_seg_plan: every
// array (guards included: nothing is written before every op has passed),
// every count, the code and the bad op, against a plain restatement -- the
// argument checks in their order, a per-chain std::vector append in op order,
// then a cut.
struct Out {
    int rc = 0;
    uint32_t ns = kGuard, na = kGuard, ne = kGuard, nv = kGuard, bad = kGuard;
    std::vector<uint32_t> act, efirst, seg_chain, sfirst, flags, ent;
    explicit Out(uint32_t cap)
        : act(cap + 2, kGuard), efirst(cap + 2, kGuard), seg_chain(cap + 2, kGuard), sfirst(cap + 2, kGuard),
          flags(cap + 2, kGuard), ent(cap + 2, kGuard) {}
    bool operator==(const Out& o) const {
        return rc == o.rc && ns == o.ns && na == o.na && ne == o.ne && nv == o.nv && bad == o.bad && act == o.act &&
               efirst == o.efirst && seg_chain == o.seg_chain && sfirst == o.sfirst && flags == o.flags && ent == o.ent;
    }
};

static Out model(bool seg, const uint32_t* oc, const uint32_t* od, uint32_t n, uint32_t n_chains, uint32_t n_digests,
                 bool outputs, uint32_t cap) {
    Out w(cap);
    w.bad = UINT32_MAX;
    w.na = w.ne = w.nv = 0;
    if (seg) w.ns = 0;
    std::vector<uint32_t>& first = seg ? w.sfirst : w.efirst;
    w.rc = MIRSHA_EINVAL;
    if (n > kFlag || n_digests > kFlag) {
        w.rc = MIRSHA_ERANGE;
        return w;
    }
    if (n == 0) {
        w.rc = MIRSHA_OK;
        if (outputs) first[0] = 0;
        return w;
    }
    if (!oc || !od) return w;
    for (uint32_t i = 0; i < n; i++) {
        const bool marker = od[i] == MIRSHA_NULL_INDEX || od[i] == MIRSHA_COMMIT_CHECKPOINT;
        if (oc[i] >= n_chains || (!marker && od[i] >= n_digests)) {
            w.bad = i;
            return w;
        }
    }
    if (!outputs) return w;
    std::vector<std::vector<uint32_t>> per(n_chains);
    for (uint32_t i = 0; i < n; i++)
        if (od[i] != MIRSHA_NULL_INDEX) per[oc[i]].push_back(od[i] == MIRSHA_COMMIT_CHECKPOINT ? (kFlag | w.nv++) : od[i]);
    w.rc = MIRSHA_OK;
    first[0] = 0;
    for (uint32_t c = 0; c < n_chains; c++) {
        const uint32_t e0 = w.ne;
        for (size_t k = 0; k < per[c].size(); k++) {
            w.ent[w.ne++] = per[c][k];
            const bool last = k + 1 == per[c].size();
            if (!seg || !((per[c][k] & kFlag) || last)) continue;
            w.seg_chain[w.ns] = c;
            // FIRST: no cut of this chain yet, so the segment begins at the chain's first entry
            w.flags[w.ns] = (w.sfirst[w.ns] == e0 ? MIRSHA_COMMIT_SEG_FIRST : 0u) | (last ? MIRSHA_COMMIT_SEG_LAST : 0u);
            w.sfirst[++w.ns] = w.ne;
        }
        if (per[c].empty()) continue;
        if (!seg) {
            w.act[w.na] = c;
            w.efirst[w.na + 1] = w.ne;
        }
        w.na++;
    }
    return w;
}

static void differ(const uint32_t* oc, const uint32_t* od, uint32_t n, uint32_t n_chains, uint32_t n_digests,
                   bool outputs, uint32_t cap, const char* what) {
    for (int seg = 0; seg < 2; seg++) {
        Out g(cap);
        auto p = [&](std::vector<uint32_t>& v) { return outputs ? v.data() : nullptr; };
        g.rc = seg ? mirsha_commit_seg_plan(oc, od, n, n_chains, n_digests, p(g.seg_chain), p(g.sfirst), p(g.flags),
                                            p(g.ent), &g.ns, &g.na, &g.ne, &g.nv, &g.bad)
                   : mirsha_commit_plan(oc, od, n, n_chains, n_digests, p(g.act), p(g.efirst), p(g.ent), &g.na, &g.ne,
                                        &g.nv, &g.bad);
        const Out w = model(seg != 0, oc, od, n, n_chains, n_digests, outputs, cap);
        EXPECT(g == w, "%s (%s plan, %u ops): rc %d/%d bad %u/%u counts %u %u %u %u / %u %u %u %u", what,
               seg ? "seg" : "commit", n, g.rc, w.rc, g.bad, w.bad, g.ns, g.na, g.ne, g.nv, w.ns, w.na, w.ne, w.nv);
    }
}

static void differential() {
    const uint32_t CP = MIRSHA_COMMIT_CHECKPOINT, NUL = MIRSHA_NULL_INDEX;
    std::mt19937_64 rng(21);
    for (int round = 0; round < 4000; round++) {
        const uint32_t n_chains = 1 + (uint32_t)(rng() % 5), n_digests = (uint32_t)(rng() % 9);
        const uint32_t n = (uint32_t)(rng() % 41);
        std::vector<uint32_t> oc(n), od(n);
        for (uint32_t i = 0; i < n; i++) {
            oc[i] = (uint32_t)(rng() % n_chains);
            const uint32_t k = (uint32_t)(rng() % 8);
            od[i] = k == 0 ? NUL : (k < 3 || n_digests == 0) ? CP : (uint32_t)(rng() % n_digests);
        }
        const uint32_t cls = (uint32_t)(rng() % 12), at = n ? (uint32_t)(rng() % n) : 0u;
        const uint32_t *pc = oc.data(), *pd = od.data();
        bool outputs = true;
        uint32_t nd = n_digests;
        const char* what = "differential: a valid programme";
        if (n && cls == 6) oc[at] = n_chains + (uint32_t)(rng() % 3), what = "differential: a bad chain";
        if (n && cls == 7) od[at] = n_digests + (uint32_t)(rng() % 3), what = "differential: a bad digest index";
        if (cls == 8) (rng() & 1 ? pc : pd) = nullptr, what = "differential: a NULL op array";
        if (cls == 9) outputs = false, what = "differential: NULL outputs";
        if (cls == 10) {  // with a bad op: the inner plan's code and bad op come first
            outputs = false, what = "differential: NULL outputs and a bad op";
            if (n) (rng() & 1 ? oc[at] = n_chains : od[at] = CP - 1u);
        }
        if (cls == 11 && round % 8 == 0) nd = kFlag + 1u, what = "differential: too many digests";
        differ(pc, pd, n, n_chains, nd, outputs, n, what);
    }
    const uint32_t one[1] = {0};
    differ(one, one, kFlag + 1u, 4, 3, true, 0, "differential: too many ops");  // refused before an array is read
    differ(one, one, kFlag + 1u, 4, 3, false, 0, "differential: too many ops, NULL outputs");
}

// ---- mirsha::host::seg_straddle over the flags of owners with the given segment
// counts, against the definition: a LAST lane whose wave index differs from
// its owner's FIRST lane's.
static void straddle(const std::vector<uint32_t>& seg_counts, bool want, const char* what) {
    std::vector<uint32_t> flags;
    for (uint32_t k : seg_counts)
        for (uint32_t j = 0; j < k; j++)
            flags.push_back((j == 0 ? MIRSHA_COMMIT_SEG_FIRST : 0u) | (j + 1 == k ? MIRSHA_COMMIT_SEG_LAST : 0u));
    bool def = false;
    for (size_t s = 0, first = 0; s < flags.size(); s++) {
        if (flags[s] & MIRSHA_COMMIT_SEG_FIRST) first = s;
        if ((flags[s] & MIRSHA_COMMIT_SEG_LAST) && s / 64 != first / 64) def = true;
    }
    EXPECT(def == want, "%s: the definition says %d", what, (int)def);
    EXPECT(mirsha::host::seg_straddle(flags.data(), (uint32_t)flags.size(), 64) == want, "%s: not %d", what, (int)want);
}

static void straddles() {
    EXPECT(!mirsha::host::seg_straddle(nullptr, 0, 64), "no segments");
    straddle({1}, false, "one segment");
    straddle({64}, false, "one chain over exactly one wave");
    straddle({65}, true, "one chain over 65 lanes");
    straddle(std::vector<uint32_t>(64, 1), false, "64 chains of one segment");
    straddle(std::vector<uint32_t>(65, 1), false, "65 chains of one segment");
    std::vector<uint32_t> lead(63, 1);  // 63 one-segment chains: the next chain's FIRST is lane 63
    auto after63 = [&](uint32_t k) {
        std::vector<uint32_t> v = lead;
        v.push_back(k);
        return v;
    };
    straddle(after63(1), false, "FIRST and LAST at lane 63");
    straddle(after63(2), true, "FIRST at lane 63, LAST at lane 64");
    straddle(after63(66), true, "FIRST at lane 63, LAST at lane 128");
    straddle({60, 10}, true, "only the second chain straddles");
    straddle({64, 1}, false, "a single FIRST | LAST segment at lane 64");
}

int main() {
    const uint32_t CP = MIRSHA_COMMIT_CHECKPOINT, NUL = MIRSHA_NULL_INDEX;
    check({}, {}, 4, 9, "empty");
    check({0, 3, 3}, {NUL, NUL, NUL}, 4, 0, "nulls only");
    check({0}, {CP}, 1, 0, "a lone checkpoint");
    check({0, 0}, {CP, CP}, 1, 0, "two checkpoints back to back");
    check({0, 0, 0}, {1, 2, CP}, 1, 3, "ends in a checkpoint");
    check({0, 0, 0}, {CP, 1, 2}, 1, 3, "starts with a checkpoint");
    check({1, 0, 1, 0, 1}, {0, CP, CP, 0, 0}, 2, 1, "two chains interleaved");
    // the parity classes: 0-3 writes before the first checkpoint x none / 0-3 between two x 0-3 after
    for (int a = 0; a < 4; a++)
        for (int m = -1; m < 4; m++)
            for (int b = 0; b < 4; b++) {
                std::vector<uint32_t> od;
                for (int k = 0; k < a; k++) od.push_back(k);
                od.push_back(CP);
                if (m >= 0) {
                    for (int k = 0; k < m; k++) od.push_back(k);
                    od.push_back(CP);
                }
                for (int k = 0; k < b; k++) od.push_back(k);
                check(std::vector<uint32_t>(od.size(), 2), od, 3, 4, "parity class");
            }
    std::mt19937_64 rng(11);
    for (int round = 0; round < 300; round++) {
        const uint32_t n_chains = 1 + (uint32_t)(rng() % 200), n_digests = (uint32_t)(rng() % 50);
        const uint32_t n_ops = (uint32_t)(rng() % 1500);
        const uint32_t p_null = (uint32_t)(rng() % 40), p_cp = (uint32_t)(rng() % 50);
        std::vector<uint32_t> oc(n_ops), od(n_ops);
        for (uint32_t i = 0; i < n_ops; i++) {
            oc[i] = (uint32_t)(rng() % n_chains);
            const uint32_t k = (uint32_t)(rng() % 100);
            if (k < p_null) od[i] = NUL;
            else if (k >= 100 - p_cp || n_digests == 0) od[i] = CP;
            else od[i] = (uint32_t)(rng() % n_digests);
        }
        check(oc, od, n_chains, n_digests, "random");
    }
    reject({0, 4, 1}, {0, 1, 2}, 4, 3, MIRSHA_EINVAL, 1, "chain id == n_chains");
    reject({0, 1, 2}, {0, 3, 1}, 4, 3, MIRSHA_EINVAL, 1, "digest index == n_digests");
    reject({0, 1, 2}, {0, 1, CP - 1}, 4, 3, MIRSHA_EINVAL, 2, "just below the markers");
    reject({0, 9}, {NUL, NUL}, 4, 0, MIRSHA_EINVAL, 1, "a null write still names a chain");
    reject({0}, {CP}, 0, 0, MIRSHA_EINVAL, 0, "no chains at all");
    reject({0}, {0}, 4, kFlag + 1u, MIRSHA_ERANGE, UINT32_MAX, "too many digests");
    {
        const uint32_t one[2] = {0, 0};
        uint32_t buf[8], cnt = 0;
        EXPECT(mirsha_commit_seg_plan(one, one, 2, 4, 3, nullptr, buf, buf, buf, &cnt, &cnt, &cnt, &cnt, nullptr) ==
                   MIRSHA_EINVAL, "NULL seg_chain_out");
        EXPECT(mirsha_commit_seg_plan(one, one, 2, 4, 3, buf, nullptr, buf, buf, &cnt, &cnt, &cnt, &cnt, nullptr) ==
                   MIRSHA_EINVAL, "NULL sfirst_out");
        EXPECT(mirsha_commit_seg_plan(one, one, 2, 4, 3, buf, buf, nullptr, buf, &cnt, &cnt, &cnt, &cnt, nullptr) ==
                   MIRSHA_EINVAL, "NULL seg_flags_out");
        EXPECT(mirsha_commit_seg_plan(one, one, 2, 4, 3, buf, buf, buf, nullptr, &cnt, &cnt, &cnt, &cnt, nullptr) ==
                   MIRSHA_EINVAL, "NULL ent_out");
        EXPECT(mirsha_commit_seg_plan(one, one, 2, 4, 3, buf, buf, buf, buf, nullptr, &cnt, &cnt, &cnt, nullptr) ==
                   MIRSHA_EINVAL, "NULL n_seg_out");
        EXPECT(mirsha_commit_seg_plan(nullptr, one, 2, 4, 3, buf, buf, buf, buf, &cnt, &cnt, &cnt, &cnt, nullptr) ==
                   MIRSHA_EINVAL, "NULL op_chain");
        // nothing to plan: no array is needed
        EXPECT(mirsha_commit_seg_plan(nullptr, nullptr, 0, 4, 3, nullptr, nullptr, nullptr, nullptr, &cnt, &cnt, &cnt,
                                      &cnt, nullptr) == MIRSHA_OK && cnt == 0, "n_ops = 0 with NULL arrays");
    }
    differential();
    straddles();
    if (fails) return 1;
    printf("commit seg unit ok\n");
    return 0;
}
